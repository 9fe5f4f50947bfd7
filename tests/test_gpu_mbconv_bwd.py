"""The reverse chain of an MBConv block, kernel form by kernel form against float64 autograd on the CPU:

    depthwise data gradient      dwconv_dgrad_s2_kernel (stride 2: all four padding parities x both K, plain / +BN / +BN+filter
                                 gradient) and the forward forms over dy with flipped taps (stride 1: LDS, window with the filter
                                 gradient, the fallbacks that refuse)        orbit_op_dwconv2d_backward / orbit_op_dwconv2d_dgrad_bn
    depthwise filter gradient    global-load form and the LDS form with the input transform
                                                                             orbit_op_dwconv2d_backward / orbit_op_dwconv2d_wgrad_xf
    squeeze-excite backward      gate_bwd_apply_bn_kernel (g written / sums only), then bn_bwd_apply_kernel or
    + BatchNorm backward         gate_bn_bwd_apply_kernel                    orbit_op_se_gate_backward_bn

Every case asks orbit_op_dwconv2d_backward_plan first and asserts the kernel family, what is carried and the partial-row counts the
case is named after; a layer the launchers refuse is asserted as a refusal (ORBIT_ERR_ARG, the message, every output untouched).
Every output is NaN-prefilled and followed by a guard tail of sentinel floats. All maps are non-square with TF-SAME padding.

Bounds (u = 2^-24; E32 = the largest error of the same graph evaluated in float32 on the CPU, on that tensor):
  elementwise dx / g / dy     err <= max(2e-5, 4 E32) max(1, max |ref64|)                     (elementwise_gate)
  sum g, sum g xhat per c     against the float64 sums of the g THE KERNEL WROTE (xhat in float64 from the fp32 y, mean, invstd):
                              2 (n + 2) u A, n terms, A the float64 sum of their magnitudes - twice any order's summation bound
                              plus the rounding of the product and of xhat
  filter gradient per (c,tap) 2 n u A + 4 E32, A = sum |dy x| over the entry's n terms (4 E32: the fast exp / rcp of the staged
                              activation)
  dgamma, dbeta, SE grads     max(4 E32, 8 u max |ref64|)                                      (tests/test_gpu_vit_ops.py)
Input families: Gaussian; one_sign (dy > 0, taps > 0, z = y scale + shift in [0.5, 2.5], mean below every y: every term of every
checked sum is positive); ReLU inputs keep |z| >= 1e-3 (no mask can flip). On the one_sign inputs one dropped or doubled term moves
a sum by more than its bound wherever n^2 stays below (min term / mean term) / 2u - about a thousand terms; the bound grows with
n^2, so the sums of NO_MARGIN (listed below) are gated by the same bound without that margin (tests/test_mbconv_bwd_reference.py).

Each check prints "[mbconv_bwd] family: case: err, bound, ratio" (pytest -s)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
import test_gpu_se_path as S  # noqa: E402
from test_gpu_se_path import GUARD, LDS, PIPE, SENTINEL, STREAM, U, WINDOW, Guarded, nhwc, options, same_pad  # noqa: E402

_report = functools.partial(S._report, tag="mbconv_bwd")
elementwise_gate = functools.partial(S.elementwise_gate, report=_report)

NONE, RELU, SILU = 0, 1, 2
# orbit_op_dwconv2d_backward_plan: modes and the families beyond the four forward forms (include/orbit_hip.h)
DGRAD, DGRAD_BN, DGRAD_BN_WG, WGRAD, WGRAD_XF = range(5)
FAM_S2, FAM_GATHER, FAM_WG_GLOBAL, FAM_WG_LDS = 4, 5, 6, 7
ERR_ARG = -1
DEFAULT_OPTS = (1, 1, 1)  # dw_window, dw_lds, dw_pipe


def _st():
    return _lib.stream_handle()


def layer(H, W, K, stride):
    """(Ho, Wo, pad_top, pad_left, pad_bottom, pad_right) of TF-SAME."""
    Ho, th, pt = same_pad(H, K, stride)
    Wo, tw, pl = same_pad(W, K, stride)
    return Ho, Wo, pt, pl, th - pt, tw - pl


def bwd_plan(lib, B, C, H, W, K, stride, mode):
    Ho, Wo, pt, pl, _, _ = layer(H, W, K, stride)
    p = _lib.DwconvBackwardPlan()
    _lib.check(lib.orbit_op_dwconv2d_backward_plan(B, H, W, C, K, stride, pt, pl, Ho, Wo, mode, ctypes.byref(p)),
               "orbit_op_dwconv2d_backward_plan")
    return p


def assert_untouched(buf, what):
    flat, n = buf.flat.cpu(), buf.t.numel()
    assert torch.isnan(flat[:n]).all(), "%s: written by a refused call" % what
    assert torch.equal(flat[n:], torch.full((GUARD,), SENTINEL)), "%s: guard tail written by a refused call" % what


# ---- inputs and references ----------------------------------------------------------------------------------------------------------
def act_fn(z, act):
    return F.silu(z) if act == SILU else F.relu(z) if act == RELU else z


def keep_off_zero(z):
    """|z| >= 2e-3: the ReLU inputs (after the round trip through y the recomputed z stays beyond 1e-3)."""
    return torch.where(z.abs() < 2e-3, torch.where(z < 0, torch.full_like(z, -2e-3), torch.full_like(z, 2e-3)), z)


def nchw_c(v):
    return v.view(1, -1, 1, 1)


def nlc(v):
    return v.view(1, 1, -1)


def dw_inputs(family, B, C, H, W, K, stride, act, seed):
    """A depthwise layer behind BatchNorm + act: raw y NCHW, folded scale / shift, mean / invstd, taps w, output gradient dy."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = layer(H, W, K, stride)[:2]
    if family == "one_sign":
        z = torch.rand(B, C, H, W, generator=g) * 1.9 + 0.55
        w = (torch.rand(C, 1, K, K, generator=g) * 0.5 + 0.75) / (K * K)
        dy = torch.rand(B, C, Ho, Wo, generator=g) * 0.5 + 0.75
    else:
        z = torch.randn(B, C, H, W, generator=g) * 1.5
        if act == RELU:
            z = keep_off_zero(z)
        w = torch.randn(C, 1, K, K, generator=g) / K
        dy = torch.randn(B, C, Ho, Wo, generator=g)
    scale = torch.rand(C, generator=g) + 0.5
    if family == "one_sign":
        shift = torch.rand(C, generator=g) * 0.5
        y = (z - nchw_c(shift)) / nchw_c(scale)
        mean = y.transpose(0, 1).reshape(C, -1).min(1).values - (torch.rand(C, generator=g) + 0.5)  # xhat > 0
    else:
        shift = torch.randn(C, generator=g) * 0.3 + 0.2
        y = (z - nchw_c(shift)) / nchw_c(scale)
        mean = torch.randn(C, generator=g) * 0.2
    return {"y": y, "w": w, "dy": dy, "scale": scale, "shift": shift, "mean": mean, "invstd": torch.rand(C, generator=g) + 0.5}


def dw_ref(t, K, stride, act, dtype):
    """Autograd through act(y * scale + shift) -> depthwise conv: the activated input a, dx = d/da, g = d/dz, dw."""
    y, w, dy, scale, shift = (t[k].to(dtype) for k in ("y", "w", "dy", "scale", "shift"))
    H, W = y.shape[2:]
    _, _, pt, pl, pb, pr = layer(H, W, K, stride)
    z = (y * nchw_c(scale) + nchw_c(shift)).requires_grad_(True)
    a = act_fn(z, act)
    a.retain_grad()
    w = w.clone().requires_grad_(True)
    out = F.conv2d(F.pad(a, [pl, pr, pt, pb]), w, None, stride, 0, 1, y.shape[1])
    assert out.shape == dy.shape
    out.backward(dy)
    return {"z": z.detach(), "a": a.detach(), "dx": a.grad, "g": z.grad, "dw": w.grad}


def wgrad_terms(t, a64, K, stride):
    """Per (channel, tap): A = the float64 sum of |dy * x| and n = the number of its terms that lie inside the map."""
    B, C, H, W = a64.shape
    Ho, Wo, pt, pl, pb, pr = layer(H, W, K, stride)
    w = torch.zeros(C, 1, K, K, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.pad(a64.abs(), [pl, pr, pt, pb]), w, None, stride, 0, 1, C).backward(t["dy"].double().abs())
    rows = torch.tensor([sum(1 for o in range(Ho) if 0 <= o * stride - pt + k < H) for k in range(K)], dtype=torch.float64)
    cols = torch.tensor([sum(1 for o in range(Wo) if 0 <= o * stride - pl + k < W) for k in range(K)], dtype=torch.float64)
    return w.grad, (B * rows[:, None] * cols[None, :]).view(1, 1, K, K)


@functools.lru_cache(maxsize=4)
def dw_case(family, B, C, H, W, K, stride, act):
    """Inputs and both references of a depthwise case, computed once and shared by the modes that run on it."""
    t = dw_inputs(family, B, C, H, W, K, stride, act, seed=B + C + 3 * H + 5 * W + 7 * K + stride + act)
    r64, r32 = dw_ref(t, K, stride, act, torch.float64), dw_ref(t, K, stride, act, torch.float32)
    A, n = wgrad_terms(t, r64["a"], K, stride)
    return t, r64, r32, A, n


# ---- checks ---------------------------------------------------------------------------------------------------------------------------
def check_channel_sums(family, what, sums, g_written, y, mean, invstd, cdim):
    """sums [2][C] against the float64 sums of the g the kernel wrote and of g * xhat, per channel: 2 (n + 2) u A."""
    shape = [1] * g_written.dim()
    shape[cdim] = -1
    gd = g_written.double()
    xhat = (y.double() - mean.double().view(*shape)) * invstd.double().view(*shape)
    dims = [d for d in range(gd.dim()) if d != cdim]
    n = gd.numel() // gd.shape[cdim]
    for k, terms in enumerate((gd, gd * xhat)):
        S_, A = terms.sum(dims), terms.abs().sum(dims)
        bound = 2.0 * (n + 2) * U * A
        err = (sums[k].double() - S_).abs()
        _report(family, "%s: sum %s" % (what, "g xhat" if k else "g"), (err / bound).max().item(), 1.0)
        assert not (err > bound).any(), (what, k, err.max().item(), bound.min().item())


def check_wgrad(family, what, got, dw64, dw32, A, n):
    """Filter gradient per (channel, tap): 2 n u A + 4 E32."""
    e32 = (dw32.double() - dw64).abs().max().item()
    bound = 2.0 * n * U * A + 4.0 * e32
    err = (got.double() - dw64).abs()
    _report(family, what, (err / bound).max().item(), 1.0)
    assert not (err > bound).any(), (what, err.max().item(), bound.min().item(), e32)


def param_gate(family, what, got, want64, want32):
    e32 = (want32.double() - want64).abs().max().item()
    tol = max(4.0 * e32, 8.0 * U * want64.abs().max().item())
    err = (got.double() - want64).abs().max().item()
    _report(family, what, err, tol)
    assert err <= tol, (what, err, tol, e32)


# ---- a / b. the depthwise data gradient -------------------------------------------------------------------------------------------
# name, B, C, H, W, K, (PT, PL), row blocks of the launch: plain, +BN, +BN+filter gradient (= the partial rows of the last two).
# Block layout: G = min(C / 4, 64) channel quads x R = 256 / G row lanes, each lane walks 2x2 blocks of dx.
S2_CASES = [
    ("k3_p00", 2, 24, 16, 14, 3, (0, 0), 3, 3, 1),           # G = 6, R = 42: 4 idle threads
    ("k3_p01", 2, 96, 16, 13, 3, (0, 1), 12, 12, 2),         # mixed parity; odd W: clamped yq, `inside` false in the last column
    ("k3_p10", 3, 144, 15, 14, 3, (1, 0), 24, 24, 6),        # mixed parity; G = 36, R = 7; odd H
    ("k3_p11", 2, 40, 15, 13, 3, (1, 1), 5, 5, 2),           # G = 10, R = 25
    ("k5_p11", 2, 40, 16, 14, 5, (1, 1), 5, 5, 1),
    ("k5_p10", 1, 1152, 16, 13, 5, (1, 0), 14, 14, 1),       # mixed; 5 column groups, the last with 32 of 64 quads
    ("k5_p01", 2, 144, 15, 14, 5, (0, 1), 16, 16, 2),        # mixed (pads 2, 1)
    ("k5_p00", 3, 96, 33, 21, 5, (0, 0), 57, 57, 9),         # 561 2x2 blocks; 9 fused rows: several strides per thread
    ("capped", 20, 256, 42, 40, 3, (0, 0), 2100, 2048, 350),  # 8400 blocks > 2048 R: the +BN mode takes a second grid stride
]
S2_IDS = [c[0] for c in S2_CASES]

# name, B, C, H, W, K, options, form, rows of the chunks, +BN carried, filter gradient carried
S1_CASES = [
    ("lds_k5", 3, 240, 17, 13, 5, DEFAULT_OPTS, LDS, [7, 7, 3], True, False),          # Wo % 4 = 1
    ("lds_k3", 1, 1152, 13, 9, 3, DEFAULT_OPTS, LDS, [13], True, False),
    ("lds_k5_7", 3, 128, 7, 6, 5, DEFAULT_OPTS, LDS, [7], True, False),                # 16-quad slices
    ("win_wg_c48", 2, 48, 30, 27, 3, DEFAULT_OPTS, WINDOW, [7, 7, 7, 7, 2], True, True),   # W % 4 = 3; cb4 12
    ("win_wg_c1152", 1, 1152, 17, 13, 3, DEFAULT_OPTS, WINDOW, [7, 7, 3], True, True),     # 6 channel slices, cb4 48, 16 idle threads
    ("win_wg_c32", 3, 32, 57, 6, 3, DEFAULT_OPTS, WINDOW, [8] * 7 + [1], True, True),      # rpc 8; the last chunk is one row
    ("unfit_k5_c40", 3, 40, 15, 10, 5, DEFAULT_OPTS, STREAM, [7, 7, 1], False, False),     # no LDS slice divides C / 4 = 10
    ("unfit_k3_c40", 1, 40, 14, 6, 3, DEFAULT_OPTS, WINDOW, [7, 7], True, False),          # window as the LDS rule's fallback
    ("pipe_forced", 3, 32, 15, 6, 3, (0, 0, 2), PIPE, [7, 7, 1], False, False),
]
S1_IDS = [c[0] for c in S1_CASES]

# mode name, plan mode, activation, input families
DGRAD_MODES = [("plain", DGRAD, NONE, ("normal",)), ("bn_silu", DGRAD_BN, SILU, ("normal", "one_sign")),
               ("bn_none", DGRAD_BN, NONE, ("normal", "one_sign")), ("bn_wg_silu", DGRAD_BN_WG, SILU, ("normal", "one_sign"))]
MODE_IDS = [m[0] for m in DGRAD_MODES]

# sums whose n is too large for the one-term margin of the one_sign family (see the module docstring): case name -> which sums
# ("g/silu", "g/none": sum g and sum g xhat behind that activation; "dw": the filter gradient)
ALL_SUMS = ("g/silu", "g/none", "dw")
NO_MARGIN = {"capped": ALL_SUMS, "k5_p00": ("g/silu", "g/none"), "win_wg_c48": ALL_SUMS, "win_wg_c32": ("g/silu",),
             "xf_13x66": ("dw",), "xf_tpb2": ("dw",), "se_capped": ("g/silu",)}


def run_dgrad(lib, device, what, t, r64, r32, A, n, B, C, H, W, K, stride, mode, act, family, refused):
    """One data-gradient call in `mode`; checks every output, or the refusal."""
    Ho, Wo, pt, pl, _, _ = layer(H, W, K, stride)
    d = _lib.dptr
    dev = {k: (nhwc(v) if v.dim() == 4 and k != "w" else v).to(device).contiguous() for k, v in t.items()}
    if mode == DGRAD:
        a = nhwc(r32["a"]).to(device).contiguous()
        dx = Guarded((B, H, W, C), device)
        _lib.check(lib.orbit_op_dwconv2d_backward(d(a), d(dev["w"]), d(dev["dy"]), d(dx.t), None, B, H, W, C, K, stride, pt, pl, Ho, Wo,
                                                  _st()), "orbit_op_dwconv2d_backward")
        torch.cuda.synchronize()
        elementwise_gate("dgrad_s%d_dx" % stride, what, dx.cpu("dx").permute(0, 3, 1, 2), r64["dx"], r32["dx"])
        return
    g, sums = Guarded((B, H, W, C), device), Guarded((2, C), device)
    dw = Guarded((C, 1, K, K), device) if mode == DGRAD_BN_WG else None
    rc = lib.orbit_op_dwconv2d_dgrad_bn(d(dev["dy"]), d(dev["w"]), d(dev["y"]), d(dev["mean"]), d(dev["invstd"]), d(dev["scale"]),
                                        d(dev["shift"]), act, d(g.t), d(sums.t), d(dw.t) if dw else None, B, H, W, C, K, stride, pt, pl,
                                        Ho, Wo, _st())
    torch.cuda.synchronize()
    if refused:
        assert rc == ERR_ARG, (what, rc)
        msg = _lib.last_error()
        assert "op_dwconv2d_dgrad_bn" in msg and refused in msg, msg
        for buf, name in ((g, "g"), (sums, "sums"), (dw, "dw")):
            if buf is not None:
                assert_untouched(buf, "%s: %s" % (what, name))
        return
    _lib.check(rc, "orbit_op_dwconv2d_dgrad_bn")
    got_g = g.cpu("g").permute(0, 3, 1, 2)
    elementwise_gate("dgrad_s%d_g" % stride, what, got_g, r64["g"], r32["g"])
    check_channel_sums("dgrad_s%d_sums" % stride, what, sums.cpu("sums"), got_g, t["y"], t["mean"], t["invstd"], 1)
    if dw is not None:
        check_wgrad("dgrad_s%d_dw" % stride, what, dw.cpu("dw"), r64["dw"], r32["dw"], A, n)


@pytest.mark.parametrize("mname,mode,act,families", DGRAD_MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,B,C,H,W,K,par,blocks,bn_rows,wg_rows", S2_CASES, ids=S2_IDS)
def test_stride2_data_gradient(lib, device, name, B, C, H, W, K, par, blocks, bn_rows, wg_rows, mname, mode, act, families):
    Ho, Wo, pt, pl, _, _ = layer(H, W, K, 2)
    assert (pt & 1, pl & 1) == par and H != W
    p = bwd_plan(lib, B, C, H, W, K, 2, mode)
    assert p.family == FAM_S2
    assert (p.epilogue, p.wgrad) == (int(mode != DGRAD), int(mode == DGRAD_BN_WG))
    assert (p.blocks, p.bn_rows, p.wgrad_rows) == {DGRAD: (blocks, 0, 0), DGRAD_BN: (bn_rows, bn_rows, 0),
                                                   DGRAD_BN_WG: (wg_rows, wg_rows, wg_rows)}[mode]
    for family in families:
        t, r64, r32, A, n = dw_case(family, B, C, H, W, K, 2, act)
        run_dgrad(lib, device, "%s/%s/%s" % (name, mname, family), t, r64, r32, A, n, B, C, H, W, K, 2, mode, act, family, None)


def test_stride2_data_gradient_relu(lib, device):
    name, B, C, H, W, K = S2_CASES[0][:6]
    for mname, mode in (("bn_relu", DGRAD_BN), ("bn_wg_relu", DGRAD_BN_WG)):
        p = bwd_plan(lib, B, C, H, W, K, 2, mode)
        assert p.family == FAM_S2 and p.epilogue == 1 and p.wgrad == int(mode == DGRAD_BN_WG)
        t, r64, r32, A, n = dw_case("normal", B, C, H, W, K, 2, RELU)
        assert r64["z"].abs().min() >= 1e-3 and r32["z"].abs().min() >= 1e-3
        run_dgrad(lib, device, "%s/%s" % (name, mname), t, r64, r32, A, n, B, C, H, W, K, 2, mode, RELU, "normal", None)


@pytest.mark.parametrize("mname,mode,act,families", DGRAD_MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,B,C,H,W,K,opts,form,rows,bn,wg", S1_CASES, ids=S1_IDS)
def test_stride1_data_gradient(lib, device, name, B, C, H, W, K, opts, form, rows, bn, wg, mname, mode, act, families):
    assert H != W
    with options(lib, dw_window=opts[0], dw_lds=opts[1], dw_pipe=opts[2]):
        p = bwd_plan(lib, B, C, H, W, K, 1, mode)
        assert p.family == form, "planned form %d, the case is named after %d" % (p.family, form)
        assert S.chunk_rows(H, p.rpc) == rows and p.chunks == len(rows) and p.blocks == B * len(rows)
        carried = (int(mode != DGRAD and bn), int(mode == DGRAD_BN_WG and wg))
        assert (p.epilogue, p.wgrad) == carried
        assert (p.bn_rows, p.wgrad_rows) == (carried[0] * B * len(rows), carried[1] * B * len(rows))
        refused = None
        if mode != DGRAD and not bn:
            refused = "no kernel form with the epilogue"
        elif mode == DGRAD_BN_WG and not wg:
            refused = "no kernel form carries the filter gradient"
        for family in families:
            t, r64, r32, A, n = dw_case(family, B, C, H, W, K, 1, act)
            run_dgrad(lib, device, "%s/%s/%s" % (name, mname, family), t, r64, r32, A, n, B, C, H, W, K, 1, mode, act, family, refused)


# ---- c. the depthwise filter gradient ---------------------------------------------------------------------------------------------
# global-load form: B, C, H, W, K, stride; Wo % NB != 0 (NB = 2 for 5x5 stride 2, else 4)
WG_GLOBAL_CASES = [(2, 24, 14, 13, 3, 1), (2, 1152, 9, 7, 5, 1), (3, 144, 15, 13, 3, 2), (2, 96, 16, 13, 5, 2)]

# LDS form with the input transform: name, B, C, H, W, K, stride, (cs4, rpc, chunks, tpb, groups) or None = refused
WG_XF_CASES = [
    ("xf_c1152_13x9", 2, 1152, 13, 9, 3, 1, (16, 13, 1, 1, 2)),     # G = 3, RL = 5, one idle lane
    ("xf_c480_17x13", 3, 480, 17, 13, 5, 1, (8, 16, 2, 1, 6)),      # the last chunk is one row
    ("xf_c240_17x13", 3, 240, 17, 13, 5, 1, (4, 16, 2, 1, 6)),
    ("xf_c672_s2", 3, 672, 14, 11, 5, 2, (8, 7, 1, 1, 3)),          # pads (1, 2)
    ("xf_c96_s2", 3, 96, 30, 27, 3, 2, (4, 11, 2, 1, 6)),           # chunks 11 + 4; patch 60720 B, near the 60 KiB limit
    ("xf_16x70_s2", 2, 64, 16, 70, 3, 2, (16, 1, 8, 1, 16)),        # rpc 1, G = 9, 7 idle lanes
    ("xf_13x66", 2, 64, 13, 66, 3, 1, (8, 4, 4, 1, 8)),             # G = 17, RL = 1, 15 idle lanes
    ("xf_tpb2", 31, 1200, 7, 6, 5, 1, (4, 7, 1, 2, 16)),            # two tiles per block, the last group has one
    ("xf_c40_refused", 2, 40, 9, 9, 3, 1, None),                    # C / 4 = 10: no slice of 16, 8 or 4 quads
]
XF_IDS = [c[0] for c in WG_XF_CASES]


@pytest.mark.parametrize("family", ["normal", "one_sign"])
@pytest.mark.parametrize("B,C,H,W,K,stride", WG_GLOBAL_CASES, ids=lambda v: str(v))
def test_filter_gradient_global_load(lib, device, B, C, H, W, K, stride, family):
    Ho, Wo, pt, pl, _, _ = layer(H, W, K, stride)
    assert Wo % (2 if (K, stride) == (5, 2) else 4) != 0 and H != W
    p = bwd_plan(lib, B, C, H, W, K, stride, WGRAD)
    assert p.family == FAM_WG_GLOBAL and p.wgrad == 1 and p.wgrad_rows == p.chunks == -(-(B * Ho) // p.rpc)
    t, r64, r32, A, n = dw_case(family, B, C, H, W, K, stride, NONE)
    d = _lib.dptr
    a, dy, w = (v.to(device).contiguous() for v in (nhwc(r32["a"]), nhwc(t["dy"]), t["w"]))
    dw = Guarded((C, 1, K, K), device)
    _lib.check(lib.orbit_op_dwconv2d_backward(d(a), d(w), d(dy), None, d(dw.t), B, H, W, C, K, stride, pt, pl, Ho, Wo, _st()),
               "orbit_op_dwconv2d_backward")
    torch.cuda.synchronize()
    check_wgrad("wgrad_global", "%dx%dx%dx%d k%d s%d/%s" % (B, C, H, W, K, stride, family), dw.cpu("dw"), r64["dw"], r32["dw"], A, n)


def run_wgrad_xf(lib, device, what, B, C, H, W, K, stride, act, family, geom):
    Ho, Wo, pt, pl, _, _ = layer(H, W, K, stride)
    p = bwd_plan(lib, B, C, H, W, K, stride, WGRAD_XF)
    assert p.family == FAM_WG_LDS and p.wgrad == int(geom is not None)
    t, r64, r32, A, n = dw_case(family, B, C, H, W, K, stride, act)
    d = _lib.dptr
    y, dy, sc, sh = (v.to(device).contiguous() for v in (nhwc(t["y"]), nhwc(t["dy"]), t["scale"], t["shift"]))
    dw = Guarded((C, 1, K, K), device)
    rc = lib.orbit_op_dwconv2d_wgrad_xf(d(y), d(sc), d(sh), act, d(dy), d(dw.t), B, H, W, C, K, stride, pt, pl, Ho, Wo, _st())
    torch.cuda.synchronize()
    if geom is None:
        assert rc == ERR_ARG and "op_dwconv2d_wgrad_xf" in _lib.last_error() and "does not fit" in _lib.last_error()
        assert_untouched(dw, what)
        return
    _lib.check(rc, "orbit_op_dwconv2d_wgrad_xf")
    assert (p.cs4, p.rpc, p.chunks, p.tpb, p.groups) == geom and p.wgrad_rows == p.groups
    check_wgrad("wgrad_xf", what, dw.cpu("dw"), r64["dw"], r32["dw"], A, n)


@pytest.mark.parametrize("family", ["normal", "one_sign"])
@pytest.mark.parametrize("name,B,C,H,W,K,stride,geom", WG_XF_CASES, ids=XF_IDS)
def test_filter_gradient_lds_with_input_transform(lib, device, name, B, C, H, W, K, stride, geom, family):
    assert H != W or geom is None
    run_wgrad_xf(lib, device, "%s/%s" % (name, family), B, C, H, W, K, stride, SILU, family, geom)


def test_filter_gradient_lds_with_input_transform_relu(lib, device):
    name, B, C, H, W, K, stride, geom = WG_XF_CASES[0]
    t, r64, r32, _, _ = dw_case("normal", B, C, H, W, K, stride, RELU)
    assert r64["z"].abs().min() >= 1e-3 and r32["z"].abs().min() >= 1e-3
    run_wgrad_xf(lib, device, name + "/relu", B, C, H, W, K, stride, RELU, "normal", geom)


# ---- d. squeeze-excite backward with the BatchNorm backward riding on it -------------------------------------------------------------
# name, B, HW, C, R
SE_CASES = [("se_c96", 5, 49, 96, 4), ("se_c1152", 3, 16, 1152, 48), ("se_c144_ragged", 2, 197, 144, 6), ("se_c32", 7, 9, 32, 8)]
# each frame has 19600 quads > 64 * 256: gate_bn_bwd_apply_kernel strides, and 16384 % 100 != 0: its q walk wraps
SE_CAPPED = ("se_capped", 256, 196, 400, 20)
BN_EPS = 1e-5


def se_inputs(family, B, HW, C, R, act, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if family == "one_sign":
        z = torch.rand(B, HW, C, generator=g) * 1.9 + 0.55
        scale, shift = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 0.5
        y = (z - nlc(shift)) / nlc(scale)
        mean = y.reshape(-1, C).min(0).values - (torch.rand(C, generator=g) + 0.5)
        invstd = torch.rand(C, generator=g) + 0.5
        gamma, beta = scale / invstd, shift + mean * scale
        dxg, ws = torch.rand(B, HW, C, generator=g) * 0.5 + 0.75, 0.1  # a small gate MLP: the pooled branch cannot turn g negative
    else:
        y = r(B, HW, C) * 1.5 + 0.3 * nlc(r(C))
        gamma, beta = torch.rand(C, generator=g) + 0.5, r(C) * 0.3 + 0.2
        mean, invstd = None, None  # the batch statistics of y (se_ref forms them in its own precision)
        dxg, ws = r(B, HW, C), 1.0
    return {"y": y, "gamma": gamma, "beta": beta, "mean": mean, "invstd": invstd, "dxg": dxg, "w1": ws * r(R, C) * C ** -0.5,
            "b1": 0.1 * r(R), "w2": ws * r(C, R) * R ** -0.5, "b2": 0.1 * r(C)}


def se_ref(t, act, train, dtype):
    """Autograd through y -> BatchNorm -> act -> x * gate(mean_hw x). With t["mean"] = None the statistics are the batch's (train) and
    dy = d/dy through them; with given statistics g, the sums and the parameter gradients come from autograd and dy from the
    BatchNorm backward's own formula k1 (g - [sum g / M + xhat sum(g xhat) / M]), the bracket only in train mode."""
    y = t["y"].to(dtype).requires_grad_(True)
    p = {k: t[k].to(dtype).clone().requires_grad_(True) for k in ("gamma", "beta", "w1", "b1", "w2", "b2")}
    batch = t["mean"] is None
    if batch:
        mean, invstd = y.mean((0, 1)), (y.var((0, 1), unbiased=False) + BN_EPS).rsqrt()
    else:
        mean, invstd = t["mean"].to(dtype), t["invstd"].to(dtype)
    xhat = (y - nlc(mean)) * nlc(invstd)
    z = nlc(p["gamma"]) * xhat + nlc(p["beta"])
    z.retain_grad()
    x = act_fn(z, act)
    pooled = x.mean(1)
    gate = torch.sigmoid(F.silu(pooled @ p["w1"].t() + p["b1"]) @ p["w2"].t() + p["b2"])
    (x * gate[:, None, :]).backward(t["dxg"].to(dtype))
    out = {"x": x.detach(), "pooled": pooled.detach(), "g": z.grad, "mean": mean.detach(), "invstd": invstd.detach(),
           "dgamma": p["gamma"].grad, "dbeta": p["beta"].grad, "dw1": p["w1"].grad, "db1": p["b1"].grad, "dw2": p["w2"].grad,
           "db2": p["b2"].grad}
    if batch and train:
        out["dy"] = y.grad
    else:
        M, xh, g = y.shape[0] * y.shape[1], xhat.detach(), z.grad
        k1 = nlc(p["gamma"].detach() * invstd.detach())
        out["dy"] = k1 * (g - nlc(g.sum((0, 1))) / M - xh * nlc((g * xh).sum((0, 1))) / M) if train else k1 * g
    return out


@functools.lru_cache(maxsize=1)
def se_case(family, B, HW, C, R, act, train):
    t = se_inputs(family, B, HW, C, R, act, seed=B + HW + C + R)
    return t, se_ref(t, act, train, torch.float64), se_ref(t, act, train, torch.float32)


def run_se_bn(lib, device, what, t, r64, B, HW, C, R, act, train, sums_only, with_params):
    """orbit_op_se_gate_backward_bn on the float32 casts of the float64 tape; returns the outputs on the CPU after the guard checks."""
    f = lambda v: v.detach().float().to(device).contiguous()  # noqa: E731
    scale = r64["invstd"] * t["gamma"].double()
    shift = t["beta"].double() - r64["mean"] * scale
    ins = [f(t["dxg"]), f(r64["x"]), f(t["y"]), f(r64["mean"]), f(r64["invstd"]), f(scale), f(shift)]
    se = [f(r64["pooled"]), f(t["w1"]), f(t["b1"]), f(t["w2"]), f(t["b2"]), f(t["gamma"])]
    out = {"g": None if sums_only else Guarded((B, HW, C), device), "sums": Guarded((2, C), device), "dy": Guarded((B, HW, C), device),
           "dgamma": Guarded((C,), device), "dbeta": Guarded((C,), device)}
    names = ["g", "sums", "dy", "dgamma", "dbeta"]
    if with_params:
        out.update(dw1=Guarded((R, C), device), db1=Guarded((R,), device), dw2=Guarded((C, R), device), db2=Guarded((C,), device))
    names += ["dw1", "db1", "dw2", "db2"]
    d = _lib.dptr
    ptr = lambda k: d(out[k].t) if out.get(k) is not None else None  # noqa: E731
    _lib.check(lib.orbit_op_se_gate_backward_bn(*[d(v) for v in ins], act, *[d(v) for v in se], train, int(sums_only),
                                                *[ptr(k) for k in names], B, HW, C, R, _st()), "orbit_op_se_gate_backward_bn")
    torch.cuda.synchronize()
    return {k: v.cpu("%s: %s" % (what, k)) for k, v in out.items() if v is not None}, ins


def check_se_bn(what, got, g_written, t, r64, r32, ins, with_params):
    if "g" in got:
        elementwise_gate("se_bn_g", what, got["g"], r64["g"], r32["g"])
    check_channel_sums("se_bn_sums", what, got["sums"], g_written, ins[2].cpu(), ins[3].cpu(), ins[4].cpu(), 2)
    elementwise_gate("se_bn_dy", what, got["dy"], r64["dy"], r32["dy"])
    for k in ("dgamma", "dbeta") + (("dw1", "db1", "dw2", "db2") if with_params else ()):
        param_gate("se_bn_" + k, what, got[k], r64[k], r32[k])


@pytest.mark.parametrize("family", ["normal", "one_sign"])
@pytest.mark.parametrize("name,B,HW,C,R", SE_CASES, ids=[c[0] for c in SE_CASES])
def test_se_backward_with_batchnorm(lib, device, name, B, HW, C, R, family):
    t, r64, r32 = se_case(family, B, HW, C, R, SILU, 1)
    full, ins = run_se_bn(lib, device, name + "/g", t, r64, B, HW, C, R, SILU, 1, False, True)
    check_se_bn("%s/%s/g written" % (name, family), full, full["g"], t, r64, r32, ins, True)
    sums, ins = run_se_bn(lib, device, name + "/sums", t, r64, B, HW, C, R, SILU, 1, True, False)
    check_se_bn("%s/%s/sums only" % (name, family), sums, full["g"], t, r64, r32, ins, False)


def test_se_backward_with_batchnorm_eval(lib, device):
    name, B, HW, C, R = SE_CASES[0]
    t = se_inputs("normal", B, HW, C, R, SILU, seed=3)
    g = torch.Generator().manual_seed(5)
    t["mean"], t["invstd"] = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5  # running statistics
    r64, r32 = se_ref(t, SILU, 0, torch.float64), se_ref(t, SILU, 0, torch.float32)
    for sums_only in (False, True):
        got, ins = run_se_bn(lib, device, name + "/eval", t, r64, B, HW, C, R, SILU, 0, sums_only, not sums_only)
        if not sums_only:
            g_written = got["g"]
        check_se_bn("%s/eval/%s" % (name, "sums only" if sums_only else "g written"), got, g_written, t, r64, r32, ins, not sums_only)


def test_se_backward_with_batchnorm_capped_grid(lib, device):
    name, B, HW, C, R = SE_CAPPED
    t, r64, r32 = se_case("normal", B, HW, C, R, SILU, 1)
    full, _ = run_se_bn(lib, device, name + "/g", t, r64, B, HW, C, R, SILU, 1, False, False)  # (the g the sums are checked against)
    got, ins = run_se_bn(lib, device, name + "/sums", t, r64, B, HW, C, R, SILU, 1, True, False)
    check_se_bn(name + "/sums only", got, full["g"], t, r64, r32, ins, False)
