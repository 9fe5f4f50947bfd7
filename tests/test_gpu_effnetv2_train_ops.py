"""The operators behind the opt-in FiLM backward through the frozen efficientnet_v2_s (csrc/train_ops.hip, csrc/extractor_train.hip),
one by one against float64 on the CPU:

  * the post-skip forms the feature adds, for timm ConvBnAct's out = silu(bn(y)) + residual: the BatchNorm backward
    (orbit_op_bn_backward_ex with ORBIT_BN_RESIDUAL_POST_ACT: dres = dout, NOT dout * silu') and the activation pass of the taped
    forward (orbit_op_scale_shift_act with the same flag);
  * the existing backward entry points at the shapes only this network has: dense 3x3 stride-2 data gradients under TF "SAME"
    padding (0 on even maps, 1 on odd ones) at 24 / 48 channels, depthwise 3x3 at 1536 channels and stride 2 under SAME padding,
    squeeze-excite up to C = 1536, R = 64.

Gate (the convention of tests/test_gpu_effnetv2_ops.py, relative to the largest reference value): max |got - ref64| <=
max(2e-5, 4 x E32) x max |ref64|, E32 = max |ref32 - ref64| / max |ref64| of the same expression evaluated in float32 on the CPU
on the same inputs; both are printed."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402

POST = 1  # ORBIT_BN_RESIDUAL_POST_ACT
SILU = 2
BN_SHAPES = [(3 * 17 * 13, 24), (126, 64), (1, 64)]  # C = 24: 6 channel quads, the non-power-of-two column layout


def _st():
    return _lib.stream_handle()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def gate(got, ref64, ref32, what, scale=None):
    """got (fp32, from the GPU) against the float64 reference; ref32 the same expression evaluated in float32 on the CPU.
    scale: max |ref64| unless the caller knows the reference to be a difference of larger terms that cancels to zero."""
    scale = ref64.abs().max().item() if scale is None else scale
    assert scale > 0, what
    e32 = (ref32.double() - ref64).abs().max().item() / scale
    err = (got.double() - ref64).abs().max().item()
    tol = max(2e-5, 4 * e32) * scale
    print("\n[effnetv2-train-ops] %s: err %.3g, E32 %.3g (relative), tol %.3g, max |ref| %.3g" % (what, err, e32, tol, scale))
    assert torch.isfinite(got).all(), what
    assert err <= tol, (what, err, tol)


# ---- the post-skip BatchNorm backward ----------------------------------------------------------------------------------------
def _bn_inputs(M, C):
    g = torch.Generator().manual_seed(1000 * C + M)
    y = torch.randn(M, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    res = torch.randn(M, C, generator=g, dtype=torch.float64)
    gamma = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    dout = torch.randn(M, C, generator=g, dtype=torch.float64)
    prior = torch.randn(M, C, generator=g, dtype=torch.float64)  # what dres already holds in the accumulating form
    run_mean = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    run_var = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    return y, res, gamma, beta, dout, prior, run_mean, run_var


def _bn_stats(y, run_mean, run_var, train, eps=1e-3):
    """(mean, invstd) the forward normalised with: batch statistics (biased variance) or the running ones."""
    if train:
        return y.mean(0), (y.var(0, unbiased=False) + eps).rsqrt()
    return run_mean.clone(), (run_var + eps).rsqrt()


def _bn_reference(M, C, train, dtype):
    """autograd through out = silu(bn(y)) + res in `dtype`: dy, dres, dgamma, dbeta of sum(out * dout)."""
    y, res, gamma, beta, dout, _, run_mean, run_var = (t.to(dtype) for t in _bn_inputs(M, C))
    y, res, gamma, beta = (t.clone().requires_grad_(True) for t in (y, res, gamma, beta))
    if train:
        mean, invstd = y.mean(0), (y.var(0, unbiased=False) + 1e-3).rsqrt()  # on the graph: dy goes through the statistics
    else:
        mean, invstd = _bn_stats(y.detach(), run_mean, run_var, 0)
    out = F.silu((y - mean) * invstd * gamma + beta) + res
    (out * dout).sum().backward()
    return y.grad, res.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("accumulate", [0, 1], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("train", [0, 1], ids=["running", "batch"])
@pytest.mark.parametrize("M,C", BN_SHAPES, ids=lambda v: str(v))
def test_post_skip_bn_backward(lib, device, M, C, train, accumulate):
    y, res, gamma, beta, dout, prior, run_mean, run_var = _bn_inputs(M, C)
    mean, invstd = _bn_stats(y.float().double(), run_mean, run_var, train)  # statistics of the fp32 tensor the kernel reads
    scale = gamma * invstd
    shift = beta - mean * scale
    f = lambda t: t.float().to(device).contiguous()
    t_dout, t_y, t_gamma, t_mean, t_invstd, t_scale, t_shift = (f(t) for t in (dout, y, gamma, mean, invstd, scale, shift))
    dy = torch.full((M, C), float("nan"), device=device)
    dres = f(prior) if accumulate else torch.full((M, C), float("nan"), device=device)
    dgamma, dbeta = torch.full((C,), float("nan"), device=device), torch.full((C,), float("nan"), device=device)
    _lib.check(lib.orbit_op_bn_backward_ex(_lib.dptr(t_dout), None, _lib.dptr(t_y), M, C, _lib.dptr(t_gamma), _lib.dptr(t_mean),
                                           _lib.dptr(t_invstd), _lib.dptr(t_scale), _lib.dptr(t_shift), train, SILU, POST,
                                           _lib.dptr(dy), _lib.dptr(dres), accumulate, _lib.dptr(dgamma), _lib.dptr(dbeta), _st()),
               "orbit_op_bn_backward_ex")
    torch.cuda.synchronize()
    r64, r32 = _bn_reference(M, C, train, torch.float64), _bn_reference(M, C, train, torch.float32)
    what = "post-skip bn backward M=%d C=%d train=%d acc=%d" % (M, C, train, accumulate)
    # the residual branch receives dout itself (+ what the slot held): equal to fp32 rounding, one addition at the most
    want_res = dout.float().double() + (prior.float().double() if accumulate else 0)
    res_err = (dres.cpu().double() - want_res).abs().max().item()
    print("\n[effnetv2-train-ops] %s: |dres - (dout + prior)| %.3g" % (what, res_err))
    assert res_err <= 2.0 ** -23 * want_res.abs().max().item()
    # ... which g = dout * silu'(.) is not: the pre-activation form of the kernel cannot pass
    z = (y - mean) * invstd * gamma + beta
    sg = torch.sigmoid(z)
    g = dout * sg * (1 + z * (1 - sg))
    assert (g - dout).abs().max().item() > 0.1
    assert (dres.cpu().double() - (g + (prior if accumulate else 0))).abs().max().item() > 0.1
    assert torch.equal(r64[1], dout)  # (and autograd agrees that d out / d res = 1)
    # batch statistics of a single row: xhat = 0 and dy = k1 * (g - mean(g)) = 0 - measured against the terms that cancel
    # (and dgamma = sum g * xhat = 0: against g)
    single = bool(train and M == 1)
    gate(dy.cpu(), r64[0], r32[0], what + " dy", (gamma * invstd * g).abs().max().item() if single else None)
    gate(dgamma.cpu(), r64[2], r32[2], what + " dgamma", g.abs().max().item() if single else None)
    gate(dbeta.cpu(), r64[3], r32[3], what + " dbeta")


def test_bn_backward_ex_without_the_flag_is_the_pre_activation_form(lib, device):
    """flags = 0 with SiLU (which the older entry refuses), a forward without a residual, out = silu(bn(y)): the gradient the
    kernel hands to `dres` is g = dout * silu'(.) - what the post-skip form must NOT write there."""
    M, C = 126, 64
    y, res, gamma, beta, dout, _, run_mean, run_var = _bn_inputs(M, C)
    mean, invstd = _bn_stats(y, run_mean, run_var, 0)
    scale = gamma * invstd
    shift = beta - mean * scale
    f = lambda t: t.float().to(device).contiguous()
    ts = [f(t) for t in (dout, y, gamma, mean, invstd, scale, shift)]
    dy, dres = torch.full((M, C), float("nan"), device=device), torch.full((M, C), float("nan"), device=device)
    dgamma, dbeta = torch.empty(C, device=device), torch.empty(C, device=device)
    _lib.check(lib.orbit_op_bn_backward_ex(_lib.dptr(ts[0]), None, _lib.dptr(ts[1]), M, C, _lib.dptr(ts[2]), _lib.dptr(ts[3]),
                                           _lib.dptr(ts[4]), _lib.dptr(ts[5]), _lib.dptr(ts[6]), 0, SILU, 0, _lib.dptr(dy),
                                           _lib.dptr(dres), 0, _lib.dptr(dgamma), _lib.dptr(dbeta), _st()), "orbit_op_bn_backward_ex")
    torch.cuda.synchronize()
    refs = {}
    for dtype in (torch.float64, torch.float32):
        yy, gg, bb, dd = (t.to(dtype) for t in (y, gamma, beta, dout))
        z = (yy - mean.to(dtype)) * invstd.to(dtype) * gg + bb
        sg = torch.sigmoid(z)
        refs[dtype] = dd * sg * (1 + z * (1 - sg))
    gate(dres.cpu(), refs[torch.float64], refs[torch.float32], "pre-activation form dres = g")
    assert lib.orbit_op_bn_backward_ex(_lib.dptr(ts[0]), None, _lib.dptr(ts[1]), M, C, _lib.dptr(ts[2]), _lib.dptr(ts[3]),
                                       _lib.dptr(ts[4]), None, None, 0, SILU, POST, _lib.dptr(dy), _lib.dptr(dres), 0,
                                       _lib.dptr(dgamma), _lib.dptr(dbeta), _st()) == -1  # SiLU without scale / shift
    assert lib.orbit_op_bn_backward_ex(_lib.dptr(ts[0]), None, _lib.dptr(ts[1]), M, C, _lib.dptr(ts[2]), _lib.dptr(ts[3]),
                                       _lib.dptr(ts[4]), _lib.dptr(ts[5]), _lib.dptr(ts[6]), 0, SILU, 2, _lib.dptr(dy),
                                       _lib.dptr(dres), 0, _lib.dptr(dgamma), _lib.dptr(dbeta), _st()) == -1  # unknown flag
    torch.cuda.synchronize()


# ---- the post-skip activation pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", BN_SHAPES, ids=lambda v: str(v))
def test_post_skip_activation_pass(lib, device, M, C):
    y, res, gamma, beta, _, _, run_mean, run_var = _bn_inputs(M, C)
    mean, invstd = _bn_stats(y, run_mean, run_var, 0)
    scale = gamma * invstd
    shift = beta - mean * scale
    f = lambda t: t.float().to(device).contiguous()
    t_y, t_scale, t_shift, t_res = f(y), f(scale), f(shift), f(res)
    out = torch.full((M + 1, C), float("nan"), device=device)
    out[M:] = 7777.0
    _lib.check(lib.orbit_op_scale_shift_act(_lib.dptr(t_y), _lib.dptr(t_scale), _lib.dptr(t_shift), _lib.dptr(t_res), SILU, M, C,
                                            POST, _lib.dptr(out), _st()), "orbit_op_scale_shift_act")
    pre = torch.full((M, C), float("nan"), device=device)
    _lib.check(lib.orbit_op_scale_shift_act(_lib.dptr(t_y), _lib.dptr(t_scale), _lib.dptr(t_shift), _lib.dptr(t_res), SILU, M, C,
                                            0, _lib.dptr(pre), _st()), "orbit_op_scale_shift_act")
    torch.cuda.synchronize()
    assert bool((out[M:] == 7777.0).all())
    ref = lambda dt: F.silu(scale.to(dt) * y.to(dt) + shift.to(dt)) + res.to(dt)
    ref_pre = lambda dt: F.silu(scale.to(dt) * y.to(dt) + shift.to(dt) + res.to(dt))
    gate(out[:M].cpu(), ref(torch.float64), ref(torch.float32), "post-skip activation pass M=%d C=%d" % (M, C))
    gate(pre.cpu(), ref_pre(torch.float64), ref_pre(torch.float32), "pre-activation form M=%d C=%d" % (M, C))
    assert (ref(torch.float64) - ref_pre(torch.float64)).abs().max().item() > 1e-2  # the two forms differ on these inputs
    # the flag without a residual is refused
    assert lib.orbit_op_scale_shift_act(_lib.dptr(t_y), _lib.dptr(t_scale), _lib.dptr(t_shift), None, SILU, M, C, POST,
                                        _lib.dptr(pre), _st()) == -1
    torch.cuda.synchronize()


# ---- existing entry points at this network's shapes --------------------------------------------------------------------------
def same_pad(size, k, stride):
    """TF "SAME": (output size, padding before, padding after); the odd unit of padding goes after."""
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2, total - total // 2


# (B, Cin, H, W, Cout, K, stride)
DGRAD_CASES = [
    (2, 24, 16, 16, 96, 3, 2),   # even map: padding 0 before, 1 after
    (2, 24, 35, 27, 96, 3, 2),   # odd map: 1 / 1 (what a 70 x 54 frame leaves after the stem)
    (2, 48, 9, 7, 192, 3, 2),
    (2, 24, 9, 7, 24, 3, 1),     # ConvBnAct
    (2, 256, 2, 3, 1536, 1, 1),  # the widest expansion
]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_dgrad_at_this_networks_shapes(lib, device, case):
    B, Cin, H, W, Cout, K, stride = case
    Ho, pt, pb = same_pad(H, K, stride)
    Wo, pl, pr = same_pad(W, K, stride)
    if case[:4] == (2, 24, 16, 16):
        assert (Ho, Wo, pt, pl) == (8, 8, 0, 0)
    if case[:4] == (2, 24, 35, 27):
        assert (Ho, Wo, pt, pl) == (18, 14, 1, 1)
    g = torch.Generator().manual_seed(sum(case))
    x0 = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w0 = torch.randn(Cout, Cin, K, K, generator=g, dtype=torch.float64) / (Cin * K * K) ** 0.5
    dy0 = torch.randn(B, Cout, Ho, Wo, generator=g, dtype=torch.float64)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        x = x0.to(dtype).clone().requires_grad_(True)
        y = F.conv2d(F.pad(x, [pl, pr, pt, pb]), w0.to(dtype), None, stride)
        assert y.shape[2:] == (Ho, Wo)
        y.backward(dy0.to(dtype))
        refs[dtype] = x.grad
    t_dy, t_w = nhwc(dy0.float()).to(device), w0.float().to(device).contiguous()
    dx = torch.full((B, H, W, Cin), float("nan"), device=device)
    _lib.check(lib.orbit_op_conv2d_dgrad(_lib.dptr(t_dy), _lib.dptr(t_w), None, _lib.dptr(dx), B, H, W, Cin, Cout, K, K, stride,
                                         pt, pl, Ho, Wo, _st()), "orbit_op_conv2d_dgrad")
    torch.cuda.synchronize()
    gate(dx.cpu().permute(0, 3, 1, 2), refs[torch.float64], refs[torch.float32], "conv dgrad " + "x".join(map(str, case)))


# (B, C, H, W, stride)
DW_CASES = [(3, 1536, 2, 2, 1), (3, 1536, 4, 3, 1), (3, 256, 8, 8, 2), (3, 256, 9, 7, 2)]


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv_backward_at_this_networks_shapes(lib, device, case):
    B, C, H, W, stride = case
    Ho, pt, pb = same_pad(H, 3, stride)
    Wo, pl, pr = same_pad(W, 3, stride)
    g = torch.Generator().manual_seed(sum(case))
    x0 = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w0 = torch.randn(C, 1, 3, 3, generator=g, dtype=torch.float64) / 3
    dy0 = torch.randn(B, C, Ho, Wo, generator=g, dtype=torch.float64)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        x, w = x0.to(dtype).clone().requires_grad_(True), w0.to(dtype).clone().requires_grad_(True)
        F.conv2d(F.pad(x, [pl, pr, pt, pb]), w, None, stride, 0, 1, C).backward(dy0.to(dtype))
        refs[dtype] = (x.grad, w.grad)
    t_x, t_w, t_dy = nhwc(x0.float()).to(device), w0.float().to(device).contiguous(), nhwc(dy0.float()).to(device)
    dx = torch.full((B, H, W, C), float("nan"), device=device)
    dw = torch.full((C, 1, 3, 3), float("nan"), device=device)
    _lib.check(lib.orbit_op_dwconv2d_backward(_lib.dptr(t_x), _lib.dptr(t_w), _lib.dptr(t_dy), _lib.dptr(dx), _lib.dptr(dw), B, H, W,
                                              C, 3, stride, pt, pl, Ho, Wo, _st()), "orbit_op_dwconv2d_backward")
    torch.cuda.synchronize()
    what = "dwconv backward " + "x".join(map(str, case))
    gate(dx.cpu().permute(0, 3, 1, 2), refs[torch.float64][0], refs[torch.float32][0], what + " dx")
    gate(dw.cpu(), refs[torch.float64][1], refs[torch.float32][1], what + " dw")


@pytest.mark.parametrize("HW", [4, 6])
@pytest.mark.parametrize("C,R", [(1536, 64), (960, 40), (256, 16)])
def test_se_gate_backward_at_this_networks_shapes(lib, device, C, R, HW):
    B = 3
    g = torch.Generator().manual_seed(C + R + HW)
    x0 = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    w1 = torch.randn(R, C, generator=g, dtype=torch.float64) / C ** 0.5
    b1 = 0.1 * torch.randn(R, generator=g, dtype=torch.float64)
    w2 = torch.randn(C, R, generator=g, dtype=torch.float64) / R ** 0.5
    b2 = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    dxg = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        x = x0.to(dtype).clone().requires_grad_(True)
        gt = torch.sigmoid(F.silu(x.mean(dim=1) @ w1.to(dtype).t() + b1.to(dtype)) @ w2.to(dtype).t() + b2.to(dtype))
        (x * gt[:, None, :]).backward(dxg.to(dtype))
        refs[dtype] = x.grad
    f = lambda t: t.float().to(device).contiguous()
    ts = [f(dxg), f(x0), f(x0.float().mean(dim=1)), f(w1), f(b1), f(w2), f(b2)]
    dx = torch.full((B, HW, C), float("nan"), device=device)
    _lib.check(lib.orbit_op_se_gate_backward(*[_lib.dptr(t) for t in ts], _lib.dptr(dx), None, None, None, None, B, HW, C, R,
                                             _st()), "orbit_op_se_gate_backward")
    torch.cuda.synchronize()
    gate(dx.cpu(), refs[torch.float64], refs[torch.float32], "se gate backward C=%d R=%d HW=%d" % (C, R, HW))
