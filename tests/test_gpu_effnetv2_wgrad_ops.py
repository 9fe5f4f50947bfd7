"""The operators behind native training of efficientnet_v2_s (ORBIT_PLAN_RES_POST_TRAINING), one by one against float64 torch
autograd on the CPU, at the smallest shapes of this network that can go wrong:

  * the dense filter gradient (csrc/conv_wgrad.hip) under TF "SAME" padding at 3x3 stride 2 / stride 1, the widest pointwise
    pair (256 <-> 1536) and the NCHW stem 3 -> 24; the gated filter gradient at 1536 -> 256 and 512 -> 128;
  * the squeeze-excite backward with its four parameter gradients from the per-block kernel (flags = 0) and from the batched
    kernel (ORBIT_SE_PARAMS_BATCHED; R = 64 takes its 16-per-thread strip form, R <= 48 the 12-strip form), at B = 3 and at
    B = 53 (more than one LDS stage of 50 frames);
  * the batch-statistics forms of the dense and the depthwise convolution at C = 24 (663 rows) and at C = 1536 on a 2 x 2 map
    (16 rows per channel): output, and the mean / inverse standard deviation their column sums give.

Gate (tests/test_gpu_vit_ops.gate): max |got - ref64| <= max(4 * e32, 8 * 2**-24 * max |ref64|), e32 = the float32 CPU run's own
error against float64 on the same inputs, measured here; every test prints its largest err / e32 (run with -s).

The 12-strip instantiation of the batched squeeze-excite kernel holds, instruction for instruction, the kernel as it was before it
became a template (compare the device assembly of two checkouts with tools/device_asm_diff.py): what R <= 48 gives through
ORBIT_SE_PARAMS_BATCHED is what efficientnet_b0's reverse pass has always computed. No entry point reaches the two instantiations
with one job, so the suite checks the batched form for determinism and through the float64 gate.

Largest err / e32 seen on the MI355X: dense filter gradient 1.40, gated 1.61, squeeze-excite per-block 1.16 / batched 2.16 (C = 960,
R = 40, HW = 6, B = 53), batch-statistics dense conv 1.77, depthwise 1.29."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from test_gpu_effnetv2_train_ops import nhwc, same_pad  # noqa: E402
from test_gpu_vit_ops import gate  # noqa: E402

BATCHED = 1  # ORBIT_SE_PARAMS_BATCHED
EPS = 1e-3   # the BatchNorm eps of tf_efficientnetv2_s


def _st():
    return _lib.stream_handle()


def _e32(ref32, ref64):
    return (ref32.double() - ref64).abs().max().item()


# ---- dense filter gradient -------------------------------------------------------------------------------------------------
# (B, Cin, H, W, Cout, K, stride)
WGRAD_CASES = [
    (3, 24, 35, 27, 96, 3, 2),    # odd map, padding 1 / 1, 756 rows: more than one split, ragged last K-step
    (2, 24, 16, 16, 96, 3, 2),    # even map, padding 0 before, single split
    (2, 48, 9, 7, 192, 3, 1),
    (2, 24, 9, 7, 24, 3, 1),      # ConvBnAct, Cout < 64
    (2, 64, 5, 4, 256, 3, 2),
    (2, 256, 2, 3, 1536, 1, 1),   # the widest expansion and its projection
    (2, 1536, 2, 3, 256, 1, 1),
]
STEM_CASES = [(2, 3, 64, 64, 24, 3, 2), (2, 3, 71, 55, 24, 3, 2)]


def _wgrad_reference(case, x0, dy0, pads):
    B, Cin, H, W, Cout, K, stride = case
    pt, pb, pl, pr = pads
    out = {}
    for dtype in (torch.float64, torch.float32):
        w = torch.zeros(Cout, Cin, K, K, dtype=dtype, requires_grad=True)
        F.conv2d(F.pad(x0.to(dtype), [pl, pr, pt, pb]), w, None, stride).backward(dy0.to(dtype))
        out[dtype] = w.grad
    return out


@pytest.mark.parametrize("case", WGRAD_CASES + STEM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_wgrad_at_this_networks_shapes(lib, device, case):
    B, Cin, H, W, Cout, K, stride = case
    nchw_in = int(Cin == 3)
    Ho, pt, pb = same_pad(H, K, stride)
    Wo, pl, pr = same_pad(W, K, stride)
    if case[:4] == (3, 24, 35, 27):
        assert (Ho, Wo, pt, pl) == (18, 14, 1, 1) and B * Ho * Wo == 756
    if case[:4] == (2, 24, 16, 16):
        assert (Ho, Wo, pt, pl) == (8, 8, 0, 0)
    g = torch.Generator().manual_seed(sum(case) + 11)
    x0 = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64).float().double()
    dy0 = torch.randn(B, Cout, Ho, Wo, generator=g, dtype=torch.float64).float().double()
    refs = _wgrad_reference(case, x0, dy0, (pt, pb, pl, pr))
    t_x = x0.float().contiguous().to(device) if nchw_in else nhwc(x0.float()).to(device)
    t_dy = nhwc(dy0.float()).to(device)
    dw = torch.full((Cout, Cin, K, K), float("nan"), device=device)
    _lib.check(lib.orbit_op_conv2d_wgrad(_lib.dptr(t_x), nchw_in, _lib.dptr(t_dy), _lib.dptr(dw), B, H, W, Cin, Cout, K, K, stride,
                                         pt, pl, Ho, Wo, _st()), "orbit_op_conv2d_wgrad")
    torch.cuda.synchronize()
    what = "conv wgrad " + "x".join(map(str, case))
    r = gate(dw.cpu(), refs[torch.float64], _e32(refs[torch.float32], refs[torch.float64]), what)
    print("\n[effnetv2-wgrad-ops] %s: err / e32 %.2f" % (what, r))


@pytest.mark.parametrize("case", [(3, 1536, 2, 3, 256), (3, 512, 4, 4, 128)], ids=lambda c: "x".join(map(str, c)))
def test_conv_wgrad_gated_at_this_networks_shapes(lib, device, case):
    B, Cin, H, W, Cout = case
    g = torch.Generator().manual_seed(sum(case) + 13)
    x0 = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64).float().double()
    gt0 = torch.rand(B, Cin, generator=g, dtype=torch.float64).float().double()
    dy0 = torch.randn(B, Cout, H, W, generator=g, dtype=torch.float64).float().double()
    refs = {}
    for dtype in (torch.float64, torch.float32):
        w = torch.zeros(Cout, Cin, 1, 1, dtype=dtype, requires_grad=True)
        F.conv2d(x0.to(dtype) * gt0.to(dtype)[:, :, None, None], w).backward(dy0.to(dtype))
        refs[dtype] = w.grad
    t_x, t_g, t_dy = nhwc(x0.float()).to(device), gt0.float().to(device), nhwc(dy0.float()).to(device)
    dw = torch.full((Cout, Cin, 1, 1), float("nan"), device=device)
    _lib.check(lib.orbit_op_conv2d_wgrad_gated(_lib.dptr(t_x), _lib.dptr(t_g), _lib.dptr(t_dy), _lib.dptr(dw), B, H, W, Cin, Cout,
                                               _st()), "orbit_op_conv2d_wgrad_gated")
    torch.cuda.synchronize()
    what = "gated conv wgrad " + "x".join(map(str, case))
    r = gate(dw.cpu(), refs[torch.float64], _e32(refs[torch.float32], refs[torch.float64]), what)
    print("\n[effnetv2-wgrad-ops] %s: err / e32 %.2f" % (what, r))


# ---- squeeze-excite backward with its parameter gradients ------------------------------------------------------------------
_SE = {}


def _se_case(C, R, HW, B):
    """inputs and the float64 / float32 autograd gradients (dx, dW1, db1, dW2, db2); computed once per shape."""
    key = (C, R, HW, B)
    if key not in _SE:
        g = torch.Generator().manual_seed(C + R + HW + 100 * B)
        f32 = lambda t: t.float().double()  # the inputs are float32 numbers: both references and the kernel read the same
        x0 = f32(torch.randn(B, HW, C, generator=g, dtype=torch.float64))
        w1 = f32(torch.randn(R, C, generator=g, dtype=torch.float64) / C ** 0.5)
        b1 = f32(0.1 * torch.randn(R, generator=g, dtype=torch.float64))
        w2 = f32(torch.randn(C, R, generator=g, dtype=torch.float64) / R ** 0.5)
        b2 = f32(0.1 * torch.randn(C, generator=g, dtype=torch.float64))
        dxg = f32(torch.randn(B, HW, C, generator=g, dtype=torch.float64))
        refs = {}
        for dtype in (torch.float64, torch.float32):
            x, a1, c1, a2, c2 = (t.to(dtype).clone().requires_grad_(True) for t in (x0, w1, b1, w2, b2))
            gt = torch.sigmoid(F.silu(x.mean(dim=1) @ a1.t() + c1) @ a2.t() + c2)
            (x * gt[:, None, :]).backward(dxg.to(dtype))
            refs[dtype] = [t.grad for t in (x, a1, c1, a2, c2)]
        _SE[key] = (x0, w1, b1, w2, b2, dxg, refs)
    return _SE[key]


def _se_run(lib, device, C, R, HW, B, flags):
    x0, w1, b1, w2, b2, dxg, _ = _se_case(C, R, HW, B)
    f = lambda t: t.float().to(device).contiguous()
    ts = [f(dxg), f(x0), f(x0.float().mean(dim=1)), f(w1), f(b1), f(w2), f(b2)]
    outs = [torch.full(s, float("nan"), device=device) for s in ((B, HW, C), (R, C), (R,), (C, R), (C,))]
    _lib.check(lib.orbit_op_se_gate_backward_ex(*[_lib.dptr(t) for t in ts], *[_lib.dptr(t) for t in outs], B, HW, C, R, flags,
                                                _st()), "orbit_op_se_gate_backward_ex")
    torch.cuda.synchronize()
    return [t.cpu() for t in outs]


@pytest.mark.parametrize("flags", [0, BATCHED], ids=["per-block", "batched"])
@pytest.mark.parametrize("B", [3, 53])
@pytest.mark.parametrize("HW", [4, 6])
@pytest.mark.parametrize("C,R", [(1536, 64), (960, 40), (256, 16)])
def test_se_gate_backward_with_parameter_gradients(lib, device, C, R, HW, B, flags):
    refs = _se_case(C, R, HW, B)[-1]
    got = _se_run(lib, device, C, R, HW, B, flags)
    worst = 0.0
    for name, t, r64, r32 in zip(("dx", "dW1", "db1", "dW2", "db2"), got, refs[torch.float64], refs[torch.float32]):
        worst = max(worst, gate(t, r64, _e32(r32, r64), "se backward C=%d R=%d HW=%d B=%d flags=%d %s" % (C, R, HW, B, flags, name)))
    print("\n[effnetv2-wgrad-ops] se backward C=%d R=%d HW=%d B=%d flags=%d: largest err / e32 %.2f" % (C, R, HW, B, flags, worst))


@pytest.mark.parametrize("C,R", [(1536, 64), (960, 40), (256, 16)])
def test_se_batched_parameter_gradients_are_deterministic_and_leave_dx_alone(lib, device, C, R):
    """Two runs of the batched form are bitwise equal (frames are added in order, no atomics), and dx - which no flag touches -
    equals the per-block call's bit for bit. (The two forms of the parameter gradients add the frames in different orders:
    they meet only through the float64 gate above.)"""
    a = _se_run(lib, device, C, R, 4, 53, BATCHED)
    b = _se_run(lib, device, C, R, 4, 53, BATCHED)
    for t, u in zip(a, b):
        assert torch.equal(t, u)
    assert torch.equal(a[0], _se_run(lib, device, C, R, 4, 53, 0)[0])


def test_se_ex_refusals(lib, device):
    z = torch.zeros(4, device=device)
    p = _lib.dptr(z)
    assert lib.orbit_op_se_gate_backward_ex(p, p, p, p, p, p, p, p, p, p, p, p, 1, 1, 4, 65, BATCHED, _st()) != 0
    assert "64" in _lib.last_error()
    assert lib.orbit_op_se_gate_backward_ex(p, p, p, p, p, p, p, p, p, p, p, p, 1, 1, 4, 4, 2, _st()) != 0
    assert "flags" in _lib.last_error()
    torch.cuda.synchronize()


# ---- batch-statistics forward ----------------------------------------------------------------------------------------------
def _stats_gate(stats, M, y64, y32, what):
    """mean and 1 / sqrt(biased variance + eps) from the kernel's column sums (s / M and ss / M - mean^2 in double, the
    expression of bn_stats_finalize_kernel) against the statistics of the float64 output."""
    s, ss = stats[0].cpu().double(), stats[1].cpu().double()
    mean = s / M
    invstd = (ss / M - mean * mean + EPS).rsqrt()
    ref = {}
    for dtype, y in ((torch.float64, y64), (torch.float32, y32)):
        yc = y.permute(0, 2, 3, 1).reshape(M, -1)
        ref[dtype] = (yc.mean(0), (yc.var(0, unbiased=False) + EPS).rsqrt())
    r1 = gate(mean.float(), ref[torch.float64][0], _e32(ref[torch.float32][0], ref[torch.float64][0]), what + " mean")
    r2 = gate(invstd.float(), ref[torch.float64][1], _e32(ref[torch.float32][1], ref[torch.float64][1]), what + " invstd")
    return max(r1, r2)


# (B, Cin, H, W, Cout, K, stride): C = 24 at 663 rows (3 x 17 x 13), and 16 rows per channel at the widest layers
CONV_TRAIN_CASES = [(3, 24, 17, 13, 24, 3, 1), (3, 24, 34, 26, 48, 3, 2), (4, 256, 2, 2, 1536, 1, 1), (4, 1536, 2, 2, 256, 1, 1)]


@pytest.mark.parametrize("case", CONV_TRAIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_batch_statistics_forward(lib, device, case):
    B, Cin, H, W, Cout, K, stride = case
    Ho, pt, pb = same_pad(H, K, stride)
    Wo, pl, pr = same_pad(W, K, stride)
    M = B * Ho * Wo
    assert M in (663, 16)
    g = torch.Generator().manual_seed(sum(case) + 17)
    x0 = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64).float().double()
    w0 = (torch.randn(Cout, Cin, K, K, generator=g, dtype=torch.float64) / (Cin * K * K) ** 0.5).float().double()
    y = {dt: F.conv2d(F.pad(x0.to(dt), [pl, pr, pt, pb]), w0.to(dt), None, stride) for dt in (torch.float64, torch.float32)}
    xd, wd = nhwc(x0.float()).to(device), w0.float().to(device).contiguous()
    out = torch.full((B, Ho, Wo, Cout), float("nan"), device=device)
    stats = torch.full((2, Cout), float("nan"), device=device)
    nblk = ctypes.c_int(-1)
    _lib.check(lib.orbit_op_conv2d_train(_lib.dptr(xd), 0, _lib.dptr(wd), _lib.dptr(out), None, B, H, W, Cin, Cout, K, K, stride, pt,
                                         pl, Ho, Wo, _lib.dptr(stats), ctypes.byref(nblk), _st()), "orbit_op_conv2d_train")
    torch.cuda.synchronize()
    what = "conv train " + "x".join(map(str, case))
    r = gate(out.cpu().permute(0, 3, 1, 2), y[torch.float64], _e32(y[torch.float32], y[torch.float64]), what + " y")
    if nblk.value > 0:  # (a launch shape that emits no partials leaves the statistics to the pass of its own)
        r = max(r, _stats_gate(stats, M, y[torch.float64], y[torch.float32], what))
    print("\n[effnetv2-wgrad-ops] %s: %d statistics blocks, largest err / e32 %.2f" % (what, nblk.value, r))


# (B, C, H, W, stride)
DW_TRAIN_CASES = [(3, 24, 17, 13, 1), (4, 1536, 2, 2, 1), (4, 1536, 4, 4, 2)]


@pytest.mark.parametrize("case", DW_TRAIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv_batch_statistics_forward(lib, device, case):
    B, C, H, W, stride = case
    Ho, pt, pb = same_pad(H, 3, stride)
    Wo, pl, pr = same_pad(W, 3, stride)
    M = B * Ho * Wo
    assert M in (663, 16)
    g = torch.Generator().manual_seed(sum(case) + 19)
    x0 = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 1.5).float().double()
    w0 = (torch.randn(C, 1, 3, 3, generator=g, dtype=torch.float64) / 3).float().double()
    y = {dt: F.conv2d(F.pad(x0.to(dt), [pl, pr, pt, pb]), w0.to(dt), None, stride, 0, 1, C) for dt in (torch.float64, torch.float32)}
    xd, wd = nhwc(x0.float()).to(device), w0.float().to(device).contiguous()
    out = torch.full((B, Ho, Wo, C), float("nan"), device=device)
    stats = torch.full((2, C), float("nan"), device=device)
    _lib.check(lib.orbit_op_dwconv2d_train(_lib.dptr(xd), _lib.dptr(wd), _lib.dptr(out), None, None, 0, B, H, W, C, 3, stride, pt, pl,
                                           Ho, Wo, _lib.dptr(stats), _st()), "orbit_op_dwconv2d_train")
    torch.cuda.synchronize()
    what = "dwconv train " + "x".join(map(str, case))
    r = gate(out.cpu().permute(0, 3, 1, 2), y[torch.float64], _e32(y[torch.float32], y[torch.float64]), what + " y")
    r = max(r, _stats_gate(stats, M, y[torch.float64], y[torch.float32], what))
    print("\n[effnetv2-wgrad-ops] %s: largest err / e32 %.2f" % (what, r))
