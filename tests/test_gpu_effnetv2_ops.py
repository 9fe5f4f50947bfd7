"""The conv epilogue form efficientnet_v2_s adds (csrc/conv_igemm.hip, RPOST), through orbit_op_conv2d_ex: the skip joins AFTER
the activation, y = act(conv(x) * scale + shift) + residual (timm ConvBnAct), in the whole-tile epilogue of each tiling and in the
split-K reduce kernel.

Gate: against the float64 evaluation, max |error| <= max(2e-5, 4 x E32) x max(1, max |y|), where E32 is the error of the same
expression evaluated in float32 on the CPU and 2e-5 the project's bound for fp32 kernels on O(1) values (tests/test_gpu_ops.py):
the kernel is an fp32 multiply-add chain over K = 216 .. 576 products like the CPU's, in another order, with the hardware exp / rcp
in SiLU."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402

POST = 1  # ORBIT_CONV_RESIDUAL_POST_ACT
SILU = 2


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _st():
    return _lib.stream_handle()


def run_conv_ex(lib, device, x, w, scale, shift, residual, flags, act=SILU):
    """3x3 stride-1 SAME conv of NCHW `x` through orbit_op_conv2d_ex; returns NCHW on the CPU."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    keep = [t.to(device).contiguous() for t in (nhwc(x), w, scale, shift, nhwc(residual))]
    y = torch.full((B, H, W, Cout), float("nan"), device=device)
    rc = lib.orbit_op_conv2d_ex(_lib.dptr(keep[0]), 0, _lib.dptr(keep[1]), _lib.dptr(y), _lib.dptr(keep[2]), _lib.dptr(keep[3]),
                                _lib.dptr(keep[4]), None, B, H, W, Cin, Cout, 3, 3, 1, 1, 1, H, W, act, 0, flags, _st())
    _lib.check(rc, "orbit_op_conv2d_ex")
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2)


def _case(C, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W = 2, 9, 7  # 126 GEMM rows: ragged against the 64- and the 128-row tile
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g) * 0.3
    return x, w, scale, shift


def _ref(x, w, scale, shift, post, dtype):
    x, w, scale, shift = (t.to(dtype) for t in (x, w, scale, shift))
    y = F.conv2d(x, w, None, 1, 1) * scale[None, :, None, None] + shift[None, :, None, None]
    return F.silu(y) + x if post else F.silu(y + x)


def _gate(got, x, w, scale, shift, what):
    want = _ref(x, w, scale, shift, True, torch.float64)
    e32 = (_ref(x, w, scale, shift, True, torch.float32).double() - want).abs().max().item()
    tol = max(2e-5, 4 * e32) * max(1.0, want.abs().max().item())
    err = (got.double() - want).abs().max().item()
    print("\n[rpost] %s: err %.3g, E32 %.3g, tol %.3g" % (what, err, e32, tol))
    assert not torch.isnan(got).any(), what
    assert err <= tol, (what, err, tol)
    pre = _ref(x, w, scale, shift, False, torch.float64)
    assert (want - pre).abs().max().item() > 1e-3  # the two forms differ: the old epilogue cannot pass
    assert (got.double() - pre).abs().max().item() > 1e-3, what


@pytest.mark.parametrize("tile", [0, 3, 4])
def test_post_activation_skip_24_to_24(lib, device, tile):
    """efficientnet_v2_s stage 0: 3x3 s1, 24 -> 24, residual = input, SiLU. conv_tile 0 = the rule (128 x 32 for Cout <= 32),
    3 = 64 x 64, 4 = 128 x 32. All of them run the batched epilogue site; the row-loop site of the kernel is compiled only for
    tilings with more than 8 output rows per thread, which no post-activation instantiation has (4, 4 and 1 rows): the edit
    there is dead code today, correct by reading, and no test reaches it."""
    x, w, scale, shift = _case(24, 5)
    prev = lib.orbit_get_option(b"conv_tile")
    lib.orbit_set_option(b"conv_tile", tile)
    try:
        got = run_conv_ex(lib, device, x, w, scale, shift, x, POST)
        old = run_conv_ex(lib, device, x, w, scale, shift, x, 0)
    finally:
        lib.orbit_set_option(b"conv_tile", prev)
    _gate(got, x, w, scale, shift, "24->24 tile %d" % tile)
    pre = _ref(x, w, scale, shift, False, torch.float64)
    assert (old.double() - pre).abs().max().item() <= 2e-5 * max(1.0, pre.abs().max().item())  # flags = 0 is orbit_op_conv2d


def test_post_activation_skip_through_split_k(lib, device):
    """64 -> 64 at 126 rows: 2 output tiles and 18 K-tiles of 32 - conv_splitk's rule cuts it three ways, so the epilogue runs
    in conv_splitk_reduce_kernel. With the option off the same conv takes the whole-tile epilogue (32 x 32 tiles, four
    K-waves): both against float64, and the two differ in their last bits (another summation order ran)."""
    x, w, scale, shift = _case(64, 9)
    got = run_conv_ex(lib, device, x, w, scale, shift, x, POST)
    prev = lib.orbit_get_option(b"conv_splitk")
    lib.orbit_set_option(b"conv_splitk", 0)
    try:
        unsplit = run_conv_ex(lib, device, x, w, scale, shift, x, POST)
    finally:
        lib.orbit_set_option(b"conv_splitk", prev)
    _gate(got, x, w, scale, shift, "64->64 split-K")
    _gate(unsplit, x, w, scale, shift, "64->64 unsplit")
    assert not torch.equal(got, unsplit)


def test_post_activation_skip_refuses_what_it_is_not_compiled_for(lib, device):
    """A pointwise conv, a gate, fused pooling, the NCHW stem or a missing residual with the flag, and an unknown flag: argument
    errors, no convolution is launched."""
    x = torch.zeros(1, 5, 5, 24, device=device)
    x3 = torch.zeros(1, 3, 5, 5, device=device)
    w1, w3, ws = (torch.zeros(s, device=device) for s in ((24, 24, 1, 1), (24, 24, 3, 3), (24, 3, 3, 3)))
    y, gate = torch.zeros(1, 5, 5, 24, device=device), torch.ones(1, 24, device=device)
    p = _lib.dptr

    def call(xx, nchw, ww, res, gt, Cin, K, pad, pool2, flags):
        return lib.orbit_op_conv2d_ex(p(xx), nchw, p(ww), p(y), None, None, p(res), p(gt), 1, 5, 5, Cin, 24, K, K, 1, pad, pad, 5, 5,
                                      SILU, pool2, flags, _st())

    for args in ((x, 0, w1, x, None, 24, 1, 0, 0, POST), (x, 0, w3, x, gate, 24, 3, 1, 0, POST), (x, 0, w3, x, None, 24, 3, 1, 1, POST),
                 (x3, 1, ws, x, None, 3, 3, 1, 0, POST), (x, 0, w3, None, None, 24, 3, 1, 0, POST), (x, 0, w3, x, None, 24, 3, 1, 0, 2)):
        assert call(*args) == -1, args
        assert "post-activation" in _lib.last_error() or "flags" in _lib.last_error() or "pool2" in _lib.last_error()
    torch.cuda.synchronize()
