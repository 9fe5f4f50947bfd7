"""The compile-time epilogue forms of conv_igemm_kernel (csrc/conv_igemm.hip, ConvEpi) against its generic epilogue, bit for bit.

Every lean instantiation - both tiles (64x64 by conv_tile = 3, 128x32 by conv_tile = 4), BK 16 (Cin 48) and 32 (Cin 64), gated
and ungated, each (activation, residual) pair - runs orbit_op_conv2d_ex twice on the same inputs: as conv_plan chooses and with
ORBIT_CONV_EPILOGUE_GENERIC; the outputs must be torch.equal. The shapes are the smallest that reach every predicate of the
form: B = 2 frames of 7x7, M = 98 rows = one full and one partial 64-row tile / one partial 128-row tile whose rows beyond M are
clamped; Cout 40 and 80 leave the last column tile partly filled on both tilings, Cout 128 fills it. The output buffer is
NaN-filled and carries guard rows behind row M: an unwritten output or a store past the tensor fails the comparison.
(ReLU / SiLU with a residual have no lean form, and the skip without a gate on a single 64-wide column tile - Cout 40 under
conv_tile = 3 - is kept generic by a measured rule of conv_plan: both launches are generic there, which
tests/test_conv_epilogue_plan.py says on the CPU and the plan query repeats here. Cout 80 and 128 reach that instantiation.)"""
import ctypes
import itertools

import pytest
import torch

from orbit_dataset_amd import _lib

pytestmark = pytest.mark.gpu

FLAG_GENERIC = 4  # ORBIT_CONV_EPILOGUE_GENERIC
B, H, W = 2, 7, 7
GUARD = 4  # rows behind the output
LEAN_OF = {(0, 0): 1, (1, 0): 2, (2, 0): 3, (0, 1): 4, (1, 1): 0, (2, 1): 0}  # (act, residual) -> ConvEpi
OPTS = {"conv_bk": 0, "conv_splitk": 1, "conv_rgemm": 0, "conv_bf3": 0}
_inputs = {}


def expected_epilogue(tile, Cout, act, residual, gated):
    if tile == 3 and Cout <= 64 and residual and not gated:  # conv_plan: measured slower in the compile-time form
        return 0
    return LEAN_OF[act, residual]


def inputs(Cin, Cout):
    """One set of tensors per (Cin, Cout), shared by every case that uses it and never written."""
    if (Cin, Cout) not in _inputs:
        g = torch.Generator(device="cuda").manual_seed(1000 * Cin + Cout)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
        _inputs[Cin, Cout] = dict(x=r(B, H, W, Cin), w=r(Cout, Cin, 1, 1) * Cin ** -0.5, scale=1.0 + 0.2 * r(Cout), shift=0.5 * r(Cout),
                                  res=r(B, H, W, Cout), gate=torch.rand(B, Cin, device="cuda", generator=g))
    return _inputs[Cin, Cout]


def run(lib, t, Cin, Cout, act, residual, gated, flags):
    M = B * H * W
    y = torch.full((M + GUARD, Cout), float("nan"), device="cuda")
    rc = lib.orbit_op_conv2d_ex(_lib.dptr(t["x"]), 0, _lib.dptr(t["w"]), _lib.dptr(y), _lib.dptr(t["scale"]), _lib.dptr(t["shift"]),
                                _lib.dptr(t["res"]) if residual else None, _lib.dptr(t["gate"]) if gated else None,
                                B, H, W, Cin, Cout, 1, 1, 1, 0, 0, H, W, act, 0, flags, _lib.stream_handle())
    _lib.check(rc, "orbit_op_conv2d_ex")
    torch.cuda.synchronize()
    return y


def planned_epilogue(lib, Cin, Cout, act, residual, gated, flags):
    row = ctypes.create_string_buffer(48)
    a, b, c, e = (ctypes.c_int(-1) for _ in range(4))
    rc = lib.orbit_op_conv2d_plan_ex(B, H, W, Cin, Cout, 1, 1, 1, 0, 0, H, W, 0, 0, gated, residual, flags, 0, 0, act, row,
                                     ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(e))
    _lib.check(rc, "orbit_op_conv2d_plan_ex")
    return row.value.decode(), e.value


@pytest.mark.parametrize("tile,Cin,gated", list(itertools.product((3, 4), (48, 64), (0, 1))),
                         ids=lambda v: str(v))
def test_lean_epilogue_equals_generic_bitwise(lib, device, tile, Cin, gated):
    prev = {k: lib.orbit_get_option(k.encode()) for k in list(OPTS) + ["conv_tile"]}
    try:
        for k, v in dict(OPTS, conv_tile=tile).items():
            lib.orbit_set_option(k.encode(), v)
        expect_row = "conv_igemm<%s,%d,nhwc%s,pw>" % ("64,64" if tile == 3 else "128,32", 16 if Cin == 48 else 32, ",gate" if gated else "")
        for Cout, act, residual in itertools.product((40, 80, 128), (0, 1, 2), (0, 1)):
            t = inputs(Cin, Cout)
            assert planned_epilogue(lib, Cin, Cout, act, residual, gated, 0) == (expect_row, expected_epilogue(tile, Cout, act, residual, gated))
            assert planned_epilogue(lib, Cin, Cout, act, residual, gated, FLAG_GENERIC) == (expect_row, 0)
            lean = run(lib, t, Cin, Cout, act, residual, gated, 0)
            generic = run(lib, t, Cin, Cout, act, residual, gated, FLAG_GENERIC)
            M = B * H * W
            assert bool(torch.isnan(lean[M:]).all()) and bool(torch.isnan(generic[M:]).all()), "store behind the last row"
            assert bool(torch.isfinite(generic[:M]).all()), (Cout, act, residual)
            assert torch.equal(lean[:M], generic[:M]), (Cout, act, residual, float((lean[:M] - generic[:M]).abs().max()))
    finally:
        for k, v in prev.items():
            lib.orbit_set_option(k.encode(), v)


def test_generic_epilogue_matches_fp64_on_these_shapes(lib, device):
    """The yardstick of the comparison above is the generic form itself: one case per tile against an fp64 reference, so that
    two equal wrong outputs cannot pass. Tolerance: fp32 products summed over K = 64 terms of magnitude <= |x||w|, bound by
    K * eps * sum |x w| per output, times the scale, doubled for the SiLU's two ~1 ulp transcendentals."""
    Cin, Cout = 64, 80
    t = inputs(Cin, Cout)
    prev = {k: lib.orbit_get_option(k.encode()) for k in list(OPTS) + ["conv_tile"]}
    try:
        for tile in (3, 4):
            for k, v in dict(OPTS, conv_tile=tile).items():
                lib.orbit_set_option(k.encode(), v)
            y = run(lib, t, Cin, Cout, 2, 0, 1, FLAG_GENERIC)[:B * H * W].double().cpu()
            xg = (t["x"] * t["gate"][:, None, None, :]).double().cpu().reshape(-1, Cin)
            w = t["w"].double().cpu().reshape(Cout, Cin)
            pre = xg @ w.T * t["scale"].double().cpu() + t["shift"].double().cpu()
            ref = pre * torch.sigmoid(pre)
            bound = 2 * (Cin * 2.0 ** -24 * (xg.abs() @ w.abs().T) * t["scale"].double().cpu().abs() + 2.0 ** -22 * (1 + pre.abs()))
            assert bool(((y - ref).abs() <= bound).all()), float(((y - ref).abs() / bound).max())
    finally:
        for k, v in prev.items():
            lib.orbit_set_option(k.encode(), v)
