"""The epilogue-form rule of conv_plan (csrc/conv_igemm.hip), through the host-only orbit_op_conv2d_plan_ex: no GPU.

A compile-time ("lean") epilogue form of conv_igemm_kernel is planned exactly for an inference launch of a stride-1 pointwise
conv with Cin % 16 == 0 on a whole 64x64 / 128x32 tile that stores one activated output, for the instantiated (activation,
residual) pairs: none, ReLU, SiLU without a residual and none with one. Statistics, the statistics sweep, dual output, split-K,
fused pooling, the post-activation skip, the four K-waves (,k4), K x K filters, strided or K-padded pointwise convs and the
narrow K-tile plan generic, and so does the one class measured slower in the compile-time form: the skip without a gate on the
64x64 tile with a single column tile; ORBIT_CONV_EPILOGUE_GENERIC plans generic everywhere; the profiler row never depends on the form.
tests/test_gpu_conv_epilogue_forms.py runs the same shapes and leans on this file for which launches are lean."""
import ctypes
import itertools

import pytest

from orbit_dataset_amd import _lib

GENERIC, NONE, RELU, SILU, NONE_RES = 0, 1, 2, 3, 4  # ConvEpi of csrc/common.h
ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2               # ORBIT_ACT_*
FLAG_RPOST, FLAG_GENERIC = 1, 4                      # ORBIT_CONV_RESIDUAL_POST_ACT, ORBIT_CONV_EPILOGUE_GENERIC
LEAN_OF = {(ACT_NONE, 0): NONE, (ACT_RELU, 0): RELU, (ACT_SILU, 0): SILU, (ACT_NONE, 1): NONE_RES,
           (ACT_RELU, 1): GENERIC, (ACT_SILU, 1): GENERIC}
FIXED = {"conv_bk": 0, "conv_splitk": 1, "conv_rgemm": 0, "conv_bf3": 0}


class options:
    def __init__(self, lib, **kv):
        self.lib, self.kv = lib, kv

    def __enter__(self):
        self.prev = {k: self.lib.orbit_get_option(k.encode()) for k in self.kv}
        for k, v in self.kv.items():
            self.lib.orbit_set_option(k.encode(), v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.lib.orbit_set_option(k.encode(), v)
        return False


def pointwise(B, H, W, Cin, Cout, stride=1):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return (B, H, W, Cin, Cout, 1, 1, stride, 0, 0, Ho, Wo)


def plan(lib, geom, act=ACT_NONE, gated=0, residual=0, flags=0, pool2=0, stats_mode=0, dual=0):
    """(row, ksplit, m_tiles, epilogue) of orbit_op_conv2d_plan_ex; geom = (B, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo)."""
    row = ctypes.create_string_buffer(48)
    ks, per, mt, epi = (ctypes.c_int(-1) for _ in range(4))
    rc = lib.orbit_op_conv2d_plan_ex(*geom, 0, pool2, gated, residual, flags, stats_mode, dual, act, row, ctypes.byref(ks),
                                     ctypes.byref(per), ctypes.byref(mt), ctypes.byref(epi))
    assert rc == 0, _lib.last_error()
    return row.value.decode(), ks.value, mt.value, epi.value


@pytest.mark.parametrize("tile,Cin,gated", list(itertools.product((3, 4), (48, 64), (0, 1))))
def test_lean_forms_are_planned_for_their_pairs_and_only_those(lib, tile, Cin, gated):
    BM, BN = (64, 64) if tile == 3 else (128, 32)
    expect_row = "conv_igemm<%d,%d,%d,nhwc%s,pw>" % (BM, BN, 16 if Cin == 48 else 32, ",gate" if gated else "")
    with options(lib, conv_tile=tile, **FIXED):
        for Cout, act, residual in itertools.product((40, 80, 128), (ACT_NONE, ACT_RELU, ACT_SILU), (0, 1)):
            geom = pointwise(2, 7, 7, Cin, Cout)
            row, ksplit, m_tiles, epi = plan(lib, geom, act, gated, residual)
            assert (row, ksplit, m_tiles) == (expect_row, 1, 0)
            slower = tile == 3 and Cout <= 64 and residual and not gated  # the measured exception (below)
            assert epi == (GENERIC if slower else LEAN_OF[act, residual]), (Cout, act, residual)
            # the launch-level switch plans generic; the row is the same, and the same as the plain plan query's
            assert plan(lib, geom, act, gated, residual, flags=FLAG_GENERIC) == (expect_row, 1, 0, GENERIC)
            r0 = ctypes.create_string_buffer(48)
            a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            assert lib.orbit_op_conv2d_plan(*geom, 0, 0, gated, residual, 0, 0, 0, r0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
            assert r0.value.decode() == expect_row


@pytest.mark.parametrize("name,kwargs,row_has", [
    ("statistics", dict(geom=pointwise(2, 7, 7, 64, 128), stats_mode=1), ",pw>"),
    ("statistics_sweep", dict(geom=pointwise(2, 7, 7, 64, 128), stats_mode=2), ",pw,stats>"),
    ("dual_output", dict(geom=pointwise(2, 7, 7, 64, 128), dual=1, act=ACT_SILU), ",pw>"),
    ("split_k", dict(geom=pointwise(2, 7, 7, 1152, 128), act=ACT_SILU), ",pw,splitk>"),
    ("pooled", dict(geom=pointwise(2, 8, 8, 64, 128), pool2=1, act=ACT_RELU), ",pool2>"),
    ("rpost", dict(geom=(2, 7, 7, 32, 128, 3, 3, 1, 1, 1, 7, 7), residual=1, flags=FLAG_RPOST, act=ACT_SILU), ",rpost>"),
    ("k_by_k", dict(geom=(2, 7, 7, 32, 128, 3, 3, 1, 1, 1, 7, 7), act=ACT_SILU), "<64,64,32,nhwc>"),
    ("strided_pointwise", dict(geom=pointwise(2, 7, 7, 64, 128, stride=2), act=ACT_NONE), ",pw>"),
    ("k_tile_8", dict(geom=pointwise(2, 7, 7, 40, 128), act=ACT_SILU), "<64,64,8,nhwc,pw>"),
    ("k_padded", dict(geom=pointwise(2, 7, 7, 20, 128), act=ACT_SILU), "<64,64,8,nhwc,pw>"),
])
def test_everything_else_plans_generic(lib, name, kwargs, row_has):
    with options(lib, conv_tile=3, **FIXED):
        row, ksplit, m_tiles, epi = plan(lib, **kwargs)
    assert row_has in row, row
    assert (ksplit > 1) == (name == "split_k")
    assert epi == GENERIC


def test_four_k_waves_plan_generic(lib):
    """Few tiles at BK 32: the heuristic takes the 32x32 tile with four K-waves, which has no lean form; so does conv_tile = 6."""
    for tile in (0, 6):
        with options(lib, conv_tile=tile, **FIXED):
            row, _, _, epi = plan(lib, pointwise(2, 7, 7, 64, 128), ACT_SILU)
        assert row == "conv_igemm<32,32,32,nhwc,pw,k4>" and epi == GENERIC


def test_the_network_shapes_of_the_issue_plan_lean(lib):
    """EfficientNet-B0's 14x14 / 7x7 dense layers at 200 frames under the default options but conv_rgemm = 0 (which routes
    1152 -> 320 to the register GEMM): expansions and conv_head SiLU, projections none with / without the skip."""
    with options(lib, conv_tile=0, **FIXED):
        for H, Cin, Cout, act, gated, residual, want in [
                (14, 80, 480, ACT_SILU, 0, 0, SILU), (14, 112, 672, ACT_SILU, 0, 0, SILU), (7, 192, 1152, ACT_SILU, 0, 0, SILU),
                (7, 320, 1280, ACT_SILU, 0, 0, SILU), (14, 480, 112, ACT_NONE, 1, 0, NONE), (14, 480, 80, ACT_NONE, 1, 1, NONE_RES),
                (14, 672, 112, ACT_NONE, 1, 1, NONE_RES), (7, 672, 192, ACT_NONE, 1, 0, NONE), (7, 1152, 192, ACT_NONE, 1, 1, NONE_RES),
                (7, 1152, 320, ACT_NONE, 1, 0, NONE)]:
            row, ksplit, _, epi = plan(lib, pointwise(200, H, H, Cin, Cout), act, gated, residual)
            assert row.startswith("conv_igemm<") and ",pw" in row and ksplit == 1, row
            assert epi == want, (row, epi)


def test_the_ungated_skip_on_one_64_wide_column_tile_stays_generic(lib):
    """240 -> 40 @28x28 with a skip and without a gate was 4 % slower in the compile-time form on two boxes
    (profiles/r08_conv_epilogue_ab.txt): that class - no gate, a residual, the 64x64 tile, one column tile, at either K-tile,
    such as efficientnet_v2_s's 256 -> 64 @28x28 - plans generic. With the gate, on the 128x32 tile or on more than one column
    tile the same launches keep the compile-time form."""
    with options(lib, conv_tile=0, **FIXED):
        for H, Cin, Cout, gated, want_tile, want in [
                (28, 240, 40, 0, "<64,64,16,", GENERIC), (28, 256, 64, 0, "<64,64,32,", GENERIC), (28, 144, 40, 0, "<64,64,16,", GENERIC),
                (28, 240, 40, 1, "<64,64,16,", NONE_RES), (14, 672, 112, 0, "<64,64,16,", NONE_RES), (7, 1152, 192, 0, "<64,64,32,", NONE_RES),
                (56, 144, 24, 0, "<128,32,16,", NONE_RES), (14, 480, 80, 0, "<128,32,16,", NONE_RES)]:
            row, _, _, epi = plan(lib, pointwise(200, H, H, Cin, Cout), ACT_NONE, gated, residual=1)
            assert want_tile in row, row
            assert epi == want, (row, epi)
            # without the skip the same launch is lean
            assert plan(lib, pointwise(200, H, H, Cin, Cout), ACT_NONE, gated, residual=0)[3] == NONE


def test_unknown_flags_are_refused(lib):
    row = ctypes.create_string_buffer(48)
    a, b, c, e = (ctypes.c_int() for _ in range(4))
    rc = lib.orbit_op_conv2d_plan_ex(*pointwise(2, 7, 7, 64, 128), 0, 0, 0, 0, 2, 0, 0, 0, row, ctypes.byref(a), ctypes.byref(b),
                                     ctypes.byref(c), ctypes.byref(e))
    assert rc != 0 and "unknown flags" in _lib.last_error()
