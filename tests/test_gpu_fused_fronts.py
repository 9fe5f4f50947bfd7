"""The row-streaming fused fronts of csrc/mbconv_rows.hip, instantiation by instantiation against float64 on the CPU:

    mbconv_rows3_kernel<.., EXACT | predicated>          orbit_op_mbconv_front       expand 1x1 -> BN1 -> SiLU -> depthwise -> BN2 -> SiLU
    mbconv_rows3_kernel<.., EXACT | predicated, RAW>     orbit_op_mbconv_front_raw   ... -> raw depthwise outputs + per-tile sum / sum of squares
    mbconv_rows3_kernel<.., EXACT, BF3>                  orbit_op_mbconv_front under conv_bf3 = 2
    stem_rows_kernel<EXACT | predicated>                 orbit_op_stem_dw_front      stem 3x3/2 -> BN -> SiLU -> depthwise 3x3 -> BN -> SiLU

for the five (K, stride, Cin) geometries the kernel serves, each on maps that tile exactly (branch-free stores) and on maps that do
not (ragged strip, ragged band, partly filled channel chunk: predicated stores). Every case is named after its tiling and first
asserts, through orbit_op_mbconv_front_plan / orbit_op_stem_dw_front_plan, the strips, bands and `exact` flag it claims
(tests/test_fused_fronts_reference.py checks the same tables, and the inputs' properties, without a GPU). Every output buffer is
pre-filled with NaN and followed by a guard tail of sentinel floats (Guarded of test_gpu_se_path.py).

Input families: `normal` (the Gaussians of tests/test_gpu_ops.py), `one_sign` (x, weights / fan-in and scales uniform in
[0.75, 1.25], shifts uniform in [0.375, 0.625]: every product positive, every output away from 0, so that one dropped or doubled
output breaks a tile's summation bound), `centred` (normal with every channel's depthwise taps summing to 0: the raw outputs then
satisfy |mu_c| <= sigma_c, the condition of test_gpu_bn_chain.py's Gaussian gates) and `impulse` (one non-zero pixel per frame at
the corners and on both sides of every strip and band seam, shift1 = 0, distinct taps, scale2 = 1, shift2 = 0: a swapped tap, a
shifted window or a seam off by one moves a value to another pixel; outside the impulse's footprint y must be exactly 0).

Bounds (u = 2^-24; none is taken from a kernel's output):
  y, raw y          elementwise_gate of test_gpu_se_path.py: max(2e-5, 4 E32) max(1, max |ref64|), E32 the error of the fp32 CPU
                    evaluation of the same closed form. The BF3 form is held to the same gate (its six-product sums differ from
                    the exact products by at most 2^-23 of them, tests/test_bf3_numerics.py: inside the gate's floor)
  pooling partials  per tile |partial - S| <= 2 n u A, S / A the float64 sum / magnitude sum of the n outputs THE KERNEL WROTE in the
                    tile's rectangle; their sum over the tiles against the plane sum at 2 Ho Wo u A
  RAW sums          the same bound;  RAW sums of squares: |partial - Q| <= 2 (n + 1) u Q, Q the float64 sum of the squares of the
                    written fp32 outputs (one rounding per square, n - 1 per sum, the factor 2 of the other summation bounds)
  RAW chain link    (centred) orbit_op_bn_stats_from_partials on the kernel's partials against the float64 statistics of the written
                    y: mean 1e-6 max(1, max |mean|), |invstd - ref| sqrt(var + eps) <= 1e-5
  bit identity      frame 0 of a B = 3 launch against a B = 1 launch (y and partial rows); y with and without pool_partial

Each check prints "[fused_fronts] family: case: err, bound, ratio" (pytest -s). Largest err / bound per kernel form on the MI355X
(152 tests, 763 checks, 1.7 s in all; every case met every gate and every bit identity held, no kernel had to change - the library
gained the two plan queries and the raw entry only):
  front exact   y 0.018 (k5s2c24_2x2/one_sign: 8.4e-07 of 4.6e-05)   partials 0.11 (k3s2c40_2x2/one_sign tile 3), plane 0.051
                impulses: y 0.015 (k3s1c24_two_strips), sums 0.045
  front pred    y 0.019 (k5s2c24_ragged/one_sign: 8.1e-07 of 4.3e-05)   partials 0.16 (k3s2c40_ragged/one_sign tile 3), plane 0.033
                impulses: y 0.006, sums 0.001 (k3s2c16_strips_15_14_quarter_chunk)
  raw exact     y 0.018 (k3s2c40_one_tile/centred: 1.8e-06 of 1.0e-04)   sums 0.11 (k5s2c24_2x2/one_sign tile 3), plane 0.042
                sums of squares 0.12 (k3s2c40_2x2/normal tile 3)   chain mean 0.033 (k3s2c40_one_tile), invstd 0.015 (k5s2c24_one_tile)
                impulses: y 0.013, sums 0.036, sums of squares 0.046 (k5s2c24_2x2 tile 3)
  raw pred      y 0.015 (k5s1c40_ragged_strips/one_sign)   sums 0.18 (k3s2c40_ragged/one_sign tile 2), plane 0.035
                sums of squares 0.18 (k3s2c40_ragged/normal tile 2)   chain mean 0.026, invstd 0.014 (k5s1c40_ragged_bands)
                impulses: y 0.004, sums 0.001, sums of squares 0.015 (k3s2c16_strips_15_14_quarter_chunk)
  bf3 exact     y 0.017 (k5s1c40_2x2_bands_28_4/one_sign: 8.2e-07 of 4.8e-05)   partials 0.11 (k3s2c40_2x2/one_sign tile 3), plane 0.004
                bits differ from the fp32 form in the four geometries with a BF3 instantiation, equal for 40 -> ., 3x3 / 2
  stem exact    y 0.014 (stem_3_strips/one_sign)   partials 0.058 (stem_2_strips_3_bands/one_sign tile 5), plane 0.014
                impulses: y 0.003, sums 0.025
  stem pred     y 0.015 (stem_ragged_57x30/normal)   partials 0.10, plane 0.10 (stem_3x3/one_sign)
"""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
import test_gpu_se_path as SE  # noqa: E402
from test_gpu_se_path import Guarded, U, elementwise_gate, options, same_pad  # noqa: E402

EPS = 1e-5
EPS32 = float(np.float32(EPS))
INF = float("inf")

_report = functools.partial(SE._report, tag="fused_fronts")


def _egate(family, what, got, want64, want32):
    elementwise_gate(family, what, got, want64, want32, report=_report)


def _st():
    return _lib.stream_handle()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- the case tables ------------------------------------------------------------------------------------------------------------------
# name, Cin, mid, K, stride, H, W, B, exact, strips, bands, seams (the impulse / BF3 / NULL-pool cases of a geometry)
MbCase = collections.namedtuple("MbCase", "name Cin mid K stride H W B exact strips bands seams")
MB_CASES = [MbCase(*c) for c in [
    # 16 -> ., 3x3 / 2 (one output row per step, one output per item)
    ("k3s2c16_one_tile_3_blocks", 16, 96, 3, 2, 12, 32, 1, 1, 1, 1, False),
    ("k3s2c16_2x2_bands_28_2", 16, 96, 3, 2, 60, 64, 3, 1, 2, 2, True),
    ("k3s2c16_half_chunk", 16, 80, 3, 2, 37, 21, 1, 1, 1, 1, False),
    ("k3s2c16_strips_15_14_quarter_chunk", 16, 72, 3, 2, 59, 58, 3, 0, 2, 2, True),
    # 24 -> ., 3x3 / 1 (two rows per step, two outputs per item)
    ("k3s1c24_one_tile", 24, 144, 3, 1, 8, 16, 1, 1, 1, 1, False),
    ("k3s1c24_two_bands", 24, 144, 3, 1, 30, 16, 3, 1, 1, 2, True),
    ("k3s1c24_two_strips", 24, 144, 3, 1, 6, 60, 3, 1, 2, 1, True),
    ("k3s1c24_bands_28_1_odd_width", 24, 100, 3, 1, 29, 17, 3, 0, 1, 2, False),
    ("k3s1c24_strips_30_29_8_blocks", 24, 100, 3, 1, 5, 59, 1, 0, 2, 1, False),
    # 24 -> ., 5x5 / 2
    ("k5s2c24_one_tile", 24, 144, 5, 2, 8, 16, 1, 1, 1, 1, False),
    ("k5s2c24_2x2", 24, 144, 5, 2, 60, 40, 3, 1, 2, 2, True),
    ("k5s2c24_ragged", 24, 100, 5, 2, 57, 29, 3, 0, 2, 2, False),
    ("k5s2c24_odd_rows_only", 24, 144, 5, 2, 42, 31, 1, 0, 2, 1, False),
    # 40 -> ., 5x5 / 1 (four rows per step, four outputs per item)
    ("k5s1c40_one_tile_8_blocks", 40, 240, 5, 1, 8, 8, 1, 1, 1, 1, False),
    ("k5s1c40_2x2_bands_28_4", 40, 240, 5, 1, 32, 32, 3, 1, 2, 2, True),
    ("k5s1c40_ragged_strips", 40, 236, 5, 1, 15, 29, 3, 0, 2, 1, False),
    ("k5s1c40_ragged_bands", 40, 236, 5, 1, 30, 10, 1, 0, 1, 2, False),
    ("k5s1c40_partial_step", 40, 240, 5, 1, 5, 8, 3, 0, 1, 1, False),
    # 40 -> ., 3x3 / 2 (no BF3 instantiation)
    ("k3s2c40_one_tile", 40, 240, 3, 2, 8, 16, 1, 1, 1, 1, False),
    ("k3s2c40_2x2", 40, 240, 3, 2, 60, 40, 3, 1, 2, 2, True),
    ("k3s2c40_ragged", 40, 236, 3, 2, 57, 30, 3, 0, 2, 2, False),
]]
MB_IDS = [c.name for c in MB_CASES]
MB_SEAM_CASES = [c for c in MB_CASES if c.seams]
MB_BF3_CASES = [c for c in MB_SEAM_CASES if c.exact]
HAS_BF3 = lambda c: (c.Cin, c.K, c.stride) != (40, 3, 2)  # noqa: E731

# name, FH, FW, B, exact, strips, bands (of the stem's ceil(FH / 2) x ceil(FW / 2) output grid), seams
StemCase = collections.namedtuple("StemCase", "name FH FW B exact strips bands seams")
STEM_CASES = [StemCase(*c) for c in [
    ("stem_one_tile", 16, 16, 1, 1, 1, 1, False),
    ("stem_2_strips_3_bands", 116, 64, 3, 1, 2, 3, True),
    ("stem_3_strips", 60, 120, 3, 1, 3, 2, False),
    ("stem_odd_19x23", 37, 45, 1, 0, 1, 1, False),
    ("stem_ragged_57x30", 113, 59, 3, 0, 2, 3, False),
    ("stem_3x3", 6, 5, 3, 0, 1, 1, False),
]]
STEM_IDS = [c.name for c in STEM_CASES]
STEM_MID = 32

FAMILIES = ["normal", "one_sign"]
FAMILY_SEED = {"normal": 1, "one_sign": 2, "centred": 1, "impulse": 4}  # (centred: the normal draw with each channel's taps centred)


def mb_out(c):
    """(Ho, pad_top, Wo, pad_left) of a case: TF-SAME."""
    Ho, _, pt = same_pad(c.H, c.K, c.stride)
    Wo, _, pl = same_pad(c.W, c.K, c.stride)
    return Ho, pt, Wo, pl


def mb_total(c):
    """Blocks of the launch: channel chunks x tiles x frames."""
    return -(-c.mid // 32) * c.strips * c.bands * c.B


# ---- the tiling, as the library reports it --------------------------------------------------------------------------------------------
PLAN_KEYS = ("strips", "bands", "strip_w", "band_rows", "exact")


def mb_plan(lib, c):
    v = [ctypes.c_int(-1) for _ in PLAN_KEYS]
    _lib.check(lib.orbit_op_mbconv_front_plan(c.H, c.W, c.Cin, c.mid, c.K, c.stride, *[ctypes.byref(x) for x in v]),
               "orbit_op_mbconv_front_plan")
    return dict(zip(PLAN_KEYS, (x.value for x in v)))


def stem_plan(lib, c):
    v = [ctypes.c_int(-1) for _ in PLAN_KEYS]
    _lib.check(lib.orbit_op_stem_dw_front_plan(-(-c.FH // 2), -(-c.FW // 2), STEM_MID, *[ctypes.byref(x) for x in v]),
               "orbit_op_stem_dw_front_plan")
    return dict(zip(PLAN_KEYS, (x.value for x in v)))


def tile_rects(plan, Ho, Wo):
    """(r0, r1, c0, c1) of tile t = band * strips + strip, clipped to the map (include/orbit_hip.h)."""
    out = []
    for band in range(plan["bands"]):
        for strip in range(plan["strips"]):
            r0, c0 = band * plan["band_rows"], strip * plan["strip_w"]
            out.append((r0, min(Ho, r0 + plan["band_rows"]), c0, min(Wo, c0 + plan["strip_w"])))
    return out


def assert_plan(plan, c, Ho, Wo):
    """The case's claims, and that the tiles are non-empty and cover the map once."""
    assert (plan["strips"], plan["bands"], plan["exact"]) == (c.strips, c.bands, c.exact), (c.name, plan)
    rects = tile_rects(plan, Ho, Wo)
    assert all(r1 > r0 and c1 > c0 for r0, r1, c0, c1 in rects), (c.name, rects)
    assert sum((r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in rects) == Ho * Wo, (c.name, rects)
    return rects


# ---- inputs and references (CPU; computed once per (case, family) and shared, never modified) ---------------------------------------
def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 1000003 + int(v)
    return torch.Generator().manual_seed(s % (2 ** 31))


def _family_params(family, g, mid, fan1, K):
    """(w1 scale, depthwise scale, s1, h1, s2, h2 makers) shared by the MBConv and stem inputs."""
    if family == "one_sign":
        pos = lambda *s: torch.rand(*s, generator=g) * 0.5 + 0.75  # noqa: E731
        sh = lambda *s: torch.rand(*s, generator=g) * 0.25 + 0.375  # noqa: E731
        return pos, 1.0 / fan1, 1.0 / (K * K), pos(mid), sh(mid), pos(mid), sh(mid)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    s1, h1 = torch.rand(mid, generator=g) + 0.5, rn(mid) * 0.3
    s2, h2 = torch.rand(mid, generator=g) + 0.5, rn(mid) * 0.1
    return rn, fan1 ** -0.5, 1.0 / K, s1, h1, s2, h2


def seam_positions(plan, H, W, stride):
    """Input pixels of the impulse frames: the four corners, and both sides of every strip seam and band seam (in input
    coordinates: output column strip * strip_w reads input column strip * strip_w * stride - pad_left and its neighbours), away
    from the other seams and at their crossings."""
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    cols = [min(W - 1, s * plan["strip_w"] * stride) for s in range(1, plan["strips"])]
    rows = [min(H - 1, b * plan["band_rows"] * stride) for b in range(1, plan["bands"])]
    for cs in cols:
        pos += [(H // 3, cs - 1), (H // 3, cs)]
    for rs in rows:
        pos += [(rs - 1, W // 3), (rs, W // 3)]
    for rs in rows:
        for cs in cols:
            pos += [(rs - 1, cs - 1), (rs, cs)]
    return pos


def _impulse_taps(mid, K):
    """Distinct, non-zero taps per channel: (1 + tap index + channel % 5) / (K K + 5)."""
    base = torch.arange(1, K * K + 1, dtype=torch.float32).view(1, 1, K, K)
    return (base + (torch.arange(mid) % 5).float().view(mid, 1, 1, 1)) / (K * K + 5)


def mb_inputs(c, family, plan=None):
    """x NCHW [B][Cin][H][W], w1 [mid][Cin][1][1], wd [mid][1][K][K], s1, h1, s2, h2."""
    g = _gen(c.Cin, c.mid, c.K, c.stride, c.H, c.W, FAMILY_SEED[family])
    if family == "impulse":
        pos = seam_positions(plan, c.H, c.W, c.stride)
        x = torch.zeros(len(pos), c.Cin, c.H, c.W)
        for b, (r, col) in enumerate(pos):
            x[b, :, r, col] = torch.randn(c.Cin, generator=g)
        w1 = torch.randn(c.mid, c.Cin, 1, 1, generator=g) * c.Cin ** -0.5
        return dict(x=x, w1=w1, wd=_impulse_taps(c.mid, c.K), s1=torch.rand(c.mid, generator=g) + 0.5, h1=torch.zeros(c.mid),
                    s2=torch.ones(c.mid), h2=torch.zeros(c.mid))
    r, k1, kd, s1, h1, s2, h2 = _family_params(family, g, c.mid, c.Cin, c.K)
    x = r(c.B, c.Cin, c.H, c.W)
    w1, wd = r(c.mid, c.Cin, 1, 1) * k1, r(c.mid, 1, c.K, c.K) * kd
    if family == "centred":
        wd = wd - wd.mean((2, 3), keepdim=True)
    return dict(x=x, w1=w1, wd=wd, s1=s1, h1=h1, s2=s2, h2=h2)


def _bc(v):
    return v[None, :, None, None]


def mb_ref(t, c, dtype):
    """(raw depthwise outputs, y) NHWC in `dtype`: silu(bn2(dw(pad(silu(bn1(x . w1^T)))))), TF-SAME padding of the EXPANDED tensor."""
    x, w1, wd, s1, h1, s2, h2 = (t[k].to(dtype) for k in ("x", "w1", "wd", "s1", "h1", "s2", "h2"))
    _, th, pt = same_pad(c.H, c.K, c.stride)
    _, tw, pl = same_pad(c.W, c.K, c.stride)
    e = F.silu(F.conv2d(x, w1) * _bc(s1) + _bc(h1))
    raw = F.conv2d(F.pad(e, [pl, tw - pl, pt, th - pt]), wd, None, c.stride, 0, 1, c.mid)
    return nhwc(raw), nhwc(F.silu(raw * _bc(s2) + _bc(h2)))


def _plan_key(plan):
    return None if plan is None else tuple(plan[k] for k in PLAN_KEYS)


@functools.lru_cache(maxsize=None)
def _mb_data(c, family, plan_key):
    plan = None if plan_key is None else dict(zip(PLAN_KEYS, plan_key))
    t = mb_inputs(c, family, plan)
    raw64, y64 = mb_ref(t, c, torch.float64)
    raw32, y32 = mb_ref(t, c, torch.float32)
    return dict(t, raw64=raw64, y64=y64, raw32=raw32, y32=y32)


def mb_data(c, family, plan=None):
    """Inputs and the float64 / float32 references of a case (shared between the tests: treat as read-only)."""
    return _mb_data(c, family, _plan_key(plan) if family == "impulse" else None)


def stem_inputs(c, family, plan=None):
    """frames NCHW [B][3][FH][FW], ws [32][3][3][3], wd [32][1][3][3], s1, h1, s2, h2."""
    mid = STEM_MID
    g = _gen(c.FH, c.FW, mid, FAMILY_SEED[family])
    if family == "impulse":
        pos = seam_positions(plan, c.FH, c.FW, 2)
        x = torch.zeros(len(pos), 3, c.FH, c.FW)
        for b, (r, col) in enumerate(pos):
            x[b, :, r, col] = torch.randn(3, generator=g)
        ws = torch.randn(mid, 3, 3, 3, generator=g) * 27 ** -0.5
        return dict(x=x, ws=ws, wd=_impulse_taps(mid, 3), s1=torch.rand(mid, generator=g) + 0.5, h1=torch.zeros(mid),
                    s2=torch.ones(mid), h2=torch.zeros(mid))
    r, k1, kd, s1, h1, s2, h2 = _family_params(family, g, mid, 27, 3)
    return dict(x=r(c.B, 3, c.FH, c.FW), ws=r(mid, 3, 3, 3) * k1, wd=r(mid, 1, 3, 3) * kd, s1=s1, h1=h1, s2=s2, h2=h2)


def stem_ref(t, c, dtype):
    """y NHWC: silu(bn2(dw3x3(silu(bn1(conv_stem 3x3 / 2, TF-SAME))), padding 1))."""
    x, ws, wd, s1, h1, s2, h2 = (t[k].to(dtype) for k in ("x", "ws", "wd", "s1", "h1", "s2", "h2"))
    _, th, pt = same_pad(c.FH, 3, 2)
    _, tw, pl = same_pad(c.FW, 3, 2)
    e = F.silu(F.conv2d(F.pad(x, [pl, tw - pl, pt, th - pt]), ws, None, 2) * _bc(s1) + _bc(h1))
    return nhwc(F.silu(F.conv2d(e, wd, None, 1, 1, 1, STEM_MID) * _bc(s2) + _bc(h2)))


@functools.lru_cache(maxsize=None)
def _stem_data(c, family, plan_key):
    plan = None if plan_key is None else dict(zip(PLAN_KEYS, plan_key))
    t = stem_inputs(c, family, plan)
    return dict(t, y64=stem_ref(t, c, torch.float64), y32=stem_ref(t, c, torch.float32))


def stem_data(c, family, plan=None):
    return _stem_data(c, family, _plan_key(plan) if family == "impulse" else None)


# ---- the checks -----------------------------------------------------------------------------------------------------------------------
def _bounded(family, what, err, bound):
    """err <= bound elementwise (tensors; a zero bound demands a zero error); reports the largest ratio."""
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, INF, 0.0)).max().item()
    _report(family, what, ratio, 1.0)
    assert not (err > bound).any(), (family, what, ratio, err.max().item())


def check_tile_sums(family, what, y, partial, rects):
    """partial [B][tiles][C] against the float64 sums of the outputs the kernel wrote (y NHWC fp32, CPU) in each tile's rectangle
    at 2 n u A, and the sum over the tiles against the plane sum at 2 Ho Wo u A."""
    B, Ho, Wo, C = y.shape
    assert tuple(partial.shape) == (B, len(rects), C)
    yd = y.double()
    for t, (r0, r1, c0, c1) in enumerate(rects):
        blk = yd[:, r0:r1, c0:c1]
        n = (r1 - r0) * (c1 - c0)
        _bounded(family, "%s tile %d" % (what, t), (partial[:, t].double() - blk.sum((1, 2))).abs(), 2.0 * n * U * blk.abs().sum((1, 2)))
    _bounded(family + "_plane", what, (partial.double().sum(1) - yd.sum((1, 2))).abs(), 2.0 * Ho * Wo * U * yd.abs().sum((1, 2)))


def check_tile_squares(family, what, y, partial, rects):
    """partial [B][tiles][C] against Q = the float64 sum of the squares of the written fp32 outputs of each tile at 2 (n + 1) u Q."""
    yd = y.double() ** 2
    for t, (r0, r1, c0, c1) in enumerate(rects):
        q = yd[:, r0:r1, c0:c1].sum((1, 2))
        n = (r1 - r0) * (c1 - c0)
        _bounded(family, "%s tile %d" % (what, t), (partial[:, t].double() - q).abs(), 2.0 * (n + 1) * U * q)


def check_footprint(what, got, want64):
    """Impulse frames: where the float64 reference is exactly 0 (outside the impulse's footprint) the kernel wrote exactly 0."""
    stray = (want64 == 0) & (got != 0)
    assert not stray.any(), (what, "non-zero outputs outside the impulse's footprint", stray.nonzero()[:4].tolist())
    assert (want64 != 0).any(), what


# ---- launches -------------------------------------------------------------------------------------------------------------------------
def run_mb_front(lib, device, t, c, B, raw=False, pool=True, bf3=0):
    """orbit_op_mbconv_front (raw: orbit_op_mbconv_front_raw) on the first B frames of the inputs; returns (y NHWC, partials
    [B][tiles][mid], raw: [B][tiles][2][mid], or None) on the CPU after the guard checks."""
    Ho, pt, Wo, pl = mb_out(c)
    tiles = c.strips * c.bands
    assert lib.orbit_op_mbconv_front_partials(c.H, c.W, c.Cin, c.mid, c.K, c.stride) == tiles
    d = _lib.dptr
    dev = {k: (nhwc(t[k][:B]) if k == "x" else t[k]).to(device).contiguous() for k in ("x", "w1", "wd", "s1", "h1", "s2", "h2")}
    y = Guarded((B, Ho, Wo, c.mid), device)
    geo = (B, c.H, c.W, c.Cin, c.mid, c.K, c.stride, pt, pl, Ho, Wo)
    with options(lib, conv_bf3=bf3):
        if raw:
            part = Guarded((B * tiles, 2, c.mid), device)
            _lib.check(lib.orbit_op_mbconv_front_raw(d(dev["x"]), d(dev["w1"]), d(dev["s1"]), d(dev["h1"]), d(dev["wd"]), d(y.t),
                                                     d(part.t), *geo, _st()), "orbit_op_mbconv_front_raw")
        else:
            part = Guarded((B, tiles, c.mid), device) if pool else None
            _lib.check(lib.orbit_op_mbconv_front(d(dev["x"]), d(dev["w1"]), d(dev["s1"]), d(dev["h1"]), d(dev["wd"]), d(dev["s2"]),
                                                 d(dev["h2"]), d(y.t), d(part.t) if pool else None, *geo, _st()),
                       "orbit_op_mbconv_front")
        torch.cuda.synchronize()
    yc = y.cpu("y")
    if part is None:
        return yc, None
    pc = part.cpu("stats_partial" if raw else "pool_partial")
    return yc, pc.view(B, tiles, 2, c.mid) if raw else pc


def run_stem_front(lib, device, t, c, B, pool=True):
    H, _, spt = same_pad(c.FH, 3, 2)
    W, _, spl = same_pad(c.FW, 3, 2)
    tiles = c.strips * c.bands
    assert lib.orbit_op_stem_dw_front_partials(H, W, STEM_MID) == tiles
    d = _lib.dptr
    dev = [t[k][:B].to(device).contiguous() if k == "x" else t[k].to(device).contiguous() for k in ("x", "ws", "s1", "h1", "wd", "s2", "h2")]
    y = Guarded((B, H, W, STEM_MID), device)
    part = Guarded((B, tiles, STEM_MID), device) if pool else None
    _lib.check(lib.orbit_op_stem_dw_front(*[d(v) for v in dev], d(y.t), d(part.t) if pool else None, B, c.FH, c.FW, spt, spl, H, W,
                                          STEM_MID, 1, 1, H, W, _st()), "orbit_op_stem_dw_front")
    torch.cuda.synchronize()
    return y.cpu("y"), part.cpu("pool_partial") if pool else None


def form(c, raw=False, bf3=False):
    return "%s_%s" % ("raw" if raw else "bf3" if bf3 else "stem" if isinstance(c, StemCase) else "front", "exact" if c.exact else "pred")


# ---- a. the SiLU form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("c", MB_CASES, ids=MB_IDS)
def test_mbconv_front(lib, device, c, family):
    Ho, _, Wo, _ = mb_out(c)
    rects = assert_plan(mb_plan(lib, c), c, Ho, Wo)
    t = mb_data(c, family)
    what = "%s/%s" % (c.name, family)
    y, part = run_mb_front(lib, device, t, c, c.B)
    _egate(form(c) + "_y", what, y, t["y64"], t["y32"])
    check_tile_sums(form(c) + "_partial", what, y, part, rects)
    if c.B > 1:  # frame 0 of the batched launch has the bits of a launch on that frame alone (another block swizzle)
        y1, p1 = run_mb_front(lib, device, t, c, 1)
        assert torch.equal(y1[0], y[0]) and torch.equal(p1[0], part[0]), what


# ---- b. the RAW (train-mode BatchNorm) form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("c", MB_CASES, ids=MB_IDS)
def test_mbconv_front_raw(lib, device, c, family):
    Ho, _, Wo, _ = mb_out(c)
    rects = assert_plan(mb_plan(lib, c), c, Ho, Wo)
    t = mb_data(c, family)
    what = "%s/%s" % (c.name, family)
    y, part = run_mb_front(lib, device, t, c, c.B, raw=True)
    _egate(form(c, raw=True) + "_y", what, y, t["raw64"], t["raw32"])
    check_tile_sums(form(c, raw=True) + "_sum", what, y, part[:, :, 0], rects)
    check_tile_squares(form(c, raw=True) + "_sumsq", what, y, part[:, :, 1], rects)
    if c.B > 1:
        y1, p1 = run_mb_front(lib, device, t, c, 1, raw=True)
        assert torch.equal(y1[0], y[0]) and torch.equal(p1[0], part[0]), what


@pytest.mark.parametrize("c", MB_CASES, ids=MB_IDS)
def test_mbconv_front_raw_feeds_the_bn_finalize(lib, device, c):
    """The kernel's [B * tiles][2][mid] partials through orbit_op_bn_stats_from_partials, as extractor_train.hip chains them,
    against the float64 statistics of the raw outputs the kernel wrote (centred taps: |mu_c| <= sigma_c, the condition of the gates)."""
    Ho, _, Wo, _ = mb_out(c)
    assert_plan(mb_plan(lib, c), c, Ho, Wo)
    t = mb_data(c, "centred")
    y, part = run_mb_front(lib, device, t, c, c.B, raw=True)
    _egate(form(c, raw=True) + "_y", c.name + "/centred", y, t["raw64"], t["raw32"])
    nblk, M = c.B * c.strips * c.bands, c.B * Ho * Wo
    pd = part.contiguous().view(nblk, 2, c.mid).to(device)
    mean, invstd = Guarded((c.mid,), device), Guarded((c.mid,), device)
    d = _lib.dptr
    _lib.check(lib.orbit_op_bn_stats_from_partials(d(pd), nblk, M, c.mid, None, None, None, EPS, 0.0, None, None, d(mean.t),
                                                   d(invstd.t), None, None, _st()), "orbit_op_bn_stats_from_partials")
    torch.cuda.synchronize()
    yd = y.double().view(M, c.mid)
    mean64 = yd.mean(0)
    sd = torch.sqrt(((yd - mean64) ** 2).mean(0) + EPS32)
    err, bound = (mean.cpu("mean").double() - mean64).abs().max().item(), 1e-6 * max(1.0, mean64.abs().max().item())
    _report(form(c, raw=True) + "_chain_mean", c.name, err, bound)
    assert err <= bound, (c.name, err, bound)
    err = ((invstd.cpu("invstd").double() - 1.0 / sd).abs() * sd).max().item()
    _report(form(c, raw=True) + "_chain_invstd", c.name, err, 1e-5)
    assert err <= 1e-5, (c.name, err)


# ---- c. the stem form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("c", STEM_CASES, ids=STEM_IDS)
def test_stem_dw_front(lib, device, c, family):
    H, W = -(-c.FH // 2), -(-c.FW // 2)
    rects = assert_plan(stem_plan(lib, c), c, H, W)
    t = stem_data(c, family)
    what = "%s/%s" % (c.name, family)
    y, part = run_stem_front(lib, device, t, c, c.B)
    _egate(form(c) + "_y", what, y, t["y64"], t["y32"])
    check_tile_sums(form(c) + "_partial", what, y, part, rects)
    if c.B > 1:
        y1, p1 = run_stem_front(lib, device, t, c, 1)
        assert torch.equal(y1[0], y[0]) and torch.equal(p1[0], part[0]), what


# ---- d. impulses at the corners and the seams --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True], ids=["silu", "raw"])
@pytest.mark.parametrize("c", MB_SEAM_CASES, ids=[c.name for c in MB_SEAM_CASES])
def test_mbconv_front_impulses(lib, device, c, raw):
    Ho, _, Wo, _ = mb_out(c)
    plan = mb_plan(lib, c)
    rects = assert_plan(plan, c, Ho, Wo)
    t = mb_data(c, "impulse", plan)
    B = t["x"].shape[0]
    assert B == 4 + 2 * (c.strips - 1) + 2 * (c.bands - 1) + 2 * (c.strips - 1) * (c.bands - 1)
    y, part = run_mb_front(lib, device, t, c, B, raw=raw)
    want64, want32 = (t["raw64"], t["raw32"]) if raw else (t["y64"], t["y32"])
    check_footprint(c.name, y, want64)
    _egate(form(c, raw=raw) + "_impulse_y", c.name, y, want64, want32)
    check_tile_sums(form(c, raw=raw) + "_impulse_sum", c.name, y, part[:, :, 0] if raw else part, rects)
    if raw:
        check_tile_squares(form(c, raw=True) + "_impulse_sumsq", c.name, y, part[:, :, 1], rects)


@pytest.mark.parametrize("c", [c for c in STEM_CASES if c.seams], ids=[c.name for c in STEM_CASES if c.seams])
def test_stem_dw_front_impulses(lib, device, c):
    H, W = -(-c.FH // 2), -(-c.FW // 2)
    plan = stem_plan(lib, c)
    rects = assert_plan(plan, c, H, W)
    t = stem_data(c, "impulse", plan)
    B = t["x"].shape[0]
    assert B == 4 + 2 * (c.strips - 1) + 2 * (c.bands - 1) + 2 * (c.strips - 1) * (c.bands - 1)
    y, part = run_stem_front(lib, device, t, c, B)
    check_footprint(c.name, y, t["y64"])
    _egate(form(c) + "_impulse_y", c.name, y, t["y64"], t["y32"])
    check_tile_sums(form(c) + "_impulse_sum", c.name, y, part, rects)


# ---- e. the BF3 expand ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("c", MB_BF3_CASES, ids=[c.name for c in MB_BF3_CASES])
def test_mbconv_front_bf3(lib, device, c, family):
    """conv_bf3 bit 2: the expand GEMM on the bf16 matrix cores with three-way split operands, exact-tiling instantiations only. Held
    to the fp32 form's gate and summation bounds: a six-product sum is within 2^-23 of the exact product (test_bf3_numerics.py),
    i.e. Cin 2^-23 max |x| max |w1| of the expanded value before BN1 - orders below the gate's floor of 2e-5. 40 -> ., 3x3 / 2 has no
    BF3 instantiation and keeps the fp32 form's bits."""
    Ho, _, Wo, _ = mb_out(c)
    rects = assert_plan(mb_plan(lib, c), c, Ho, Wo)
    t = mb_data(c, family)
    what = "%s/%s" % (c.name, family)
    y, part = run_mb_front(lib, device, t, c, c.B, bf3=2)
    _egate(form(c, bf3=True) + "_y", what, y, t["y64"], t["y32"])
    check_tile_sums(form(c, bf3=True) + "_partial", what, y, part, rects)
    y0, p0 = run_mb_front(lib, device, t, c, c.B)
    if HAS_BF3(c):
        assert not torch.equal(y0, y), what + ": the split form did not run"
    else:
        assert torch.equal(y0, y) and torch.equal(p0, part), what


# ---- f. no pooling partials ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pick", ["k3s2c16_2x2_bands_28_2", "k5s2c24_ragged"])
def test_mbconv_front_without_pool_partial(lib, device, pick):
    c = next(c for c in MB_CASES if c.name == pick)
    t = mb_data(c, "normal")
    y, _ = run_mb_front(lib, device, t, c, c.B)
    bare, none = run_mb_front(lib, device, t, c, c.B, pool=False)
    assert none is None and torch.equal(bare, y), pick + ": y depends on pool_partial"


@pytest.mark.parametrize("pick", ["stem_2_strips_3_bands", "stem_ragged_57x30"])
def test_stem_dw_front_without_pool_partial(lib, device, pick):
    c = next(c for c in STEM_CASES if c.name == pick)
    t = stem_data(c, "normal")
    y, _ = run_stem_front(lib, device, t, c, c.B)
    bare, none = run_stem_front(lib, device, t, c, c.B, pool=False)
    assert none is None and torch.equal(bare, y), pick + ": y depends on pool_partial"


# ---- g. refusals --------------------------------------------------------------------------------------------------------------------------
# what, Cin, mid, K, stride, H, W, the shape itself is refused
REFUSALS = [
    ("cin32", 32, 96, 3, 2, 12, 32, True),
    ("6x3_below_one_mfma_tile", 16, 96, 3, 2, 6, 3, True),
    ("mid_not_a_multiple_of_4", 16, 98, 3, 2, 12, 32, True),
    ("null_stats_partial", 16, 96, 3, 2, 12, 32, False),
]


def untouched(g):
    flat = g.flat.cpu()
    n = g.t.numel()
    return bool(torch.isnan(flat[:n]).all()) and torch.equal(flat[n:], torch.full((SE.GUARD,), SE.SENTINEL))


@pytest.mark.parametrize("what,Cin,mid,K,stride,H,W,shape_refused", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_entry_and_write_nothing(lib, device, what, Cin, mid, K, stride, H, W, shape_refused):
    B = 2
    Ho, _, pt = same_pad(H, K, stride)
    Wo, _, pl = same_pad(W, K, stride)
    d = _lib.dptr
    z = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
    x, w1, wd, v = z(B, H, W, Cin), z(mid, Cin, 1, 1), z(mid, 1, K, K), z(mid)
    y, part = Guarded((B, Ho, Wo, mid), device), Guarded((B * 4, 2, mid), device)
    geo = (B, H, W, Cin, mid, K, stride, pt, pl, Ho, Wo)
    out = [ctypes.c_int(-7) for _ in PLAN_KEYS]
    if shape_refused:
        assert lib.orbit_op_mbconv_front_partials(H, W, Cin, mid, K, stride) == 0
        assert lib.orbit_op_mbconv_front_plan(H, W, Cin, mid, K, stride, *[ctypes.byref(o) for o in out]) != 0
        assert "op_mbconv_front_plan" in _lib.last_error() and all(o.value == -7 for o in out)
        assert lib.orbit_op_mbconv_front(d(x), d(w1), d(v), d(v), d(wd), d(v), d(v), d(y.t), d(part.t), *geo, _st()) != 0
        assert "op_mbconv_front:" in _lib.last_error()
        assert lib.orbit_op_mbconv_front_raw(d(x), d(w1), d(v), d(v), d(wd), d(y.t), d(part.t), *geo, _st()) != 0
        assert "op_mbconv_front_raw" in _lib.last_error()
    else:
        assert lib.orbit_op_mbconv_front_partials(H, W, Cin, mid, K, stride) == 1
        assert lib.orbit_op_mbconv_front_plan(H, W, Cin, mid, K, stride, *[ctypes.byref(o) for o in out]) == 0
        assert lib.orbit_op_mbconv_front_raw(d(x), d(w1), d(v), d(v), d(wd), d(y.t), None, *geo, _st()) != 0
        assert "op_mbconv_front_raw" in _lib.last_error()
    torch.cuda.synchronize()
    assert untouched(y) and untouched(part), what
