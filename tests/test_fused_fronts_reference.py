"""CPU side of tests/test_gpu_fused_fronts.py: what that file assumes about its own cases and references, checked without a GPU.

  * orbit_op_mbconv_front_plan / orbit_op_stem_dw_front_plan (host only) report, for every case, the strips, bands and `exact` flag
    the case is named after, agree with the *_partials queries, and refuse what the launch entries refuse;
  * the tables cover all five geometries in both instantiations, both stem instantiations, and the block-count, seam and
    channel-chunk edges they are meant to;
  * the one-sign inputs keep every reference output so far from 0 that one dropped or doubled output breaks a tile's summation bound
    (y, raw y and raw y^2: smallest term > 2x the tile's bound) - shown on the reference, and by feeding the checks such a partial;
  * the centred-tap inputs satisfy |mu_c| <= sigma_c in every channel, the condition of the BatchNorm chain's Gaussian gates;
  * the impulse references are exactly 0 outside a footprint of at most K x K outputs per frame and channel."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib
import test_gpu_fused_fronts as T

U = T.U


def _rects(lib, c):
    if isinstance(c, T.StemCase):
        H, W = -(-c.FH // 2), -(-c.FW // 2)
        return T.assert_plan(T.stem_plan(lib, c), c, H, W)
    Ho, _, Wo, _ = T.mb_out(c)
    return T.assert_plan(T.mb_plan(lib, c), c, Ho, Wo)


@pytest.mark.parametrize("c", T.MB_CASES, ids=T.MB_IDS)
def test_mbconv_plan_query_names_the_tiling(lib, c):
    rects = _rects(lib, c)
    plan = T.mb_plan(lib, c)
    assert len(rects) == lib.orbit_op_mbconv_front_partials(c.H, c.W, c.Cin, c.mid, c.K, c.stride) == c.strips * c.bands
    assert plan["band_rows"] == 28 and plan["strip_w"] * plan["strips"] >= T.mb_out(c)[2] > plan["strip_w"] * (plan["strips"] - 1)


@pytest.mark.parametrize("c", T.STEM_CASES, ids=T.STEM_IDS)
def test_stem_plan_query_names_the_tiling(lib, c):
    rects = _rects(lib, c)
    assert len(rects) == lib.orbit_op_stem_dw_front_partials(-(-c.FH // 2), -(-c.FW // 2), T.STEM_MID) == c.strips * c.bands


def test_plan_queries_refuse_what_the_entries_refuse(lib):
    out = [ctypes.c_int(-7) for _ in T.PLAN_KEYS]
    refs = [ctypes.byref(o) for o in out]
    for what, Cin, mid, K, stride, H, W, shape_refused in T.REFUSALS:
        rc = lib.orbit_op_mbconv_front_plan(H, W, Cin, mid, K, stride, *refs)
        assert (rc != 0) == shape_refused, what
        assert (lib.orbit_op_mbconv_front_partials(H, W, Cin, mid, K, stride) == 0) == shape_refused, what
        if shape_refused:
            assert "op_mbconv_front_plan" in _lib.last_error() and all(o.value == -7 for o in out), what
    for o in out:
        o.value = -7
    assert lib.orbit_op_mbconv_front_plan(12, 32, 16, 96, 3, 0, *refs) != 0  # stride
    assert lib.orbit_op_mbconv_front_plan(12, 32, 16, 96, 3, 2, None, *refs[1:]) != 0
    assert lib.orbit_op_stem_dw_front_plan(8, 8, 24, *refs) != 0 and "op_stem_dw_front_plan" in _lib.last_error()
    assert lib.orbit_op_stem_dw_front_plan(8, 0, 32, *refs) != 0
    assert lib.orbit_op_stem_dw_front_plan(8, 8, 32, *refs[:4], None) != 0
    assert all(o.value == -7 for o in out)
    assert lib.orbit_op_stem_dw_front_partials(8, 8, 24) == 0


def test_cases_cover_what_they_are_meant_to():
    geoms = {(16, 3, 2), (24, 3, 1), (24, 5, 2), (40, 5, 1), (40, 3, 2)}
    assert {(c.Cin, c.K, c.stride, c.exact) for c in T.MB_CASES} == {g + (e,) for g in geoms for e in (0, 1)}
    assert {c.exact for c in T.STEM_CASES} == {0, 1}
    totals = [T.mb_total(c) for c in T.MB_CASES]
    assert any(t < 8 for t in totals) and 8 in totals and any(t > 8 and t % 8 != 0 for t in totals)
    for exact in (0, 1):  # the swizzle edges in both instantiations
        sub = [T.mb_total(c) for c in T.MB_CASES if c.exact == exact]
        assert 8 in sub and any(t % 8 != 0 for t in sub)
    assert {c.B for c in T.MB_CASES} == {1, 3} and {c.B for c in T.STEM_CASES} == {1, 3}
    for cases in (T.MB_CASES, T.STEM_CASES):
        assert any(c.strips > 1 for c in cases) and any(c.bands > 1 for c in cases)
        assert any(c.strips > 1 and c.bands > 1 and c.exact for c in cases)
        assert any(c.strips > 1 and c.bands > 1 and not c.exact for c in cases)
    chunk = {c.mid % 32 for c in T.MB_CASES}
    assert {0, 16} < chunk and all(m % 4 == 0 for m in chunk)  # a full, a half-full and an otherwise filled last chunk
    assert {c.mid % 32 for c in T.MB_CASES if c.exact} == {0, 16}
    assert len({c.mid % 32 for c in T.MB_CASES if not c.exact} - {0, 16}) >= 3
    # every geometry has an exact case with strip seams and one with band seams for the impulses and the BF3 form
    for g in geoms:
        sub = [c for c in T.MB_BF3_CASES if (c.Cin, c.K, c.stride) == g]
        assert any(c.strips > 1 for c in sub) and any(c.bands > 1 for c in sub), g
    assert any(c.seams and c.exact and c.strips > 1 and c.bands > 1 for c in T.STEM_CASES)
    # stride 2: TF-SAME pads unevenly somewhere (pad_top != pad_left)
    assert any(T.mb_out(c)[1] != T.mb_out(c)[3] for c in T.MB_CASES if c.stride == 2)


def _tile_margins(y64, rects, squares=False):
    """(smallest term, tile bound) pairs, worst ratio first: per tile, frame and channel on the float64 reference (NHWC)."""
    worst = float("inf")
    for r0, r1, c0, c1 in rects:
        blk = y64[:, r0:r1, c0:c1]
        n = (r1 - r0) * (c1 - c0)
        if squares:
            lo, bound = (blk ** 2).amin((1, 2)), 2.0 * (n + 1) * U * (blk ** 2).sum((1, 2))
        else:
            lo, bound = blk.abs().amin((1, 2)), 2.0 * n * U * blk.abs().sum((1, 2))
        worst = min(worst, (lo / bound).min().item())
    return worst


@pytest.mark.parametrize("c", T.MB_CASES + T.STEM_CASES, ids=T.MB_IDS + T.STEM_IDS)
def test_one_sign_outputs_stay_away_from_zero(lib, c):
    rects = _rects(lib, c)
    stem = isinstance(c, T.StemCase)
    t = T.stem_data(c, "one_sign") if stem else T.mb_data(c, "one_sign")
    assert _tile_margins(t["y64"], rects) > 2.0
    if not stem:
        assert _tile_margins(t["raw64"], rects) > 2.0
        assert _tile_margins(t["raw64"], rects, squares=True) > 2.0
        assert (t["raw64"] > 0).all()


PICKS = ["k3s2c16_2x2_bands_28_2", "k3s1c24_two_strips", "k5s1c40_ragged_bands", "stem_2_strips_3_bands"]


@pytest.mark.parametrize("pick", PICKS)
def test_partial_checks_catch_one_dropped_or_doubled_output(lib, pick):
    """The tile checks on stand-in kernel results: fp32 sums of the fp32-rounded reference outputs pass; the same sums with the
    SMALLEST output of one tile dropped, or added twice, do not - for the sums and for the sums of squares."""
    c = next(c for c in T.MB_CASES + T.STEM_CASES if c.name == pick)
    rects = _rects(lib, c)
    stem = isinstance(c, T.StemCase)
    t = T.stem_data(c, "one_sign") if stem else T.mb_data(c, "one_sign")
    for key, squares in [("y64", False)] + ([] if stem else [("raw64", False), ("raw64", True)]):
        y = t[key].float()
        check = T.check_tile_squares if squares else T.check_tile_sums
        term = (lambda b: b * b) if squares else (lambda b: b)  # noqa: E731
        partial = torch.stack([term(y[:, r0:r1, c0:c1]).sum((1, 2)) for r0, r1, c0, c1 in rects], 1)  # [B][tiles][C], fp32 sums
        check("standin", pick, y, partial, rects)
        k = max(range(len(rects)), key=lambda i: (rects[i][1] - rects[i][0]) * (rects[i][3] - rects[i][2]))  # the largest tile
        r0, r1, c0, c1 = rects[k]
        for sign in (-1.0, 1.0):
            bad = partial.clone()
            bad[0, k, 5] += sign * term(y[0, r0:r1, c0:c1, 5]).min()
            with pytest.raises(AssertionError):
                check("standin", pick, y, bad, rects)


@pytest.mark.parametrize("c", T.MB_CASES, ids=T.MB_IDS)
def test_centred_taps_keep_the_mean_below_the_deviation(c):
    t = T.mb_data(c, "centred")
    assert t["wd"].sum((2, 3)).abs().max().item() < 1e-6
    y = t["raw64"].reshape(-1, c.mid)
    mu, sigma = y.mean(0), y.std(0, unbiased=False)
    assert (mu.abs() <= sigma).all(), (mu.abs() / sigma).max().item()


@pytest.mark.parametrize("c", T.MB_SEAM_CASES + [c for c in T.STEM_CASES if c.seams],
                         ids=[c.name for c in T.MB_SEAM_CASES] + [c.name for c in T.STEM_CASES if c.seams])
def test_impulse_references_have_a_footprint(lib, c):
    """One non-zero input pixel per frame: each frame's reference is exactly 0 outside at most K x K outputs (stem: 4 x 4 - a frame
    pixel reaches 2 x 2 stem outputs) and non-zero inside; the positions are distinct and include both sides of every seam."""
    stem = isinstance(c, T.StemCase)
    if stem:
        plan, H, W, stride, area = T.stem_plan(lib, c), c.FH, c.FW, 2, 16
        t = T.stem_data(c, "impulse", plan)
    else:
        plan, H, W, stride, area = T.mb_plan(lib, c), c.H, c.W, c.stride, c.K * c.K
        t = T.mb_data(c, "impulse", plan)
    pos = T.seam_positions(plan, H, W, stride)
    assert len(set(pos)) == len(pos) == t["x"].shape[0] and all(0 <= r < H and 0 <= q < W for r, q in pos)
    for s in range(1, plan["strips"]):
        cs = s * plan["strip_w"] * stride
        assert {q for _, q in pos} >= {cs - 1, cs}
    for b in range(1, plan["bands"]):
        rs = b * plan["band_rows"] * stride
        assert {r for r, _ in pos} >= {rs - 1, rs}
    for key in ("y64",) if stem else ("y64", "raw64"):
        nz = (t[key] != 0).sum((1, 2))  # [B][C]
        assert (nz >= 1).all() and (nz <= area).all(), (key, nz.min().item(), nz.max().item())
    taps = t["wd"].flatten(1)
    assert all(len(set(row.tolist())) == row.numel() for row in taps) and (taps > 0).all()
