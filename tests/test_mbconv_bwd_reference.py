"""CPU side of tests/test_gpu_mbconv_bwd.py: what that file assumes about its own cases, inputs and checks, shown without a GPU.

  * orbit_op_dwconv2d_backward_plan (host only) names, for every case and mode, the kernel family, what is carried and the
    geometry the case tables claim, under the case's options, and leaves the options as they were;
  * the case lists cover all four padding parities x both K at stride 2, a filter-gradient block that walks two tiles with a
    ragged last group, RL = 1, rpc = 1, ragged column groups, several column groups with a partly filled last one, and the three
    refusals;
  * on the one_sign inputs the smallest term of every checked sum exceeds that sum's bound - except for the sums listed in
    NO_MARGIN, which are shown to be exactly the ones whose bound (it grows with n^2) has outgrown a single term; each sum check
    raises on a stand-in result with one term dropped or added twice;
  * the ReLU inputs keep |z| >= 1e-3."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib
import test_gpu_mbconv_bwd as T

U = T.U
OPTS = (b"dw_window", b"dw_lds", b"dw_pipe")


# ---- the plan query ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,C,H,W,K,par,blocks,bn_rows,wg_rows", T.S2_CASES, ids=T.S2_IDS)
def test_plan_names_the_stride2_kernel_and_its_rows(lib, name, B, C, H, W, K, par, blocks, bn_rows, wg_rows):
    Ho, Wo, pt, pl, _, _ = T.layer(H, W, K, 2)
    assert (pt & 1, pl & 1) == par
    for mode, want in ((T.DGRAD, (0, 0, blocks, 0, 0)), (T.DGRAD_BN, (1, 0, bn_rows, bn_rows, 0)),
                       (T.DGRAD_BN_WG, (1, 1, wg_rows, wg_rows, wg_rows))):
        p = T.bwd_plan(lib, B, C, H, W, K, 2, mode)
        assert p.family == T.FAM_S2 and (p.epilogue, p.wgrad, p.blocks, p.bn_rows, p.wgrad_rows) == want, (name, mode)
    # the rows against the layout the case comments name: G quads x R row lanes, a row block per R 2x2 blocks, caps 16384 / 2048
    R = 256 // min(C // 4, 64)
    blocks2 = B * ((H + 1) // 2) * ((W + 1) // 2)
    assert blocks == min(-(-blocks2 // R), 16384) and bn_rows == min(blocks, 2048) and wg_rows <= bn_rows
    assert (blocks2 > wg_rows * R) and (name != "capped" or (bn_rows * R < blocks2 <= blocks * R))  # fused: several strides per lane


@pytest.mark.parametrize("name,B,C,H,W,K,opts,form,rows,bn,wg", T.S1_CASES, ids=T.S1_IDS)
def test_plan_names_the_stride1_form_and_what_it_carries(lib, name, B, C, H, W, K, opts, form, rows, bn, wg):
    before = [lib.orbit_get_option(k) for k in OPTS]
    with T.options(lib, dw_window=opts[0], dw_lds=opts[1], dw_pipe=opts[2]):
        for mode in (T.DGRAD, T.DGRAD_BN, T.DGRAD_BN_WG):
            p = T.bwd_plan(lib, B, C, H, W, K, 1, mode)
            assert p.family == form and T.S.chunk_rows(H, p.rpc) == rows and p.chunks == len(rows) and sum(rows) == H
            carried = (int(mode != T.DGRAD and bn), int(mode == T.DGRAD_BN_WG and wg))
            assert (p.epilogue, p.wgrad, p.bn_rows, p.wgrad_rows) == carried + (carried[0] * B * len(rows), carried[1] * B * len(rows))
        # the data gradient is a forward launch over dy with H output rows: the forward plan query names the same form
        assert T.S.dw_plan(lib, B, C, K, 1, H, W)[0] == form
    assert [lib.orbit_get_option(k) for k in OPTS] == before


@pytest.mark.parametrize("name,B,C,H,W,K,stride,geom", T.WG_XF_CASES, ids=T.XF_IDS)
def test_plan_names_the_lds_filter_gradient_geometry(lib, name, B, C, H, W, K, stride, geom):
    p = T.bwd_plan(lib, B, C, H, W, K, stride, T.WGRAD_XF)
    assert p.family == T.FAM_WG_LDS
    if geom is None:
        assert (p.wgrad, p.wgrad_rows, p.groups) == (0, 0, 0)
        return
    assert p.wgrad == 1 and (p.cs4, p.rpc, p.chunks, p.tpb, p.groups) == geom and p.wgrad_rows == p.groups
    Ho = T.layer(H, W, K, stride)[0]
    assert p.chunks == -(-Ho // p.rpc) and p.groups == -(-(B * p.chunks) // p.tpb)


def test_plan_names_the_global_load_filter_gradient(lib):
    for B, C, H, W, K, stride in T.WG_GLOBAL_CASES:
        Ho, Wo = T.layer(H, W, K, stride)[:2]
        p = T.bwd_plan(lib, B, C, H, W, K, stride, T.WGRAD)
        assert p.family == T.FAM_WG_GLOBAL and p.wgrad == 1 and p.wgrad_rows == p.chunks == -(-(B * Ho) // p.rpc)
        assert Wo % (2 if (K, stride) == (5, 2) else 4) != 0
    assert {(c[4], c[5]) for c in T.WG_GLOBAL_CASES} == {(3, 1), (5, 1), (3, 2), (5, 2)}
    assert any(c[1] // 4 > 64 and (c[1] // 4) % 64 for c in T.WG_GLOBAL_CASES)  # several column groups, the last partly filled


def test_plan_query_refuses_bad_arguments(lib):
    p = _lib.DwconvBackwardPlan()
    r = ctypes.byref(p)
    ok = (2, 16, 14, 32, 3, 2, 0, 0, 8, 7, T.DGRAD)
    assert lib.orbit_op_dwconv2d_backward_plan(*ok, r) == 0
    assert lib.orbit_op_dwconv2d_backward_plan(*ok, None) != 0
    for i, v in ((3, 30), (4, 4), (5, 3), (10, 5), (10, -1), (0, 0)):  # C % 4, K, stride, mode, mode, B
        bad = list(ok)
        bad[i] = v
        assert lib.orbit_op_dwconv2d_backward_plan(*bad, r) == T.ERR_ARG, (i, v)
        assert "op_dwconv2d_backward_plan" in _lib.last_error()


def test_cases_cover_what_they_are_meant_to(lib):
    assert {(c[5], c[6]) for c in T.S2_CASES if c[0] != "capped"} == {(K, (a, b)) for K in (3, 5) for a in (0, 1) for b in (0, 1)}
    assert all(c[3] != c[4] for c in T.S2_CASES + T.S1_CASES)  # no square map
    assert any(c[4] % 2 for c in T.S2_CASES) and any(c[3] % 2 for c in T.S2_CASES)  # odd W / odd H: 2x2 blocks over the edge
    assert any(c[2] // 4 > 64 and (c[2] // 4) % 64 for c in T.S2_CASES)  # several column groups, the last partly filled
    s1 = {c[0]: c for c in T.S1_CASES}
    assert {c[7] for c in T.S1_CASES} == {T.LDS, T.WINDOW, T.STREAM, T.PIPE}
    assert any(c[4] % 4 for c in T.S1_CASES if c[10]) and any(c[8][-1] == 1 for c in T.S1_CASES if c[10])  # ragged columns / one-row chunk
    assert any(256 % max(d for d in range(1, min(c[2] // 4, 64) + 1) if (c[2] // 4) % d == 0) for c in T.S1_CASES if c[10])  # 256 % cb4
    # the three refusals of the data gradient and the one of the filter gradient
    assert not s1["unfit_k5_c40"][9] and not s1["pipe_forced"][9] and s1["unfit_k3_c40"][9] and not s1["unfit_k3_c40"][10]
    assert sum(1 for c in T.WG_XF_CASES if c[7] is None) == 1
    xf = [c for c in T.WG_XF_CASES if c[7]]
    assert any(c[7][3] > 1 and (c[1] * c[7][2]) % c[7][3] for c in xf)  # tpb > 1, ragged last group
    assert any(c[7][1] == 1 for c in xf)  # rpc = 1
    G = lambda c: -(-T.layer(c[3], c[4], c[5], c[6])[1] // 4)  # noqa: E731
    assert any((256 // c[7][0]) // G(c) == 1 and (256 // c[7][0]) % G(c) for c in xf)  # RL = 1 with idle pixel lanes
    assert any(T.layer(c[3], c[4], c[5], c[6])[1] % 4 for c in xf) and {c[6] for c in xf} == {1, 2} and {c[5] for c in xf} == {3, 5}
    name, B, HW, C, R = T.SE_CAPPED
    assert HW * (C // 4) > 64 * 256 and (64 * 256) % (C // 4) != 0 and -(-16384 // B) == 64  # capped grid, wrapping q walk
    assert any(c[2] == 197 for c in T.SE_CASES)


# ---- the one_sign margin ----------------------------------------------------------------------------------------------------------------
def sum_margin(terms, cdim):
    """Per channel: the smallest term against the bound 2 (n + 2) u A of the channel's sum. True where the term is larger."""
    dims = [d for d in range(terms.dim()) if d != cdim]
    n = terms.numel() // terms.shape[cdim]
    return terms.abs().amin(dims) > 2.0 * (n + 2) * U * terms.abs().sum(dims)


def dw_sum_margins(B, C, H, W, K, stride, act, want_dw):
    """{sum name: the margin holds in every channel} for a depthwise case on the one_sign inputs."""
    t, r64, r32, A, n = T.dw_case("one_sign", B, C, H, W, K, stride, act)
    assert (r64["g"] > 0).all() and (r64["a"] > 0).all() and (t["dy"] > 0).all() and (t["w"] > 0).all()
    xhat = (t["y"].double() - T.nchw_c(t["mean"].double())) * T.nchw_c(t["invstd"].double())
    assert (xhat > 0).all()
    out = {"g/silu" if act == T.SILU else "g/none": bool(sum_margin(r64["g"], 1).all() and sum_margin(r64["g"] * xhat, 1).all())}
    if want_dw:
        e32 = (r32["dw"].double() - r64["dw"]).abs().max().item()
        lo = t["dy"].double().amin((0, 2, 3)) * r64["a"].amin((0, 2, 3))  # below every term dy * x of the channel
        out["dw"] = bool((lo.view(-1, 1, 1, 1) > 2.0 * n * U * A + 4.0 * e32).all())
    return out


def expect_margins(name, got):
    """Every margin holds unless NO_MARGIN names the sum - and there it does not (the list is exact)."""
    for k, holds in got.items():
        assert holds != (k in T.NO_MARGIN.get(name, ())), (name, k, holds)


@pytest.mark.parametrize("name,B,C,H,W,K,par,blocks,bn_rows,wg_rows", T.S2_CASES, ids=T.S2_IDS)
def test_one_sign_terms_exceed_the_sum_bounds_stride2(name, B, C, H, W, K, par, blocks, bn_rows, wg_rows):
    if name == "capped":  # 2 n (n + 2) u >= 1: the bound exceeds the MEAN term, whatever the inputs
        n = B * H * W
        assert 2.0 * n * (n + 2) * U >= 1.0 and T.NO_MARGIN[name] == T.ALL_SUMS
        return
    expect_margins(name, dw_sum_margins(B, C, H, W, K, 2, T.SILU, True))
    expect_margins(name, dw_sum_margins(B, C, H, W, K, 2, T.NONE, False))


@pytest.mark.parametrize("name,B,C,H,W,K,opts,form,rows,bn,wg", T.S1_CASES, ids=T.S1_IDS)
def test_one_sign_terms_exceed_the_sum_bounds_stride1(name, B, C, H, W, K, opts, form, rows, bn, wg):
    if not bn:
        return
    got = dw_sum_margins(B, C, H, W, K, 1, T.SILU, wg)
    expect_margins(name, got)
    expect_margins(name, dw_sum_margins(B, C, H, W, K, 1, T.NONE, False))


def test_one_sign_terms_exceed_the_filter_gradient_bounds():
    for B, C, H, W, K, stride in T.WG_GLOBAL_CASES:
        expect_margins("global", {"dw": dw_sum_margins(B, C, H, W, K, stride, T.NONE, True)["dw"]})
    for name, B, C, H, W, K, stride, geom in T.WG_XF_CASES:
        if geom:
            expect_margins(name, {"dw": dw_sum_margins(B, C, H, W, K, stride, T.SILU, True)["dw"]})


def test_one_sign_terms_exceed_the_sum_bounds_squeeze_excite():
    for name, B, HW, C, R in T.SE_CASES:
        t, r64, _ = T.se_case("one_sign", B, HW, C, R, T.SILU, 1)
        xhat = (t["y"].double() - T.nlc(t["mean"].double())) * T.nlc(t["invstd"].double())
        assert (r64["g"] > 0).all() and (xhat > 0).all()
        expect_margins(name, {"g/silu": bool(sum_margin(r64["g"], 2).all() and sum_margin(r64["g"] * xhat, 2).all())})
    name, B, HW, C, R = T.SE_CAPPED
    n = B * HW
    assert 2.0 * n * (n + 2) * U >= 1.0 and T.NO_MARGIN[name] == ("g/silu",)


# ---- the sum checks on stand-in results ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pick", ["k3_p01", "k5_p10", "k5_p01"])
def test_channel_sum_check_catches_one_dropped_or_doubled_term(pick):
    """fp32 sums of the fp32 reference g pass; with the channel's SMALLEST term dropped, or added twice, they do not."""
    name, B, C, H, W, K = next(c for c in T.S2_CASES if c[0] == pick)[:6]
    t, r64, r32, _, _ = T.dw_case("one_sign", B, C, H, W, K, 2, T.SILU)
    g = r32["g"]
    xhat = (t["y"] - T.nchw_c(t["mean"])) * T.nchw_c(t["invstd"])
    sums = torch.stack([g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))])
    T.check_channel_sums("standin", pick, sums, g, t["y"], t["mean"], t["invstd"], 1)
    c = C // 2
    for k, terms in enumerate((g, g * xhat)):
        for sign in (-1.0, 1.0):
            bad = sums.clone()
            bad[k, c] += sign * terms[:, c].min()
            with pytest.raises(AssertionError):
                T.check_channel_sums("standin", pick, bad, g, t["y"], t["mean"], t["invstd"], 1)


@pytest.mark.parametrize("pick", ["xf_c1152_13x9", "xf_16x70_s2"])
def test_filter_gradient_check_catches_one_dropped_or_doubled_term(pick):
    name, B, C, H, W, K, stride, _ = next(c for c in T.WG_XF_CASES if c[0] == pick)
    t, r64, r32, A, n = T.dw_case("one_sign", B, C, H, W, K, stride, T.SILU)
    T.check_wgrad("standin", pick, r32["dw"], r64["dw"], r32["dw"], A, n)
    # the term of tap (0, 0) at the first output pixel that reaches inside the map
    Ho, Wo, pt, pl, _, _ = T.layer(H, W, K, stride)
    ho, wo = -(-pt // stride), -(-pl // stride)
    c = C // 2
    term = t["dy"][0, c, ho, wo] * r32["a"][0, c, ho * stride - pt, wo * stride - pl]
    for sign in (-1.0, 1.0):
        bad = r32["dw"].clone()
        bad[c, 0, 0, 0] += sign * term
        with pytest.raises(AssertionError):
            T.check_wgrad("standin", pick, bad, r64["dw"], r32["dw"], A, n)


def test_squeeze_excite_sum_check_catches_one_dropped_or_doubled_term():
    name, B, HW, C, R = T.SE_CASES[2]
    t, r64, r32 = T.se_case("one_sign", B, HW, C, R, T.SILU, 1)
    g = r32["g"]
    xhat = (t["y"] - T.nlc(t["mean"])) * T.nlc(t["invstd"])
    sums = torch.stack([g.sum((0, 1)), (g * xhat).sum((0, 1))])
    T.check_channel_sums("standin", name, sums, g, t["y"], t["mean"], t["invstd"], 2)
    for k, terms in enumerate((g, g * xhat)):
        for sign in (-1.0, 1.0):
            bad = sums.clone()
            bad[k, 7] += sign * terms[:, :, 7].min()
            with pytest.raises(AssertionError):
                T.check_channel_sums("standin", name, bad, g, t["y"], t["mean"], t["invstd"], 2)


# ---- the ReLU inputs ------------------------------------------------------------------------------------------------------------------------
def test_relu_inputs_stay_off_zero():
    for B, C, H, W, K, stride in (T.S2_CASES[0][1:6] + (2,), T.WG_XF_CASES[0][1:7]):
        _, r64, r32, _, _ = T.dw_case("normal", B, C, H, W, K, stride, T.RELU)
        assert r64["z"].abs().min() >= 1e-3 and r32["z"].abs().min() >= 1e-3
        assert ((r64["z"] > 0) == (r32["z"] > 0)).all() and 0.3 < (r64["z"] > 0).double().mean() < 0.7
