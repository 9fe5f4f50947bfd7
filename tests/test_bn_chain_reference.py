"""CPU side of tests/test_gpu_bn_chain.py: what that file assumes about its own cases and inputs, checked without a GPU.

  * orbit_op_bn_reduce_plan and orbit_op_se_pool_chunks (host only) agree with a Python restatement of the layout rules of
    csrc/train_ops.hip for every case, and with the block, chunk and compaction-group counts the case names claim;
  * the case tables cover what they say: idle threads, one and two column groups, a ragged last block, chunk and compaction
    group, at least three grid trips of the streaming kernels;
  * every exact-family input keeps every partial sum below 2^24, an fp32 sum of it in three shuffled orders has the bits of the
    float64 sum, and one dropped or doubled row, a chunk boundary moved by one or a skipped last compaction group changes a sum
    the GPU file checks;
  * the Gaussian inputs satisfy |mu_c| <= sigma_c and the ReLU inputs keep their margin."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib
import test_gpu_bn_chain as T


def cdiv(a, b):
    return -(-a // b)


# ---- the layout rules, restated --------------------------------------------------------------------------------------------------------
def col_layout(C):
    Q = C // 4
    G = min(Q, 256)
    return dict(G=G, R=256 // G, ygroups=cdiv(Q, G))


def reduce_plan(M, C):
    L = col_layout(C)
    rows = max(cdiv(M, 1024), 4 * L["R"])  # enough blocks to fill the chip, at least 4 rows per row lane
    nblk = cdiv(M, rows)
    return dict(L, nblk=nblk, rpb=cdiv(M, nblk))


def pool_chunks(B, HW, C):
    L = col_layout(C)
    want = max(1, min(cdiv(2048, B * L["ygroups"]), cdiv(HW, 4 * L["R"])))
    chunks = cdiv(HW, cdiv(HW, want))
    return chunks, cdiv(HW, chunks)


def compaction(nblk):
    """(group size, compacted blocks, blocks of the last group) above 2048 blocks, else None."""
    if nblk <= 2048:
        return None
    gs = cdiv(nblk, 1024)
    nout = cdiv(nblk, gs)
    return gs, nout, nblk - (nout - 1) * gs


ALL_MC = [(c[1], c[2]) for c in T.STATS_CASES] + T.FORM_SHAPES + [(v[0], v[1]) for v in T.TRIP_CASES.values()]


@pytest.mark.parametrize("M,C", ALL_MC)
def test_reduce_plan_query_follows_the_rules(lib, M, C):
    assert T.reduce_plan(lib, M, C) == reduce_plan(M, C)


@pytest.mark.parametrize("name,M,C,claim", T.STATS_CASES, ids=T.STATS_IDS)
def test_statistics_cases_are_what_their_names_claim(lib, name, M, C, claim):
    T.assert_reduce_plan(lib, M, C, claim)
    p = reduce_plan(M, C)
    rows = T.block_rows(M, p["rpb"])
    assert dict(p, idle=256 - p["G"] * p["R"], last=rows[-1]) == claim
    assert len(rows) == p["nblk"] and all(r > 0 for r in rows)


@pytest.mark.parametrize("name,B,HW,C,rows", T.POOL_CASES, ids=T.POOL_IDS)
def test_pool_chunk_query_follows_the_rules(lib, name, B, HW, C, rows):
    chunks, rpc = T.pool_chunks(lib, B, HW, C)
    assert (chunks, rpc) == pool_chunks(B, HW, C)
    assert T.block_rows(HW, rpc) == rows and chunks == len(rows) and sum(rows) == HW


def test_compaction_groups_are_what_the_table_claims():
    for nblk in T.PARTIAL_NBLK:
        assert compaction(nblk) == T.COMPACTION.get(nblk), nblk
    assert {1, 2048, 2050, 4099} <= set(T.PARTIAL_NBLK)


def test_queries_refuse_bad_arguments(lib):
    v = ctypes.c_int(0)
    r = ctypes.byref(v)
    assert lib.orbit_op_bn_reduce_plan(8, 8, r, r, r, r, None) != 0
    assert lib.orbit_op_bn_reduce_plan(0, 8, r, r, r, r, r) != 0
    assert lib.orbit_op_bn_reduce_plan(8, 6, r, r, r, r, r) != 0
    assert "op_bn_reduce_plan" in _lib.last_error()
    assert lib.orbit_op_se_pool_chunks(1, 8, 8, None, r) != 0
    assert lib.orbit_op_se_pool_chunks(0, 8, 8, r, r) != 0
    assert lib.orbit_op_se_pool_chunks(1, 0, 8, r, r) != 0
    assert lib.orbit_op_se_pool_chunks(1, 8, 10, r, r) != 0
    assert "op_se_pool_chunks" in _lib.last_error()


def test_cases_cover_what_they_are_meant_to():
    claims = [c[3] for c in T.STATS_CASES]
    assert any(c["idle"] > 0 for c in claims) and any(c["idle"] == 0 for c in claims)
    assert {c["ygroups"] for c in claims} == {1, 2}
    assert any(c["nblk"] > 1 and c["last"] < c["rpb"] for c in claims) and any(c["last"] == 1 and c["nblk"] > 1 for c in claims)
    assert any(c["nblk"] == 1 for c in claims) and any(c[1] == 1 for c in T.STATS_CASES)  # one block; M == 1
    assert any(c["R"] == 1 for c in claims) and any(c["R"] == 128 for c in claims)
    # two column groups, the second with one live quad
    assert all(C // 4 - 256 == 1 for _, _, C, c in T.STATS_CASES if c["ygroups"] == 2)
    pools = [(col_layout(c[3]), c[4]) for c in T.POOL_CASES]
    assert {L["ygroups"] for L, _ in pools} == {1, 2}
    assert any(256 - L["G"] * L["R"] > 0 for L, _ in pools)
    assert any(len(rows) > 1 and rows[-1] < rows[0] for _, rows in pools) and any(len(rows) == 1 for _, rows in pools)
    assert any(rows[-1] == 1 and len(rows) > 1 for _, rows in pools)
    assert any(c[2] == 1 for c in T.POOL_CASES)  # one pixel per frame
    assert any(rows[0] < 4 * L["R"] for L, rows in pools)  # row lanes without a row
    # ragged and full last compaction group, and the threshold itself
    groups = [T.COMPACTION[n] for n in T.PARTIAL_NBLK if n in T.COMPACTION]
    assert any(last == gs for gs, _, last in groups) and any(last == 1 for _, _, last in groups)
    assert any(1 < last < gs for gs, _, last in groups) and 2048 in T.PARTIAL_NBLK and 2049 in T.PARTIAL_NBLK
    # the streaming kernels: more than two full trips, the incremental channel walk with a stride that is no multiple of C / 4
    for M, C, stride_mod in T.TRIP_CASES.values():
        total4 = M * (C // 4)
        assert 2 * T.GRID_STRIDE < total4 <= 3 * T.GRID_STRIDE and total4 % T.GRID_STRIDE != 0
        assert T.GRID_STRIDE % (C // 4) == stride_mod != 0
    assert all(M * (C // 4) <= T.GRID_STRIDE for M, C in [(c[1], c[2]) for c in T.STATS_CASES] + T.FORM_SHAPES)
    assert {T.GRAM_P[0], 256, 257} <= set(T.GRAM_P) and max(T.GRAM_P) > 3 * 256 * 32  # several Gram blocks


# ---- the exact family -------------------------------------------------------------------------------------------------------------------
def assert_exact_sums(terms):
    """terms [n][C] float64: every partial sum of every order stays below 2^24 (the sum of magnitudes does), and fp32 sums in three
    shuffled orders - serial, so that every intermediate is an fp32 number - have the bits of the float64 sum."""
    assert terms.abs().sum(0).max().item() < 2 ** 24
    assert torch.equal(terms.float().double(), terms)
    want = terms.sum(0)
    g = torch.Generator().manual_seed(terms.shape[0])
    for _ in range(3):
        t32 = terms.float()[torch.randperm(terms.shape[0], generator=g)]
        # cumsum in fp32 is a serial sum: compare its last row, and a two-halves pairing of it
        assert torch.equal(t32.cumsum(0)[-1].double(), want)
        h = t32.shape[0] // 2
        assert torch.equal((t32[:h].sum(0) + t32[h:].sum(0)).double(), want)


@pytest.mark.parametrize("name,M,C,claim", T.STATS_CASES, ids=T.STATS_IDS)
def test_exact_statistics_inputs(name, M, C, claim):
    y = T.y_input("exact", M, C, 1, M, C).double()
    assert ((y.abs() >= 1) & (y.abs() <= 3) & (y == y.round())).all()
    for terms in (y, y * y):
        assert_exact_sums(terms)
        S = terms.sum(0)
        # one row dropped or counted twice: every such sum differs from S in fp32
        assert ((S - terms).float() != S.float()).all() and ((S + terms).float() != S.float()).all()
    t = T.exact_backward_inputs(M, C)
    g, xh = t["dout"].double(), (t["y"].double() - t["mean"].double()) * t["invstd"].double()
    assert (t["mean"] == t["mean"].round()).all() and (t["invstd"] == 0.5).all() and (g != 0).all()
    assert_exact_sums(g)
    assert_exact_sums(g * xh)
    S = g.sum(0)
    assert ((S - g).float() != S.float()).all() and ((S + g).float() != S.float()).all()  # dbeta sees every row


@pytest.mark.parametrize("nblk", T.PARTIAL_NBLK)
def test_exact_partials_and_their_compaction_groups(nblk):
    """The producer stand-in's partials are exact, tile the rows, and a skipped last compaction group (or last block) changes both
    sums in every channel."""
    C = 8
    y, partial = T.stats_partials("exact", C, nblk)
    assert y.shape[0] == T.partial_rows(nblk) and partial.shape == (nblk, 2, C)
    assert torch.equal(partial[:, 0].double().sum(0), y.double().sum(0))
    assert torch.equal(partial[:, 1].double().sum(0), (y.double() ** 2).sum(0))
    assert_exact_sums(partial[:, 0].double())
    assert_exact_sums(partial[:, 1].double())
    assert (partial[:, 1] > 0).all()  # every block, so every group, carries weight in the sum of squares
    if nblk in T.COMPACTION:
        gs, nout, last = T.COMPACTION[nblk]
        full = partial.double().sum(0)
        skipped = partial[:(nout - 1) * gs].double().sum(0)
        assert partial[(nout - 1) * gs:].shape[0] == last and (skipped[1].float() != full[1].float()).all()
    t = T.reduced_inputs(C, nblk)
    assert_exact_sums(t["partial"][:, 0].double())
    assert_exact_sums(t["partial"][:, 1].double())
    ref = T.bwd_ref(t["dout"], t["y"], None, t["mean"], t["invstd"], t["gamma"], None, None, 1, T.NONE, False, None, torch.float64)
    assert torch.equal(t["partial"][:, 1].double().sum(0), ref[2]) and torch.equal(t["partial"][:, 0].double().sum(0), ref[3])


@pytest.mark.parametrize("Cin", [16, 24])
def test_exact_gram_inputs(Cin):
    x, w = T.gram_inputs(Cin, max(T.GRAM_P))
    assert (x == x.round()).all() and x.abs().max() <= 2 and torch.equal(w * 8, (w * 8).round())
    xd = x.double()
    assert 2 * xd.abs().sum(0).max().item() < 2 ** 24  # |x_i x_j| <= 2 |x_i|: every Gram partial sum is an fp32 number
    assert_exact_sums(xd)
    assert_exact_sums(xd[:, :1] * xd)
    y = xd @ w.double().t()
    assert torch.equal(y * 8, (y * 8).round())


@pytest.mark.parametrize("act", [T.NONE, T.RELU], ids=["none", "relu"])
@pytest.mark.parametrize("name,B,HW,C,rows", T.POOL_CASES, ids=T.POOL_IDS)
def test_exact_pool_inputs(name, B, HW, C, rows, act):
    y, scale, shift = T.pool_inputs("exact", B, HW, C, act)
    assert (scale == 1).all() and (shift == 0).all()
    out = T.apply_ref(y, scale, shift, None, act, False, torch.float64)
    for b in range(B):
        assert_exact_sums(out[b])
    # a chunk boundary moved by one row changes the sums of both chunks in some channel
    r0 = 0
    for nr in rows[:-1]:
        r0 += nr
        assert (out[:, r0 - 1] != 0).any(1).all() and (out[:, r0] != 0).any(1).all()
    # ... and a dropped or doubled row its chunk's sum
    assert (out != 0).any(2).all()


# ---- the Gaussian family ----------------------------------------------------------------------------------------------------------------
def test_gaussian_channels_are_no_more_offset_than_wide():
    for C in sorted({c[2] for c in T.STATS_CASES} | {c[3] for c in T.POOL_CASES} | {s[1] for s in T.FORM_SHAPES} | {36, 100}):
        mu, sigma = T.gauss_params(C, T._gen(C))
        assert (mu.abs() <= sigma).all() and (sigma >= 0.5).all()
    # ... and the samples follow: batch statistics of the larger cases
    for M, C, seed in [(2049, 1028, (1, 2049, 1028)), (1025, 8, (1, 1025, 8)), (470_000, 36, (15,))]:
        y = T.y_input("gauss", M, C, *seed).double()
        assert (y.mean(0).abs() <= 1.25 * y.std(0)).all()


@pytest.mark.parametrize("M,C", T.FORM_SHAPES)
def test_relu_inputs_keep_their_margin(M, C):
    for post, pre_res in ((True, False), (False, True), (False, False)):
        t = T.form_inputs(M, C, T.RELU, post, pre_res)
        z = t["y"].double() * t["scale"].double() + t["shift"].double()
        if t["res"] is not None and not post:
            z = z + t["res"].double()
        assert z.abs().min().item() >= T.RELU_MARGIN and (t["scale"] > 0).all()
    for name, B, HW, C2, rows in T.POOL_CASES:
        y, scale, shift = T.pool_inputs("gauss", B, HW, C2, T.RELU)
        assert (y.double() * scale.double() + shift.double()).abs().min().item() >= T.RELU_MARGIN
