"""The dense filter-gradient kernels of csrc/conv_wgrad.hip, instantiation by instantiation, against exact integers and float64.

One table (CASES) names, for every case, the geometry and the LITERAL plan the launch must take, as orbit_op_conv2d_wgrad_plan
(host only) reports it: the form (tiled NHWC, tiled NCHW, thin), for the thin register form TF, TT, fat_is_co, groups,
tiles_per_group, blocks, rows_per_wave - conv_wgrad_thin_kernel<TF, TT, FAT_IS_CO, GATE> - and for the 64x64-tile kernel co_tiles,
n_tiles, splits, steps_per_split. Every case asserts the plan against the table, runs under the profiler and must produce
exactly one conv_wgrad_thin / conv_wgrad<nhwc> / conv_wgrad<nchw> row, runs again and must repeat its bits. dw is NaN-filled and
followed by a sentinel tail (Guarded of tests/test_gpu_se_path.py). conv_bf3 is 0 for the whole file.

Two input families per case:
  exact   x and dy integers in [-3, 3], gates from {0, 0.5, 1, 2}: every product and every partial sum in any order is a multiple
          of 0.5 of magnitude <= 18 M < 2^23 (M <= 2^18 + 2^13), so fp32 arithmetic is exact in any order and the result must
          equal the integer reference bit for bit (in int64, in units of 0.5; for the 2^18-row cases the sums are evaluated by
          float64 BLAS, which is exact on integers below 2^53, and converted - tests/test_conv_wgrad_reference.py holds the
          claim and the equality of the two evaluations). No tolerance: a dropped, doubled or misplaced row, a wrong gate frame
          or a transposed output cannot hide.
  normal  zero-mean Gaussians, gates uniform in (0, 1) with exact zeros in an eighth of the (frame, channel) entries, against
          float64 under gate() of tests/test_gpu_vit_ops.py: max |got - ref64| <= max(4 e32, 8 u max |ref64|). e32 is the error
          against float64 of blocked_chain(): the same sums in float32 on the CPU in the plan's order - rows in runs of
          rows_per_wave (thin) or steps_per_split * 32 (tiled), one product after the other (the 4 / 2 products of an MFMA as
          sequential adds), the 4 waves of a block in wave order, then the partial tiles as the reduce kernel adds them: each
          of 16 lanes every 16th one, the lanes in order. Evaluated on every output where there are at most 32 768 of them
          (all thin cases), else on a random sample of at least 4096.

Thin form (pointwise, unpadded, M >= 2^18 rows, the thinner side <= 2 tiles of 16 channels): maps of 2048 x 8x16 (M = 2^18:
rows_per_wave 64, 1024 blocks, no tail), 1 x 5x52429 (M = 2^18 + 1: rows_per_wave 96, 683 blocks, the last one 96 + 96 + 65 rows
and an idle wave, one lane group of the last step live) and 3237 x 9x9 (M = 262 197, H W = 81: a frame boundary inside a 4-row
step about every 20 rows, the last wave 21 rows). Every case runs ungated and gated on the same operands.

Batched reduce (orbit_op_conv2d_wgrad_batched, n = 1, 3, 48 layers of all three forms): every dw bit-equal to the same layer
through orbit_op_conv2d_wgrad / _gated, on the normal family; n = 49 refused with the launcher's message, nothing written.

Data gradient's own kernels (conv_pack_dgrad_kernel, upsample_zero_kernel) through orbit_op_conv2d_dgrad: exact family only.

What the launch rules make of the table (found while writing it; the plan assertion is the check):
  * conv_wgrad_thin_kernel<2, 2, false, *> cannot be reached: fat = x needs tco < tci, TT = 2 means tco = 2, so tci >= 3 and the
    group holds >= 3 tiles, which is TF = 4. With equal tile counts (28 -> 24, 2 and 2) the fat side is dy. 30 of the 32
    instantiations are reachable and every one of them is in the table, gated and ungated;
  * M = 2^18 - 1 (73 maps of 27x133) plans the tiled form for 16 -> 96, and 40 -> 240 (3 thin tiles) plans it at any M;
  * in NHWC Cout % 4 == 0 and Cin % 4 == 0 make Cout * NC a multiple of 16, so only an NCHW job (4 x 27, 20 x 27) can leave the
    last 16-output block of a reduce job partial; 20 x 12 = 240 is whole blocks;
  * total_steps 7 and 8 both plan one split (max_splits = total_steps / 8), 25 steps plan 9 + 9 + 7, 75 steps 8 x 9 + 3.
Every case got the plan the table gives it, every exact case came back bit for bit, and the batched reduce repeated the per-layer
bits at n = 1, 3 and 48: nothing had to be fixed or refused.

Largest err / e32 per form on the MI355X (each normal case prints "[wgrad-forms] name: err, e32, err/e32"; run with -s). 4 e32 was
the bound of every case, the floor 8 u max |ref64| of none (it is 0.4 - 0.65 of 4 e32 on the thin cases, 0.15 - 0.75 on the tiled):
  thin         err / e32 1.38  (thin_32to16_5x52429/plain)     gated: 1.35 (thin_136to20_8x16)
  tiled nhwc   err / e32 1.49  (gated_672to112_14x14/gated)    ungated: 1.14 (steps7_cout4)
  tiled nchw   err / e32 1.26  (stem_nc27_cout4/plain)
What the file notices, tried once with a deliberately wrong build: the gate frame taken from a step's first row instead of the
lane's own row fails the six gated exact cases on the 9x9 map and none on the 8x16 map; a batched reduce that walks first_block[]
one block late fails n = 3 and n = 48.
"""
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from test_gpu_se_path import GUARD, SENTINEL, Guarded, options  # noqa: E402
from test_gpu_vit_ops import U, _prof_rows, gate  # noqa: E402

NHWC, NCHW, THIN = 0, 1, 2                      # WgradForm of csrc/common.h, as orbit_op_conv2d_wgrad_plan reports it
ROW = {NHWC: "conv_wgrad<nhwc>", NCHW: "conv_wgrad<nchw>", THIN: "conv_wgrad_thin"}
FORM_NAME = {NHWC: "tiled nhwc", NCHW: "tiled nchw", THIN: "thin"}
WGRAD_REDUCE_JOBS = 48
NO_THIN, NO_TILED = (0,) * 7, (0,) * 4
# map name -> (B, H, W), and the (blocks, rows_per_wave) every thin plan has on it
MAPS = {"8x16": (2048, 8, 16), "5x52429": (1, 5, 52429), "9x9": (3237, 9, 9), "27x133": (73, 27, 133)}
THIN_SPLIT = {"8x16": (1024, 64), "5x52429": (683, 96), "9x9": (683, 96)}
M_MAX = 3237 * 81
POOL_WIDTH = 272


def _st():
    return _lib.stream_handle()


def thin(cin, cout, where, TF, TT, fat_is_co, groups, tpg):
    """A thin-form case: pointwise cin -> cout on the map `where`; the plan it must get."""
    B, H, W = MAPS[where]
    return {"name": "thin_%dto%d_%s" % (cin, cout, where), "geom": (B, cin, H, W, cout, 1, 1, 1, 0, 0, H, W), "nchw": 0,
            "gated": (False, True), "pool": True, "plan": (THIN, (TF, TT, fat_is_co, groups, tpg) + THIN_SPLIT[where], NO_TILED)}


def tiled(name, geom, plan4, nchw=0, gated=(False,), pool=False):
    """A tiled-form case. geom = (B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo); plan4 = (co_tiles, n_tiles, splits,
    steps_per_split)."""
    return {"name": name, "geom": geom, "nchw": nchw, "gated": gated, "pool": pool, "plan": (NCHW if nchw else NHWC, NO_THIN, plan4)}


def pw(cin, cout, where):
    B, H, W = MAPS[where]
    return (B, cin, H, W, cout, 1, 1, 1, 0, 0, H, W)


CASES = [
    # ---- thin: TF x TT x fat side at the smallest widths that name the instantiation (module docstring: <2, 2, x> does not exist)
    thin(16, 16, "9x9", 2, 1, 1, 1, 1),
    thin(32, 16, "9x9", 2, 1, 0, 1, 2),
    thin(24, 28, "8x16", 2, 2, 1, 1, 2),
    thin(28, 24, "8x16", 2, 2, 1, 1, 2),       # equal tile counts: the fat side is dy
    thin(16, 64, "8x16", 4, 1, 1, 1, 4),
    thin(64, 16, "8x16", 4, 1, 0, 1, 4),
    thin(20, 48, "9x9", 4, 2, 1, 1, 3),        # 3 tiles in a group of TF = 4
    thin(60, 24, "9x9", 4, 2, 0, 1, 4),
    thin(16, 96, "8x16", 6, 1, 1, 1, 6),
    thin(96, 16, "8x16", 6, 1, 0, 1, 6),
    thin(24, 144, "8x16", 6, 2, 1, 2, 5),      # groups of 5 + 4
    thin(136, 20, "8x16", 6, 2, 0, 2, 5),      # ragged last fat tile (8 channels), ragged thin tile (4)
    thin(16, 128, "8x16", 8, 1, 1, 1, 8),
    thin(128, 16, "9x9", 8, 1, 0, 1, 8),
    thin(24, 240, "9x9", 8, 2, 1, 2, 8),       # groups of 8 + 7: a group short of TF at tpg = 8
    thin(240, 32, "8x16", 8, 2, 0, 2, 8),
    thin(16, 272, "8x16", 6, 1, 1, 3, 6),      # three groups: 6 + 6 + 5
    thin(12, 20, "8x16", 2, 1, 1, 1, 2),       # fok and tok both mask lanes of the last tile
    thin(16, 116, "8x16", 8, 1, 1, 1, 8),
    # M = 2^18 + 1: rows_per_wave 96, the last block 96 + 96 + 65 + an idle wave
    thin(16, 96, "5x52429", 6, 1, 1, 1, 6),
    thin(136, 20, "5x52429", 6, 2, 0, 2, 5),
    thin(32, 16, "5x52429", 2, 1, 0, 1, 2),
    # ---- the boundary of the thin rule: one row short, and a 3-tile thin side
    tiled("rule_m262143_16to96", pw(16, 96, "27x133"), (2, 1, 745, 11), pool=True),
    tiled("rule_3tiles_40to240", pw(40, 240, "8x16"), (4, 1, 373, 22), gated=(False, True), pool=True),
    # ---- tiled: total_steps 7 and 8 (one split), 25 (9 + 9 + 7), 75 (8 x 9 + 3), 160 (20 splits: more than the reduce's 16 lanes)
    tiled("steps7_cout4", (1, 8, 14, 16, 4, 3, 3, 1, 1, 1, 14, 16), (1, 2, 1, 7)),
    tiled("steps8_cout68_m255", (1, 8, 15, 17, 68, 3, 3, 1, 1, 1, 15, 17), (2, 2, 1, 8)),
    tiled("steps25_3x1_cout68", (1, 24, 25, 32, 68, 3, 1, 1, 1, 0, 25, 32), (2, 2, 3, 9)),
    tiled("steps75_pw_cout132", (1, 16, 40, 60, 132, 1, 1, 1, 0, 0, 40, 60), (3, 1, 9, 9)),
    tiled("steps160_nc216_cout4", (2, 24, 51, 50, 4, 3, 3, 1, 1, 1, 51, 50), (1, 4, 20, 8)),
    # NCHW stem, NC = 27; stride 2 with TF-SAME pads (0, 1) / (1, 2); KH != KW; VALID stride 2 (row 7 and column 9 unread)
    tiled("stem_nc27_cout4", (3, 3, 9, 11, 4, 3, 3, 1, 1, 1, 9, 11), (1, 1, 1, 10), nchw=1),
    tiled("stem_s2_pad01_cout20", (3, 3, 8, 11, 20, 3, 3, 2, 0, 1, 4, 6), (1, 1, 1, 3), nchw=1),
    tiled("s2_pad01_nc216_cout132", (3, 24, 8, 11, 132, 3, 3, 2, 0, 1, 4, 6), (3, 4, 1, 3)),
    tiled("k5_s2_pad12_nc200_cout68", (2, 8, 10, 13, 68, 5, 5, 2, 1, 2, 5, 7), (2, 4, 1, 3)),
    tiled("k1x3_cin12_cout20", (3, 12, 7, 9, 20, 1, 3, 1, 0, 1, 7, 9), (1, 1, 1, 6)),
    tiled("s2_valid_8x10_cout36", (3, 12, 8, 10, 36, 3, 3, 2, 0, 0, 3, 4), (1, 2, 1, 2)),
    tiled("pw_s2_pad00_7x9", (2, 12, 7, 9, 20, 1, 1, 2, 0, 0, 4, 5), (1, 1, 1, 2)),
    # the gated tiled form: 672 -> 112 at 14x14
    tiled("gated_672to112_14x14", (3, 672, 14, 14, 112, 1, 1, 1, 0, 0, 14, 14), (2, 11, 2, 10), gated=(True,)),
]
CASE_IDS = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}

# the layers of the batched-reduce tests: (case name, gated). 4 x 27 and 20 x 27 end on a partial 16-output block.
BATCH_3 = [("stem_nc27_cout4", False), ("thin_12to20_8x16", True), ("pw_s2_pad00_7x9", False)]
BATCH_CYCLE = [("stem_nc27_cout4", False), ("k1x3_cin12_cout20", False), ("stem_s2_pad01_cout20", False), ("steps25_3x1_cout68", False),
               ("pw_s2_pad00_7x9", False), ("steps160_nc216_cout4", False), ("s2_valid_8x10_cout36", False), ("steps7_cout4", False)]
BATCH_48 = [BATCH_CYCLE[i % 8] for i in range(48)]
BATCH_48[5], BATCH_48[30] = ("thin_12to20_8x16", False), ("thin_32to16_5x52429", True)
BATCH_48[17] = ("gated_672to112_14x14", True)

# data gradient: name, (B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo)
DGRAD_CASES = [
    ("k3x1_cin12_cout20", (3, 12, 5, 7, 20, 3, 1, 1, 1, 0, 5, 7)),
    ("k1x3_cin20_cout12", (1, 20, 5, 7, 12, 1, 3, 1, 0, 1, 5, 7)),
    ("s2_odd_7x9_pad00", (3, 12, 7, 9, 36, 3, 3, 2, 0, 0, 3, 4)),
    ("s2_even_8x10_valid", (1, 12, 8, 10, 36, 3, 3, 2, 0, 0, 3, 4)),      # input row 7 and column 9: no output reads them
    ("s2_even_odd_8x11_pad01", (3, 20, 8, 11, 68, 3, 3, 2, 0, 1, 4, 6)),
    ("s2_odd_7x9_pad11", (1, 4, 7, 9, 68, 3, 3, 2, 1, 1, 4, 5)),
    ("s2_even_8x10_pad11", (3, 36, 8, 10, 4, 3, 3, 2, 1, 1, 4, 5)),
    ("pw_s2_8x10_valid", (3, 12, 8, 10, 20, 1, 1, 2, 0, 0, 4, 5)),       # odd input rows and columns: exact zeros
    ("k5_s2_pad12", (1, 8, 10, 13, 36, 5, 5, 2, 1, 2, 5, 7)),
]


# ---- inputs --------------------------------------------------------------------------------------------------------------
_pools = {}


def pools(family):
    """(x, dy) [M_MAX][272] of a family, made once: every 2^18-row case reads its leading rows and channels."""
    if family not in _pools:
        g = torch.Generator().manual_seed({"exact": 11, "normal": 12}[family])
        if family == "exact":
            _pools[family] = tuple(torch.randint(-3, 4, (M_MAX, POOL_WIDTH), generator=g).float() for _ in range(2))
        else:
            _pools[family] = tuple(torch.randn(M_MAX, POOL_WIDTH, generator=g) for _ in range(2))
    return _pools[family]


def make_gate(name, B, Cin, family):
    """[B][Cin]: exact - {0.5, 1, 2} and an eighth exact zeros; normal - uniform in (0, 1) and an eighth exact zeros."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000 + 7)
    if family == "exact":
        return torch.tensor([0.0, 0.5, 1.0, 2.0, 0.5, 1.0, 2.0, 1.0])[torch.randint(8, (B, Cin), generator=g)]
    gt = torch.rand(B, Cin, generator=g).clamp_min(2.0 ** -20)
    gt[torch.rand(B, Cin, generator=g) < 0.125] = 0.0
    return gt


def case_inputs(case, family):
    """CPU fp32 operands of a case: x in the layout the kernel reads ([B][H][W][Cin], or [B][Cin][H][W] for nchw), x_nchw
    [B][Cin][H][W] (None for the pooled 2^18-row cases, whose x rows are their own im2col), dy [M][Cout], gate [B][Cin]."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = case["geom"]
    M = B * Ho * Wo
    if case["pool"]:
        px, pdy = pools(family)
        return {"x": px[:M, :Cin].contiguous().view(B, H, W, Cin), "x_nchw": None, "dy": pdy[:M, :Cout].contiguous(),
                "gate": make_gate(case["name"], B, Cin, family)}
    g = torch.Generator().manual_seed(zlib.crc32(case["name"].encode()) % 100000)
    if family == "exact":
        xn = torch.randint(-3, 4, (B, Cin, H, W), generator=g).float()
        dy = torch.randint(-3, 4, (M, Cout), generator=g).float()
    else:
        xn, dy = torch.randn(B, Cin, H, W, generator=g), torch.randn(M, Cout, generator=g)
    return {"x": xn if case["nchw"] else xn.permute(0, 2, 3, 1).contiguous(), "x_nchw": xn, "dy": dy,
            "gate": make_gate(case["name"], B, Cin, family)}


def im2col(x_nchw, geom):
    """[M][Cin * KH * KW], columns in OIHW order (ci, kh, kw), rows m = (b, ho, wo): the rows the filter gradient sums over."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    nh, nw = (Ho - 1) * stride + KH, (Wo - 1) * stride + KW
    xp = F.pad(x_nchw, (pad_l, max(nw - W - pad_l, 0), pad_t, max(nh - H - pad_t, 0)))[:, :, :nh, :nw]
    cols = F.unfold(xp, (KH, KW), stride=stride)
    assert cols.shape == (B, Cin * KH * KW, Ho * Wo)
    return cols.transpose(1, 2).reshape(B * Ho * Wo, Cin * KH * KW)


def gated_columns(case, t, gated, dtype):
    """The B operand of the reduction in `dtype`: im2col of x * gate (the product rounded in `dtype`, as the kernel rounds it in
    fp32), [M][Cin * KH * KW]."""
    B, Cin, H, W, Cout, KH, KW = case["geom"][:7]
    if t["x_nchw"] is None:
        x = t["x"].to(dtype).view(B, H * W, Cin)
        return (x * t["gate"].to(dtype)[:, None, :] if gated else x).reshape(B * H * W, Cin)
    x = t["x_nchw"].to(dtype)
    return im2col(x * t["gate"].to(dtype)[:, :, None, None] if gated else x, case["geom"])


def reference64(case, t, gated):
    """dw [Cout][Cin * KH * KW] in float64."""
    return t["dy"].double().t() @ gated_columns(case, t, gated, torch.float64)


def exact_halves(ref64):
    """The exact family's reference in int64, in units of 0.5."""
    twice = ref64 * 2
    assert torch.equal(twice, twice.round()) and twice.abs().max().item() < 2.0 ** 24
    return twice.round().long()


# ---- the float32 restatement of the plan's summation order -----------------------------------------------------------------
def chain_partials(A, Bm, run, runs, co=None, n=None, budget=1 << 20):
    """partial[k][o] = the fp32 sum over the rows of run k (rows k * run ... , in order, one product after the other, from 0) of
    A[m][co[o]] * Bm[m][n[o]]; o runs over the whole (co, n) grid, co major, where co is None. Rows beyond M are zeros."""
    M, P = A.shape
    Q = Bm.shape[1]
    assert Bm.shape[0] == M and 0 <= runs * run - M
    if runs * run > M:
        A = torch.cat([A, torch.zeros(runs * run - M, P)])
        Bm = torch.cat([Bm, torch.zeros(runs * run - M, Q)])
    A3, B3 = A.view(runs, run, P), Bm.view(runs, run, Q)
    full = co is None
    S = P * Q if full else co.numel()
    out = torch.empty(runs, S)
    chunk = max(1, budget // S)
    for k0 in range(0, runs, chunk):
        a, b = A3[k0:k0 + chunk], B3[k0:k0 + chunk]
        if not full:
            a, b = a[:, :, co], b[:, :, n]
        c = a.shape[0]
        acc = torch.zeros((c, P, Q) if full else (c, S))
        tmp = torch.empty_like(acc)
        for r in range(run):
            if full:
                torch.mul(a[:, r, :, None], b[:, r, None, :], out=tmp)
            else:
                torch.mul(a[:, r], b[:, r], out=tmp)
            acc.add_(tmp)
        out[k0:k0 + c] = acc.view(c, S)
    return out


def add_waves(partial, waves=4):
    """[blocks * waves][S] -> [blocks][S]: a block's waves added in wave order."""
    p = partial.view(-1, waves, partial.shape[1])
    s = p[:, 0].clone()
    for w in range(1, waves):
        s.add_(p[:, w])
    return s


def reduce_lanes(partial, lanes=16):
    """The reduce kernel's order over [K][S] partial tiles: lane l adds tiles l, l + 16, ... from 0, then the lanes in order."""
    K, S = partial.shape
    per = []
    for ln in range(lanes):
        s = torch.zeros(S)
        for k in range(ln, K, lanes):
            s = s + partial[k]
        per.append(s)
    total = per[0]
    for ln in range(1, lanes):
        total = total + per[ln]
    return total


def blocked_chain(A, Bm, plan, co=None, n=None):
    """fp32 restatement of dw[co][n] = sum_m A[m][co] * Bm[m][n] in the order of `plan` (form, thin7, tiled4), parametrised by
    the plan's numbers alone."""
    form, th, td = plan
    if form == THIN:
        blocks, rpw = th[5], th[6]
        return reduce_lanes(add_waves(chain_partials(A, Bm, rpw, blocks * 4, co, n)))
    splits, sps = td[2], td[3]
    return reduce_lanes(chain_partials(A, Bm, sps * 32, splits, co, n))


def sample_outputs(P, Q, seed, sample=4096):
    """(co, n) index tensors of the outputs e32 is evaluated on: None, None (all) up to 8 * sample outputs, as linear_e32."""
    total = P * Q
    if total <= 8 * sample:
        return None, None
    idx = torch.unique(torch.randint(total, (sample + sample // 4,), generator=torch.Generator().manual_seed(seed)))
    assert idx.numel() >= sample
    return idx // Q, idx % Q


def e32_of(case, t, gated, ref64):
    A, Bm = t["dy"], gated_columns(case, t, gated, torch.float32)
    co, n = sample_outputs(A.shape[1], Bm.shape[1], zlib.crc32(case["name"].encode()) % 1000)
    chain = blocked_chain(A, Bm, case["plan"], co, n)
    want = ref64.reshape(-1) if co is None else ref64[co, n]
    return (chain.double() - want).abs().max().item()


# ---- running ---------------------------------------------------------------------------------------------------------------
def query_plan(lib, geom, x_nchw, gated):
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    form, th, td = ctypes.c_int(-1), (ctypes.c_int * 7)(), (ctypes.c_int * 4)()
    _lib.check(lib.orbit_op_conv2d_wgrad_plan(B, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, x_nchw, 1 if gated else 0,
                                              ctypes.byref(form), th, td), "orbit_op_conv2d_wgrad_plan")
    return form.value, tuple(th), tuple(td)


def run_wgrad(lib, device, case, d, gated):
    """orbit_op_conv2d_wgrad / _gated into a guarded dw; [Cout][Cin * KH * KW] on the CPU after the guard checks."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = case["geom"]
    dw = Guarded((Cout, Cin, KH, KW), device)
    p = _lib.dptr
    if gated:
        assert (KH, KW, stride, pad_t, pad_l, case["nchw"]) == (1, 1, 1, 0, 0, 0)
        _lib.check(lib.orbit_op_conv2d_wgrad_gated(p(d["x"]), p(d["gate"]), p(d["dy"]), p(dw.t), B, H, W, Cin, Cout, _st()),
                   "orbit_op_conv2d_wgrad_gated")
    else:
        _lib.check(lib.orbit_op_conv2d_wgrad(p(d["x"]), case["nchw"], p(d["dy"]), p(dw.t), B, H, W, Cin, Cout, KH, KW, stride, pad_t,
                                             pad_l, Ho, Wo, _st()), "orbit_op_conv2d_wgrad")
    torch.cuda.synchronize()
    return dw.cpu(case["name"]).view(Cout, Cin * KH * KW)


def profiled(lib, fn):
    """(fn(), {conv_* profiler row: launches}) of one call under the profiler."""
    lib.orbit_prof_enable(1)
    try:
        out = fn()
        rows = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    return out, {k: v for k, v in rows.items() if k.startswith("conv_")}


_device_cache = {}


def on_device(case, family, device):
    """CPU and device operands of (case, family); the last one is kept, so a case's gated and ungated runs share them."""
    key = (case["name"], family)
    if _device_cache.get("key") != key:
        _device_cache.clear()
        t = case_inputs(case, family)
        _device_cache.update(key=key, t=t, d={k: t[k].to(device) for k in ("x", "dy", "gate")})
    return _device_cache["t"], _device_cache["d"]


@pytest.fixture(scope="module", autouse=True)
def no_bf3(lib):
    with options(lib, conv_bf3=0):
        yield
    _device_cache.clear()
    _pools.clear()


_worst = {}


def report(what, form, err, e32, ref64):
    floor = 8 * U * ref64.abs().max().item()
    key = (FORM_NAME[form], "4e32" if 4 * e32 >= floor else "floor")
    unit = e32 if key[1] == "4e32" else floor
    if unit > 0:
        _worst[key] = max(_worst.get(key, 0.0), err / unit)
    print("\n[wgrad-forms] %s: err %.3g, e32 %.3g, err/e32 %.2f   (worst %s: %s)"
          % (what, err, e32, err / e32 if e32 > 0 else 0.0, key[0],
             ", ".join("err/%s %.2f" % (k[1], v) for k, v in sorted(_worst.items()) if k[0] == key[0])))


PARAMS = [pytest.param(c, g, f, id="%s-%s-%s" % (c["name"], "gated" if g else "plain", f))
          for c in CASES for f in ("exact", "normal") for g in c["gated"]]


@pytest.mark.parametrize("case,gated,family", PARAMS)
def test_wgrad_form(lib, device, case, gated, family):
    what = "%s/%s/%s" % (case["name"], "gated" if gated else "plain", family)
    form = case["plan"][0]
    assert query_plan(lib, case["geom"], case["nchw"], gated) == case["plan"], what
    t, d = on_device(case, family, device)
    got, rows = profiled(lib, lambda: run_wgrad(lib, device, case, d, gated))
    assert rows == {ROW[form]: 1}, (what, rows)
    again = run_wgrad(lib, device, case, d, gated)
    assert torch.equal(got, again), what + ": two runs differ in bits"
    ref64 = reference64(case, t, gated)
    assert got.shape == ref64.shape
    if family == "exact":
        halves = exact_halves(ref64)
        bad = ((got.double() * 2).long() != halves) | (got.double() != ref64)
        assert not bad.any(), "%s: %d of %d outputs differ from the integer reference, first at (co, n) = %s" % (
            what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()))
        assert torch.equal(got, ref64.float())
    else:
        e32 = e32_of(case, t, gated, ref64)
        report(what, form, (got.double() - ref64).abs().max().item(), e32, ref64)
        gate(got, ref64, e32, what)


# ---- batched reduce ----------------------------------------------------------------------------------------------------------
def run_batched(lib, device, layers, ds):
    """orbit_op_conv2d_wgrad_batched over `layers` [(case, gated)] with device operands ds; (rc, [Guarded dw])."""
    n = len(layers)
    dws = [Guarded((c["geom"][4], c["geom"][1], c["geom"][5], c["geom"][6]), device) for c, _ in layers]
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    geom = (ctypes.c_int * (12 * n))(*[v for c, _ in layers for v in (c["geom"][0], c["geom"][2], c["geom"][3], c["geom"][1]) + c["geom"][4:]])
    flags = (ctypes.c_int * n)(*[c["nchw"] for c, _ in layers])
    rc = lib.orbit_op_conv2d_wgrad_batched(n, ptrs([d["x"] for d in ds]), flags, ptrs([d["dy"] for d in ds]), ptrs([w.t for w in dws]),
                                           ptrs([d["gate"] if g else None for d, (_, g) in zip(ds, layers)]), geom, _st())
    torch.cuda.synchronize()
    return rc, dws


@pytest.mark.parametrize("spec", [BATCH_3[:1], BATCH_3, BATCH_48], ids=["n1", "n3", "n48"])
def test_batched_reduce_repeats_the_per_layer_bits(lib, device, spec):
    layers = [(BY_NAME[name], g) for name, g in spec]
    assert {c["plan"][0] for c, _ in layers} == ({NCHW} if len(spec) == 1 else {NHWC, NCHW, THIN})
    ops = {}
    for c, _ in layers:
        if c["name"] not in ops:
            t = case_inputs(c, "normal")
            ops[c["name"]] = {k: t[k].to(device) for k in ("x", "dy", "gate")}
    ds = [ops[c["name"]] for c, _ in layers]
    want = {}
    for (c, g), d in zip(layers, ds):
        if (c["name"], g) not in want:
            want[c["name"], g] = run_wgrad(lib, device, c, d, g)
    (rc, dws), rows = profiled(lib, lambda: run_batched(lib, device, layers, ds))
    _lib.check(rc, "orbit_op_conv2d_wgrad_batched")
    expect_rows = {}
    for c, _ in layers:
        expect_rows[ROW[c["plan"][0]]] = expect_rows.get(ROW[c["plan"][0]], 0) + 1
    assert rows == expect_rows, rows
    for k, ((c, g), dw) in enumerate(zip(layers, dws)):
        got = dw.cpu("layer %d (%s)" % (k, c["name"])).view(c["geom"][4], -1)
        assert torch.equal(got, want[c["name"], g]), "layer %d (%s): the batched reduce and the per-layer reduce differ in bits" % (
            k, c["name"])


def test_batched_reduce_refuses_49_layers(lib, device):
    c = BY_NAME["stem_nc27_cout4"]
    t = case_inputs(c, "normal")
    d = {k: t[k].to(device) for k in ("x", "dy", "gate")}
    n = WGRAD_REDUCE_JOBS + 1
    rc, dws = run_batched(lib, device, [(c, False)] * n, [d] * n)
    assert rc != 0 and "conv_wgrad_reduce_batched: 49 jobs" in _lib.last_error(), (rc, _lib.last_error())
    for dw in dws:
        flat = dw.flat.cpu()
        assert torch.isnan(flat[:dw.t.numel()]).all() and torch.equal(flat[dw.t.numel():], torch.full((GUARD,), SENTINEL)), \
            "a refused call wrote"
    rc, _ = run_batched(lib, device, [(c, False)] * WGRAD_REDUCE_JOBS, [d] * WGRAD_REDUCE_JOBS)
    assert rc == 0, _lib.last_error()


# ---- the data gradient's own kernels ------------------------------------------------------------------------------------------
def dgrad_inputs(name, geom):
    """Integers in [-3, 3]: dy [B][Cout][Ho][Wo], w OIHW, accumulate [B][Cin][H][W]."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)
    r = lambda *s: torch.randint(-3, 4, s, generator=g)  # noqa: E731
    return r(B, Cout, Ho, Wo), r(Cout, Cin, KH, KW), r(B, Cin, H, W)


def dgrad_reference(geom, dy, w):
    """dx [B][Cin][H][W] in int64: the transposed convolution spread over the padded map, cropped to the input; input rows and
    columns that no output reads are zeros."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    full = F.conv_transpose2d(dy.double(), w.double(), stride=stride)
    assert full.shape[2:] == ((Ho - 1) * stride + KH, (Wo - 1) * stride + KW)
    full = F.pad(full, (0, max(W + pad_l - full.shape[3], 0), 0, max(H + pad_t - full.shape[2], 0)))
    dx = full[:, :, pad_t:pad_t + H, pad_l:pad_l + W]
    assert torch.equal(dx, dx.round()) and dx.abs().max().item() < 2.0 ** 23
    return dx.long()


@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("name,geom", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_dgrad_exact(lib, device, name, geom, accumulate):
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    dy, w, acc = dgrad_inputs(name, geom)
    want = dgrad_reference(geom, dy, w) + (acc if accumulate else 0)
    d_dy = dy.float().permute(0, 2, 3, 1).contiguous().to(device)
    d_w = w.float().to(device)
    d_acc = acc.float().permute(0, 2, 3, 1).contiguous().to(device) if accumulate else None
    outs = []
    for _ in range(2):
        dx = Guarded((B, H, W, Cin), device)
        _lib.check(lib.orbit_op_conv2d_dgrad(_lib.dptr(d_dy), _lib.dptr(d_w), _lib.dptr(d_acc), _lib.dptr(dx.t), B, H, W, Cin, Cout, KH,
                                             KW, stride, pad_t, pad_l, Ho, Wo, _st()), "orbit_op_conv2d_dgrad")
        torch.cuda.synchronize()
        outs.append(dx.cpu(name).permute(0, 3, 1, 2))
    assert torch.equal(outs[0], outs[1]), name + ": two runs differ in bits"
    got = outs[0].double()
    assert torch.equal(got, got.round())
    bad = got.long() != want
    assert not bad.any(), "%s: %d of %d elements differ from the int64 reference, first at %s" % (
        name, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()))
    assert lib.orbit_get_option(b"conv_bf3") == 0
