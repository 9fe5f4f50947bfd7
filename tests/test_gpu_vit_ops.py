"""The transformer kernels of csrc/vit.hip one by one (orbit_op_vit_linear / _patch_embed / _layernorm / _attention) against
a float64 CPU evaluation of the same operation on the same fp32 inputs.

Reference: plain torch in float64 (F.linear + F.gelu / residual add; F.conv2d stride 32 + cat + pos_embed; F.layer_norm; the
four-line attention of tests/vit_pin.py). Outputs are NaN-filled before each call and followed by guard rows holding a
sentinel (a whole 128-row tile of them, so that a store that lost its row predicate lands in memory the test owns).

Tolerance: nothing here is tuned to the kernels. Every case measures its own yardstick on the reference side only - `e32`, the
largest error against float64 of a plain fp32 CPU evaluation of the same operation on the same inputs (torch fp32 for LayerNorm,
attention and the epilogues - LayerNorm in 8 channel orders, see test_layernorm; an explicit k = 0, 1, 2, ... fp32 multiply-add chain, the order the kernel documents, on a random
sample of >= 4096 outputs for the GEMMs - torch's blocked fp32 matmul is more accurate than any k-ordered chain). The gate is

    max |got - ref64|  <=  max(4 * e32, 8 * 2**-24 * max |ref64|)

4: the MFMA rounds its 2-deep product differently from the emulation, the GPU's expf / erff differ from the CPU's by an ulp or
two, and the maximum over another draw of rounding errors sits in the same tail; a wrong index, a dropped K step or a missing
max subtraction is orders of magnitude beyond it. The floor covers cases whose fp32 CPU evaluation happens to be exact (uniform
attention, constant rows). The GEMMs additionally meet, element by element, the textbook bound of ANY correct fp32 evaluation in
any order, gamma_(K+2) * (|x| @ |w|^T + |bias| + |residual|), gamma_n = n u / (1 - n u), u = 2**-24 (through erf-GELU: times
its Lipschitz constant 1.13, plus 8 u |pre-activation| for the activation's own arithmetic).

Largest err / e32 seen on the MI355X (every case prints its ratio; run with -s):
  token GEMM       2.49  (3072x768 residual, M = 3350: the maximum over 2.6 M outputs against a sample of 4096)
  patch embedding  1.96
  LayerNorm        1.11
  attention        1.21
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402

U = 2.0 ** -24
GUARD = 128          # guard rows after a GEMM / LayerNorm / attention output: one whole tall tile
GUARD_TOKENS = 192   # after the patch embedding's tokens: 127 GEMM rows past the tail reach token row 50 B + 129
SENTINEL = 7777.0
NAN = float("nan")
EPI_BIAS, EPI_GELU, EPI_RESIDUAL = 0, 1, 2
TILES = (64, 128)
SWITCH = 512         # launch_gemm: 128-row tiles when cdiv(M, 128) * (N / 128) >= 512 (include/orbit_hip.h)

# the model's own layers: (K, N, epilogue) of qkv, proj, fc1, fc2 of ViT-S/32 and ViT-B/32
LAYERS = [(384, 1152, EPI_BIAS), (384, 384, EPI_RESIDUAL), (384, 1536, EPI_GELU), (1536, 384, EPI_RESIDUAL),
          (768, 2304, EPI_BIAS), (768, 768, EPI_RESIDUAL), (768, 3072, EPI_GELU), (3072, 768, EPI_RESIDUAL)]
LAYER_IDS = ["%dx%d-%s" % (k, n, ("bias", "gelu", "residual")[e]) for k, n, e in LAYERS]
M_BIG = 3350         # 67 frames; 3350 % 128 = 22
# 275 % 128 = 19 and 3350 % 128 = 22: the last 128-row block has whole 32-row MFMA tiles past the tail
M_SWEEP = (1, 49, 50, 63, 64, 65, 127, 128, 129, 275, M_BIG)
WHAT = {EPI_BIAS: "vit_op_linear", EPI_GELU: "vit_op_linear_gelu", EPI_RESIDUAL: "vit_op_linear_residual"}


def _st():
    return _lib.stream_handle()


def _prof_rows(lib):
    """{profiling row: launches} since orbit_prof_enable(1)."""
    lib.orbit_prof_collect(None, None, None)
    buf, n = ctypes.create_string_buffer(48), ctypes.c_long(0)
    rows = {}
    for i in range(lib.orbit_prof_num_variants()):
        lib.orbit_prof_variant(i, buf, ctypes.byref(n), None, None, None)
        rows[buf.value.decode()] = rows.get(buf.value.decode(), 0) + n.value
    return rows


def _sync():
    torch.cuda.synchronize()


def gate(got, ref64, e32, what):
    """The module's gate (docstring); returns err / e32 and prints it."""
    assert torch.isfinite(got).all(), "%s: non-finite or unwritten output" % what
    err = (got.double() - ref64).abs().max().item()
    tol = max(4 * e32, 8 * U * ref64.abs().max().item())
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
    print("[vit-ops] %-58s err %.3g  e32 %.3g  err/e32 %.2f" % (what, err, e32, ratio))
    assert err <= tol, "%s: max |got - ref64| = %.4g > %.4g (e32 = %.4g, err / e32 = %.2f)" % (what, err, tol, e32, ratio)
    return ratio


# ---- token GEMM ------------------------------------------------------------------------------------------------------
def linear_inputs(K, N, M, family, seed):
    """fp32 x [M][K], w [N][K], bias [N], residual [M][N] of one input family."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = 0.5 * torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    if family == "outlier":     # 4 outlier K-columns of magnitude 100 against weights of normal scale
        cols = torch.randperm(K, generator=g)[:4]
        x[:, cols] = 100.0 * torch.sign(x[:, cols]) * (1 + 0.1 * torch.randn(M, 4, generator=g))
    elif family == "one_sign":  # no cancellation anywhere: a dropped K step has nothing to hide behind
        x, w, bias, res = x.abs(), w.abs(), bias.abs(), res.abs()
    else:
        assert family == "normal"
    return x, w, bias, res


def linear_ref64(x, w, bias, res, epi):
    """(ref64, elementwise textbook bound) of rows of x."""
    K = x.shape[1]
    pre = F.linear(x.double(), w.double(), None if bias is None else bias.double())
    mag = x.double().abs() @ w.double().abs().t()
    if bias is not None:
        mag = mag + bias.double().abs()
    gamma = (K + 2) * U / (1 - (K + 2) * U)
    if epi == EPI_GELU:
        return F.gelu(pre), 1.13 * gamma * mag + 8 * U * pre.abs()
    if epi == EPI_RESIDUAL:
        return pre + res.double(), gamma * (mag + res.double().abs())
    return pre, gamma * mag


def linear_e32(x, w, bias, res, epi, ref64, M, seed, sample=4096):
    """Yardstick of one case: error of the sequential-k fp32 chain (acc = acc + x[k] * w[k], k ascending; then the epilogue in
    torch fp32) against ref64, on a random sample of at least `sample` of the M x N outputs (all of them when there are few)."""
    N, K = w.shape
    total = M * N
    if total <= 8 * sample:
        idx = torch.arange(total)
    else:
        idx = torch.unique(torch.randint(total, (sample + sample // 4,), generator=torch.Generator().manual_seed(seed)))
        assert idx.numel() >= sample
    r, c = idx // N, idx % N
    xs, ws = x[r].t().contiguous(), w[c].t().contiguous()  # [K][samples]
    acc = torch.zeros(idx.numel())
    tmp = torch.empty_like(acc)
    for k in range(K):
        torch.mul(xs[k], ws[k], out=tmp)
        acc.add_(tmp)
    if bias is not None:
        acc = acc + bias[c]
    if epi == EPI_GELU:
        acc = F.gelu(acc)
    elif epi == EPI_RESIDUAL:
        acc = acc + res[r, c]
    return (acc.double() - ref64[r, c]).abs().max().item()


def run_linear(lib, device, x, w, bias, res, M, epi, tile, in_place=False):
    """orbit_op_vit_linear on the first M rows of the device tensors x / res. x is followed by 128 NaN rows, y (NaN-filled) and
    the residual by 128 guard rows; returns the M result rows on the CPU after checking the guard."""
    N, K = w.shape
    xp = torch.full((M + GUARD, K), NAN, device=device)
    xp[:M] = x[:M]
    y = torch.full((M + GUARD, N), NAN, device=device)
    y[M:] = SENTINEL
    rp = None
    if epi == EPI_RESIDUAL:
        if in_place:
            y[:M] = res[:M]
            rp = y
        else:
            rp = torch.zeros(M + GUARD, N, device=device)
            rp[:M] = res[:M]
    rc = lib.orbit_op_vit_linear(_lib.dptr(xp), _lib.dptr(w), _lib.dptr(bias), _lib.dptr(rp), _lib.dptr(y), M, N, K, epi, tile,
                                 _st())
    _lib.check(rc, "orbit_op_vit_linear")
    _sync()
    assert bool((y[M:] == SENTINEL).all()), "rows past M were written (M=%d N=%d K=%d tile=%d)" % (M, N, K, tile)
    return y[:M].cpu()


def check_linear(got, ref64, bound, e32, what):
    ratio = gate(got, ref64, e32, what)
    over = ((got.double() - ref64).abs() / bound.clamp_min(1e-300)).max().item()
    assert over <= 1.0, "%s: an element is %.3g x the worst-case fp32 bound gamma_(K+2) (|x| |w|^T + |b| + |r|)" % (what, over)
    return ratio


@pytest.mark.parametrize("K,N,epi", LAYERS, ids=LAYER_IDS)
def test_linear_every_row_count_at_both_tile_heights(lib, device, K, N, epi):
    """Both instantiations of the layer's kernel at M = 1 .. 3350 (tails of 1, 31, 32, 33, 63, 64, 65 rows and whole MFMA tiles
    past the tail), each against float64; rows past M of x are NaN, rows past M of y are guarded; and every row is BITWISE the
    same whatever M and whatever the tile height, per layer."""
    x, w, bias, res = linear_inputs(K, N, M_BIG, "normal", 100 + K + N)
    ref64, bound = linear_ref64(x, w, bias, res, epi)
    xd, wd, bd, rd = x.to(device), w.to(device), bias.to(device), res.to(device)
    lib.orbit_prof_enable(1)
    try:
        out = {}
        for M in M_SWEEP:
            e32 = linear_e32(x, w, bias, res, epi, ref64, M, seed=M)
            for tile in TILES:
                got = run_linear(lib, device, xd, wd, bd, rd, M, epi, tile)
                check_linear(got, ref64[:M], bound[:M], e32, "linear %s M=%d tile=%d" % (LAYER_IDS[LAYERS.index((K, N, epi))], M, tile))
                out[M, tile] = got
        rows = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    for tile in TILES:
        assert rows.get("%s<%d>" % (WHAT[epi], tile), 0) == len(M_SWEEP), rows
    big = out[M_BIG, 64]
    for (M, tile), got in out.items():
        assert torch.equal(got, big[:M]), "rows depend on M or on the tile height (M=%d, tile=%d)" % (M, tile)


@pytest.mark.parametrize("family", ["outlier", "one_sign"])
@pytest.mark.parametrize("K,N,epi", LAYERS, ids=LAYER_IDS)
def test_linear_input_distributions(lib, device, K, N, epi, family):
    """Outlier K-columns (trained ViTs have them) and all-positive operands (no cancellation: the accumulation's worst case)."""
    M = 275
    x, w, bias, res = linear_inputs(K, N, M, family, 200 + K + N)
    ref64, bound = linear_ref64(x, w, bias, res, epi)
    e32 = linear_e32(x, w, bias, res, epi, ref64, M, seed=1)
    xd, wd, bd, rd = x.to(device), w.to(device), bias.to(device), res.to(device)
    got = {}
    for tile in TILES:
        got[tile] = run_linear(lib, device, xd, wd, bd, rd, M, epi, tile)
        check_linear(got[tile], ref64, bound, e32, "linear %s %s tile=%d" % (LAYER_IDS[LAYERS.index((K, N, epi))], family, tile))
    assert torch.equal(got[64], got[128])


def _switch_rows(N):
    """Largest M that still takes 64-row tiles under the plan's rule (M + 1 takes 128-row tiles)."""
    n_tiles = N // 128
    return 128 * (-(-SWITCH // n_tiles) - 1)


@pytest.mark.parametrize("K,N,epi", [(384, 1152, EPI_BIAS), (384, 384, EPI_RESIDUAL), (384, 1536, EPI_GELU),
                                     (768, 2304, EPI_BIAS), (768, 768, EPI_RESIDUAL), (768, 3072, EPI_GELU)],
                         ids=lambda v: str(v))
def test_linear_auto_rule_switches_tile_height(lib, device, K, N, epi):
    """tile_rows = 0 at the last M of the 64-row side and the first M of the 128-row side, for every N of the models: the
    profiling row names the instantiation that ran, and each is checked against float64 (and equals the forced run)."""
    below = _switch_rows(N)
    assert -(-below // 128) * (N // 128) < SWITCH <= -(-(below + 1) // 128) * (N // 128)
    x, w, bias, res = linear_inputs(K, N, below + 1, "normal", 300 + K + N)
    ref64, bound = linear_ref64(x, w, bias, res, epi)
    xd, wd, bd, rd = x.to(device), w.to(device), bias.to(device), res.to(device)
    for M, tile in ((below, 64), (below + 1, 128)):
        e32 = linear_e32(x, w, bias, res, epi, ref64, M, seed=M)
        lib.orbit_prof_enable(1)
        try:
            got = run_linear(lib, device, xd, wd, bd, rd, M, epi, 0)
            rows = {k: v for k, v in _prof_rows(lib).items() if k.startswith("vit_")}
        finally:
            lib.orbit_prof_enable(0)
        assert rows == {"%s<%d>" % (WHAT[epi], tile): 1}, (M, rows)
        check_linear(got, ref64[:M], bound[:M], e32, "linear auto N=%d K=%d M=%d -> <%d>" % (N, K, M, tile))
        assert torch.equal(got, run_linear(lib, device, xd, wd, bd, rd, M, epi, tile))


@pytest.mark.parametrize("K,N,epi", [l for l in LAYERS if l[2] == EPI_RESIDUAL],
                         ids=[i for i, l in zip(LAYER_IDS, LAYERS) if l[2] == EPI_RESIDUAL])
def test_linear_residual_in_place(lib, device, K, N, epi):
    """y aliasing the residual: how orbit_vit_forward calls proj and fc2 (x += ...)."""
    x, w, bias, res = linear_inputs(K, N, M_BIG, "normal", 400 + K + N)
    ref64, bound = linear_ref64(x, w, bias, res, epi)
    xd, wd, bd, rd = x.to(device), w.to(device), bias.to(device), res.to(device)
    for M in (129, M_BIG):
        e32 = linear_e32(x, w, bias, res, epi, ref64, M, seed=M)
        for tile in TILES:
            got = run_linear(lib, device, xd, wd, bd, rd, M, epi, tile, in_place=True)
            check_linear(got, ref64[:M], bound[:M], e32, "linear in place %dx%d M=%d tile=%d" % (K, N, M, tile))
            assert torch.equal(got, run_linear(lib, device, xd, wd, bd, rd, M, epi, tile))


@pytest.mark.parametrize("K,N,epi", LAYERS, ids=LAYER_IDS)
def test_linear_without_bias(lib, device, K, N, epi):
    """bias = NULL (CLIP's patch embedding has none; the epilogue must not read it)."""
    M = 129
    x, w, _, res = linear_inputs(K, N, M, "normal", 500 + K + N)
    ref64, bound = linear_ref64(x, w, None, res, epi)
    e32 = linear_e32(x, w, None, res, epi, ref64, M, seed=2)
    xd, wd, rd = x.to(device), w.to(device), res.to(device)
    for tile in TILES:
        got = run_linear(lib, device, xd, wd, None, rd, M, epi, tile)
        check_linear(got, ref64, bound, e32, "linear no bias %dx%d tile=%d" % (K, N, tile))


# ---- patch embedding -------------------------------------------------------------------------------------------------
def patch_inputs(D, B, seed):
    """Frames in which every (channel, row, column) position has its own value (a ramp over c, h, w plus per-frame noise): a
    swapped kh / kw or a c * 1024 vs c * 32 slip in the gather then moves the result by far more than rounding."""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(-1.0, 1.0, 3 * 224 * 224).reshape(1, 3, 224, 224)
    frames = ramp + 0.25 * torch.randn(B, 3, 224, 224, generator=g)
    w = torch.randn(D, 3, 32, 32, generator=g) / 3072 ** 0.5
    bias = 0.5 * torch.randn(D, generator=g)
    pos = torch.randn(50, D, generator=g)
    cls = torch.randn(D, generator=g)
    return frames, w, bias, pos, cls


def patch_ref64(frames, w, bias, pos, cls):
    t = F.conv2d(frames.double(), w.double(), None if bias is None else bias.double(), stride=32).flatten(2).transpose(1, 2)
    return torch.cat((cls.double().expand(t.shape[0], 1, -1), t), dim=1) + pos.double()


def run_patch_embed(lib, device, frames, w, bias, pos, cls, B, tile):
    D = w.shape[0]
    tokens = torch.full((B * 50 + GUARD_TOKENS, D), NAN, device=device)
    tokens[B * 50:] = SENTINEL
    fr = frames[:B].contiguous()
    rc = lib.orbit_op_vit_patch_embed(_lib.dptr(fr), _lib.dptr(w), _lib.dptr(bias), _lib.dptr(pos), _lib.dptr(cls),
                                      _lib.dptr(tokens), B, D, tile, _st())
    _lib.check(rc, "orbit_op_vit_patch_embed")
    _sync()
    assert bool((tokens[B * 50:] == SENTINEL).all()), "token rows past B * 50 were written (B=%d tile=%d)" % (B, tile)
    return tokens[:B * 50].cpu().reshape(B, 50, D)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("D", [384, 768])
def test_patch_embed(lib, device, D, with_bias):
    Bs = (1, 2, 3, 67)
    frames, w, bias, pos, cls = patch_inputs(D, max(Bs), 600 + D)
    if not with_bias:
        bias = None
    ref64 = patch_ref64(frames, w, bias, pos, cls)
    # the same GEMM, k = c * 1024 + kh * 32 + kw (F.unfold's order is the OIHW filter's), for the sequential-k yardstick and
    # the textbook bound
    rows = F.unfold(frames, 32, stride=32).transpose(1, 2).reshape(-1, 3072).contiguous()
    w2 = w.reshape(D, 3072)
    posr = pos[1:].repeat(max(Bs), 1)
    gamma = (3072 + 3) * U / (1 - (3072 + 3) * U)
    mag = rows.double().abs() @ w2.double().abs().t() + posr.double().abs()
    if bias is not None:
        mag = mag + bias.double().abs()
    bound = gamma * mag
    dev = [None if t is None else t.to(device) for t in (frames, w, bias, pos, cls)]
    row0 = cls + pos[0]
    out = {}
    lib.orbit_prof_enable(1)
    try:
        for B in Bs:
            patches64 = ref64[:B, 1:].reshape(B * 49, D)
            e32 = linear_e32(rows, w2, bias, posr, EPI_RESIDUAL, patches64, B * 49, seed=B)
            for tile in TILES:
                got = run_patch_embed(lib, device, *dev, B, tile)
                what = "patch_embed D=%d %s B=%d tile=%d" % (D, "bias" if with_bias else "no bias", B, tile)
                gate(got, ref64[:B], e32, what)
                over = ((got[:, 1:].reshape(B * 49, D).double() - patches64).abs() / bound[:B * 49]).max().item()
                assert over <= 1.0, "%s: an element is %.3g x the worst-case fp32 bound" % (what, over)
                assert torch.equal(got[:, 0], row0.expand(B, D)), "%s: class-token row is not cls_token + pos_embed[0]" % what
                out[B, tile] = got
        prof = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    for tile in TILES:
        assert prof.get("vit_op_patch_embed<%d>" % tile, 0) == len(Bs), prof
    for (B, tile), got in out.items():
        assert torch.equal(got, out[max(Bs), 64][:B]), "tokens depend on the batch or the tile height (B=%d, tile=%d)" % (B, tile)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 3, 4, 5, 50, 3350)  # blocks hold 4 rows
LN_FAMILIES = ("normal", "offset", "near_constant", "constant", "outlier")


def layernorm_inputs(D, rows, family, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    if family == "offset":            # mean >> std: a one-pass E[x^2] - E[x]^2 variance cancels here
        x = x + 1e3
    elif family == "near_constant":   # variance ~ 1e-6: eps decides the answer
        x = 3.0 + 1e-3 * x
    elif family == "constant":        # row sums exact in fp32: variance exactly 0, the output is beta
        x = torch.full((rows, D), 3.0)
    elif family == "outlier":
        x[torch.arange(rows), torch.randint(D, (rows,), generator=g)] = 1e4
    # gamma and beta of mixed sign and magnitude (1e-2 .. 1e1)
    gamma = torch.randn(D, generator=g) * 10 ** (3 * torch.rand(D, generator=g) - 2)
    beta = torch.randn(D, generator=g) * 10 ** (3 * torch.rand(D, generator=g) - 2)
    return x, gamma, beta


def run_layernorm(lib, device, x, gamma, beta, eps, layout):
    """layout: 'plain' (contiguous rows, separate y), 'strided' (x_stride = 50 D, the final-norm form: row r is token 0 of frame
    r, every other token NaN) or 'in_place'. Guard rows (a whole block and more) follow y."""
    rows, D = x.shape
    if layout == "strided":
        xb = torch.full((rows, 50, D), NAN, device=device)
        xb[:, 0] = x
        xs = 50 * D
    else:
        xb = torch.full((rows + GUARD, D), SENTINEL, device=device)
        xb[:rows] = x
        xs = D
    if layout == "in_place":
        y = xb
    else:
        y = torch.full((rows + GUARD, D), NAN, device=device)
        y[rows:] = SENTINEL
    rc = lib.orbit_op_vit_layernorm(_lib.dptr(xb), xs, _lib.dptr(y), D, rows, D, _lib.dptr(gamma), _lib.dptr(beta), eps, _st())
    _lib.check(rc, "orbit_op_vit_layernorm")
    _sync()
    assert bool((y[rows:] == SENTINEL).all()), "rows past the last were written (rows=%d, %s)" % (rows, layout)
    return y[:rows].cpu()


@pytest.mark.parametrize("family", LN_FAMILIES)
@pytest.mark.parametrize("D", [384, 768])
def test_layernorm(lib, device, D, family):
    x, gamma, beta = layernorm_inputs(D, max(LN_ROWS), family, 700 + D)
    gd, bd = gamma.to(device), beta.to(device)
    # LayerNorm is equivariant under a permutation of the D channels, and each order is another plain fp32 evaluation with its
    # own rounding errors. A row's error at mean >> std is ONE draw (the rounding of its mean, shared by its D outputs), so
    # with 1..5 rows a single evaluation is a yardstick of 1..5 draws; torch fp32 in 8 channel orders gives every row 8.
    gp = torch.Generator().manual_seed(D)
    perms = [torch.arange(D)] + [torch.randperm(D, generator=gp) for _ in range(7)]
    for eps in (1e-6, 1e-5):
        ref64 = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), eps)
        row_e32 = torch.zeros(x.shape[0], dtype=torch.float64)
        for p in perms:
            y32 = F.layer_norm(x[:, p].contiguous(), (D,), gamma[p], beta[p], eps)
            row_e32 = torch.maximum(row_e32, (y32.double() - ref64[:, p]).abs().amax(dim=1))
        if family == "near_constant":  # the two eps give different answers here: a swapped eps is a macroscopic error
            other = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5 if eps == 1e-6 else 1e-6)
            assert (other - ref64).abs().max().item() > 0.1 * ref64.abs().max().item()
        for rows in LN_ROWS:
            e32 = row_e32[:rows].max().item()
            xd = x[:rows].to(device)
            for layout in ("plain", "strided", "in_place"):
                got = run_layernorm(lib, device, xd, gd, bd, eps, layout)
                gate(got, ref64[:rows], e32, "layernorm D=%d %s eps=%g rows=%d %s" % (D, family, eps, rows, layout))
                if family == "constant":
                    assert torch.equal(got, beta.expand(rows, D)), "constant rows must give beta exactly"


# ---- attention -------------------------------------------------------------------------------------------------------
ATTN_FAMILIES = ("normal", "logits_200", "one_key", "identical_keys", "max_at_49", "huge_v", "head_constant_v")


def attention_ref(qkv, heads):
    """tests/vit_pin.py _Attention.forward between qkv and proj, in qkv's dtype."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    q, k, v = qkv.reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4).unbind(0)
    attn = ((q @ k.transpose(-2, -1)) * (C // heads) ** -0.5).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, N, C)


def attention_inputs(B, heads, family, seed):
    """qkv [B][50][3 * heads * 64] fp32 of one family."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, 50, heads, 64, generator=g) for _ in range(3))
    unit = torch.full((64,), 0.125)  # |unit| = 1
    if family == "logits_200":
        # logits reach +-200: expf overflows fp32 above 88.7, so a softmax without the max subtraction gives inf / inf here
        top = (torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / 8).abs().max().item()
        s = (200.0 / top) ** 0.5
        q, k = q * s, k * s
    elif family == "one_key":
        # key 17 dominates every row (logit ~ 50 against ~ 0): P is one-hot to e^-50, the output is V[17]
        q = 0.1 * q + 4.0 * unit
        k = 0.1 * k
        k[:, 17] += 100.0 * unit
    elif family == "identical_keys":
        # every logit of a row is the same number: P is exactly 1/50, the output is the mean of V
        k = k[:, :1].expand(B, 50, heads, 64).contiguous()
    elif family == "max_at_49":
        # logits rise by 4 per token from -196 to 0 at token 49, the last valid lane of the softmax wave (lanes 50..63 are masked)
        q = 0.01 * q + 8.0 * unit
        k = 0.01 * k + (4.0 * (torch.arange(50.0) - 49.0))[None, :, None, None] * unit
    elif family == "huge_v":
        v[B - 1, 23, heads - 1, 5] = 1e6
    elif family == "head_constant_v":
        v = (torch.arange(heads) + 1.0)[None, None, :, None].expand(B, 50, heads, 64).contiguous()
    else:
        assert family == "normal"
    return torch.stack((q, k, v), dim=2).reshape(B, 50, 3 * heads * 64).contiguous()


def run_attention(lib, device, qkv, heads):
    B, D = qkv.shape[0], heads * 64
    out = torch.full((B * 50 + GUARD, D), NAN, device=device)
    out[B * 50:] = SENTINEL
    qd = qkv.to(device)
    rc = lib.orbit_op_vit_attention(_lib.dptr(qd), _lib.dptr(out), B, D, heads, _st())
    _lib.check(rc, "orbit_op_vit_attention")
    _sync()
    assert bool((out[B * 50:] == SENTINEL).all()), "rows past B * 50 were written"
    return out[:B * 50].cpu().reshape(B, 50, D)


@pytest.mark.parametrize("family", ATTN_FAMILIES)
@pytest.mark.parametrize("D,heads", [(384, 6), (768, 12)])
def test_attention(lib, device, D, heads, family):
    for B in (1, 2, 5, 7):  # 5 and 7 frames: 30, 42, 60, 84 workgroups
        qkv = attention_inputs(B, heads, family, 800 + D + B)
        ref64 = attention_ref(qkv.double(), heads)
        e32 = (attention_ref(qkv, heads).double() - ref64).abs().max().item()
        v = qkv.reshape(B, 50, 3, heads, 64)[:, :, 2].double()
        if family == "logits_200":
            q, k = qkv.reshape(B, 50, 3, heads, 64)[:, :, 0].double(), qkv.reshape(B, 50, 3, heads, 64)[:, :, 1].double()
            assert (torch.einsum("bqhd,bkhd->bhqk", q, k) / 8).abs().max().item() > 199.0
        elif family == "one_key":
            assert (ref64 - v[:, 17:18].reshape(B, 1, D)).abs().max().item() < 1e-12
        elif family == "identical_keys":
            assert (ref64 - v.mean(1, keepdim=True).reshape(B, 1, D)).abs().max().item() < 1e-12
        got = run_attention(lib, device, qkv, heads)
        gate(got, ref64, e32, "attention D=%d %s B=%d" % (D, family, B))
        if family == "head_constant_v":
            want = (torch.arange(heads) + 1.0).repeat_interleave(64)
            assert (got - want).abs().max().item() <= 64 * U * heads, "a head's output is not in columns h * 64 .. h * 64 + 63"
