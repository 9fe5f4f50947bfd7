"""The train-mode BatchNorm chain of csrc/train_ops.hip, kernel by kernel against float64 on the CPU:

    statistics sweep              orbit_op_bn_train_forward        bn_stats_partial_kernel -> finalize -> scale_shift_act_kernel
    finalize from partials        orbit_op_bn_stats_from_partials  (bn_partial_compact_kernel above 2048 blocks) -> bn_stats_finalize_kernel
    Gram statistics               orbit_op_bn_stats_from_gram      gram_partial_kernel -> gram_bn_finalize_kernel
    pooled apply                  orbit_op_scale_shift_act_pool    scale_shift_act_pool_kernel (-> orbit_op_se_gate2)
    apply / three-pass backward   orbit_op_scale_shift_act, orbit_op_bn_backward_ex
    backward behind a producer    orbit_op_bn_backward_reduced     (compaction) -> bn_bwd_finalize_kernel -> bn_bwd_apply_kernel

Every output buffer is pre-filled with NaN and followed by a guard tail of sentinel floats (Guarded of test_gpu_se_path.py): no
NaN may remain and the tail must come back untouched. Every case is named after the layout it exercises, and asserts that layout
through the host queries orbit_op_bn_reduce_plan / orbit_op_se_pool_chunks before it launches (tests/test_bn_chain_reference.py
checks the same tables, and the inputs' properties, without a GPU).

Two input families.

EXACT: y and dout are integers in {-3..3} without 0, given means are integers, given invstd is 0.5, (where sums are checked)
scale = 1, shift = 0 and the activation is none or ReLU; the Gram test has x integer in {-2..2} and weights that are multiples of
1/8. Every term and every partial sum of every reduction is then an exactly representable fp32 number (< 2^24 in magnitude), so
ANY summation order gives the same bits and a row, chunk or compaction group counted zero times or twice changes them:
  sums of g, g * xhat, pooling partials, dbeta, dgamma   bit-equal to the float64 sums rounded once to fp32
  mean                                                   bit-equal to float(S / M)
  invstd                                                 within 1 fp32 ulp of float(1 / sqrt(var64 + double(float(eps))))
  scale, shift, running statistics                       within 4 u (sum of the magnitudes of the terms of their expression),
                                                         u = 2^-24 (the compiler may or may not contract those fp32 expressions)

GAUSSIAN: y ~ N(mu_c, sigma_c^2) with |mu_c| <= sigma_c in every channel. THAT CONDITION IS PART OF THE FAMILY: the one-pass
E[y^2] - mean^2 over fp32 partial sums has a conditioning limit, and strongly offset or near-constant channels are out of scope
here. A one-row batch is a constant channel (its one-pass variance is rounding noise of y^2, ~u y^2, against eps), so the M == 1
case runs in the exact family only. Gates:
  elementwise out, dy, dres   elementwise_gate of test_gpu_se_path.py: max(2e-5, 4 E32) max(1, max |ref64|), E32 the error of the
                              fp32 CPU evaluation of the same closed form
  mean                        1e-6 max(1, max |mean64|);   invstd: |invstd - ref| sqrt(var + eps) <= 1e-5   (test_bn_train_forward)
  running mean / variance     1e-6 / 1e-5 times max(1, max |ref64|)                                          (test_bn_train_forward)
  scale, shift                4 u (sum of term magnitudes) around the float64 fold of the mean / invstd THE KERNEL WROTE
  dgamma, dbeta               max(4 E32, 8 u max |ref64|)                                                    (test_gpu_vit_ops.py)
  pooling partials            |partial - S| <= 2 n u A over the n outputs THE KERNEL WROTE                   (test_gpu_se_path.py)
  pooled means                2 (chunks + 1) u sum_k |partial_k| / HW                                        (test_gpu_se_path.py)
ReLU cases whose mask enters a gradient or a sum keep |z| >= 1e-3 at the activation's input (relu_margin), so no mask can flip;
the statistics sweep's ReLU output is continuous in z and needs none. All backward references are closed forms, not autograd.

The statistics sweep's fp32 yardstick evaluates the fold the chain defines, y * scale + shift (not the centred form), so that E32
carries the fold's own cancellation where invstd is large (one row: 1 / sqrt(eps) = 316).

Each check prints "[bn_chain] family: case: err, bound, ratio" (pytest -s). Largest err / bound per family on the MI355X (157
tests, 1961 checks, 6.5 s in all; every case met every gate, no kernel had to change):
  exact   mean, dgamma, dbeta, dres, pooling partials (none / ReLU): bit-equal everywhere;  invstd: 0 ulp everywhere
          scale / shift 0.59 (C1028 nblk1, shift)   running statistics 0.56 (C1028 nblk64, mean)   out 0.25 (one_row)
          dy 0.006 (reduced C1028 nblk4099)   SiLU pooling partials 0.21, pooled means 0.43
  gauss   mean 0.22, invstd 0.023, running 0.22, out 0.014 (all idle4_one_block, 37x24)   scale / shift 0.41 (C1028 nblk64)
          dgamma 0.35, dbeta 0.35 (37x24)   dy 0.011, dres 0.012, apply 0.007 (the grid-trip cases)
          pooling partials 0.30 (two_groups_36_chunks_last3, SiLU)   pooled means 0.46 (two_chunks_32_31)   pool out 0.006
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
import test_gpu_se_path as SE  # noqa: E402
from test_gpu_se_path import Guarded, elementwise_gate  # noqa: E402

NONE, RELU, SILU = 0, 1, 2
POST = 1  # ORBIT_BN_RESIDUAL_POST_ACT
U = 2.0 ** -24
EPS = 1e-5
EPS32 = float(np.float32(EPS))
RELU_MARGIN = 1e-3
ACT_NAMES = {NONE: "none", RELU: "relu", SILU: "silu"}


def _report(family, what, err, bound):
    if bound == 0.0:  # bit-equality: err is the largest difference, 0 or a failure
        print("\n[bn_chain] %s: %s: err %.3g, bound 0, ratio %s" % (family, what, err, "0" if err == 0.0 else "inf"))
        return 0.0 if err == 0.0 else float("inf")
    return SE._report(family, what, err, bound, tag="bn_chain")


def _egate(family, what, got, want64, want32):
    elementwise_gate(family, what, got, want64, want32, report=_report)


def _st():
    return _lib.stream_handle()


def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 1000003 + int(v)
    return torch.Generator().manual_seed(s % (2 ** 31))


def guarded_from(t, device):
    """A guarded buffer that starts with the content of the CPU tensor t (NaN allowed)."""
    g = Guarded(tuple(t.shape), device)
    g.t.copy_(t.to(device))
    return g


def untouched(g):
    flat = g.flat.cpu()
    n = g.t.numel()
    return bool(torch.isnan(flat[:n]).all()) and torch.equal(flat[n:], torch.full((SE.GUARD,), SE.SENTINEL))


# ---- inputs (CPU, deterministic; tests/test_bn_chain_reference.py checks their properties) -----------------------------------------
def exact_ints(shape, top, g):
    """Integers in {-top..top} without 0."""
    return (torch.randint(1, top + 1, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def gauss_params(C, g):
    sigma = 0.5 + torch.rand(C, generator=g)
    return sigma * (2.0 * torch.rand(C, generator=g) - 1.0), sigma  # |mu_c| <= sigma_c


def y_input(family, M, C, *seed):
    g = _gen(*seed)
    if family == "exact":
        return exact_ints((M, C), 3, g)
    mu, sigma = gauss_params(C, g)
    return torch.randn(M, C, generator=g) * sigma + mu


def affine_input(C, *seed):
    g = _gen(*seed)
    return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2  # gamma, beta


def relu_margin(y, scale, shift, res=None):
    """y, moved where needed so that |y * scale + shift (+ res)| >= RELU_MARGIN in float64 (scale > 0)."""
    z = y.double() * scale.double() + shift.double() + (0.0 if res is None else res.double())
    push = torch.where(z >= 0, 1.0, -1.0) * (2.0 * RELU_MARGIN) / scale.double()
    y = torch.where(z.abs() < 2.0 * RELU_MARGIN, y.double() + push, y.double()).float()
    z = y.double() * scale.double() + shift.double() + (0.0 if res is None else res.double())
    assert z.abs().min().item() >= RELU_MARGIN
    return y


# ---- references ---------------------------------------------------------------------------------------------------------------------
def act_fn(act, z):
    return z if act == NONE else torch.relu(z) if act == RELU else z * torch.sigmoid(z)


def apply_ref(y, scale, shift, res, act, post, dtype):
    """act(y * scale + shift + res), or act(y * scale + shift) + res for the post-activation skip."""
    z = y.to(dtype) * scale.to(dtype) + shift.to(dtype)
    if res is not None and not post:
        z = z + res.to(dtype)
    a = act_fn(act, z)
    return a + res.to(dtype) if post else a


def bwd_ref(dout, y, out, mean, invstd, gamma, scale, shift, train, act, post, dres0, dtype):
    """Closed form of the three-pass backward: g = dout * act'(.), dbeta = sum g, dgamma = sum g xhat,
    dy = gamma invstd (g - dbeta / M - xhat dgamma / M) (eval: gamma invstd g), dres = dout (post) or g, plus dres0."""
    c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    dout, y, mean, invstd, gamma, scale, shift, dres0 = (c(t) for t in (dout, y, mean, invstd, gamma, scale, shift, dres0))
    M = y.shape[0]
    if act == NONE:
        g = dout
    elif act == RELU:
        g = dout * ((y * scale + shift > 0) if post else (out > 0)).to(dtype)
    else:
        z = y * scale + shift
        s = torch.sigmoid(z)
        g = dout * s * (1 + z * (1 - s))
    xh = (y - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    k1 = invstd if gamma is None else gamma * invstd
    dy = k1 * (g - dbeta / M - xh * (dgamma / M)) if train else k1 * g
    dres = dout if post else g
    return dy, (dres if dres0 is None else dres + dres0), dgamma, dbeta


def stats64(y):
    """(sum, mean, biased variance) per channel in float64, two-pass."""
    yd = y.double()
    S = yd.sum(0)
    mean = S / y.shape[0]
    return S, mean, ((yd - mean) ** 2).mean(0)


def ulp32(t):
    return torch.from_numpy(np.spacing(np.abs(t.float().numpy()))).double()


def bit_equal(family, what, got, want64):
    want = want64.float()
    err = (got.double() - want.double()).abs().max().item()
    _report(family, what, err, 0.0)
    assert torch.equal(got, want), (what, err, int((got != want).sum()))


def bounded(family, what, got, want64, bound):
    """|got - want64| <= bound elementwise (bound a tensor); reports the largest ratio."""
    err = (got.double() - want64).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0)).max().item()
    _report(family, what, ratio, 1.0)
    assert not (err > bound).any(), (what, err.max().item(), ratio)


def check_stats(family, what, M, S64, mean64, var64, got_mean, got_invstd):
    sd = torch.sqrt(var64 + EPS32)
    if family == "exact":
        bit_equal("exact_mean", what, got_mean, S64 / M)
        ref = (1.0 / sd).float()
        bounded("exact_invstd_ulp", what, got_invstd, ref.double(), ulp32(ref))
    else:
        err = (got_mean.double() - mean64).abs().max().item()
        bound = 1e-6 * max(1.0, mean64.abs().max().item())
        _report("gauss_mean", what, err, bound)
        assert err <= bound, (what, err, bound)
        err = ((got_invstd.double() - 1.0 / sd).abs() * sd).max().item()
        _report("gauss_invstd", what, err, 1e-5)
        assert err <= 1e-5, (what, err)


def running_ref(mean64, var64, M, momentum, rm0, rv0, cb):
    """(running mean, magnitude of its terms, running variance, magnitude of its terms) after one update."""
    m = float(np.float32(momentum))
    unbiased = var64 * M / (M - 1) if M > 1 else var64
    cbd = torch.zeros_like(mean64) if cb is None else cb.double()
    if m >= 1.0:
        return mean64 + cbd, mean64.abs() + cbd.abs(), unbiased, unbiased.abs()
    keep = 1.0 - m
    return (keep * rm0.double() + m * (mean64 + cbd), keep * rm0.double().abs() + m * (mean64.abs() + cbd.abs()),
            keep * rv0.double() + m * unbiased, keep * rv0.double().abs() + m * unbiased.abs())


def check_running(family, what, mean64, var64, M, momentum, rm0, rv0, cb, got_rm, got_rv):
    rm, tm, rv, tv = running_ref(mean64, var64, M, momentum, rm0, rv0, cb)
    if family == "exact":
        bounded("exact_running", what + " mean", got_rm, rm, 4 * U * tm)
        bounded("exact_running", what + " var", got_rv, rv, 4 * U * tv)
    else:
        for name, got, want, c in (("mean", got_rm, rm, 1e-6), ("var", got_rv, rv, 1e-5)):
            err = (got.double() - want).abs().max().item()
            bound = c * max(1.0, want.abs().max().item())
            _report("gauss_running", "%s %s" % (what, name), err, bound)
            assert err <= bound, (what, name, err, bound)


def check_fold(family, what, mean_for_fold, invstd_for_fold, gamma, beta, got_scale, got_shift):
    """scale = gamma invstd, shift = beta - mean scale around float64 values of mean / invstd (exact family: the references;
    Gaussian family: what the kernel wrote)."""
    g = torch.ones_like(mean_for_fold) if gamma is None else gamma.double()
    b = torch.zeros_like(mean_for_fold) if beta is None else beta.double()
    sc = g * invstd_for_fold
    bounded(family + "_fold", what + " scale", got_scale, sc, 4 * U * sc.abs())
    bounded(family + "_fold", what + " shift", got_shift, b - mean_for_fold * sc, 4 * U * (b.abs() + (mean_for_fold * sc).abs()))


def check_sum_gate(family, what, got, want64, want32):
    """dgamma / dbeta: max(4 E32, 8 u max |ref64|)."""
    e32 = (want32.double() - want64).abs().max().item()
    tol = max(4 * e32, 8 * U * want64.abs().max().item())
    err = (got.double() - want64).abs().max().item()
    _report(family, what, err, tol)
    assert err <= tol, (what, err, tol, e32)


# ---- the layout queries -------------------------------------------------------------------------------------------------------------
def reduce_plan(lib, M, C):
    v = [ctypes.c_int(-1) for _ in range(5)]
    _lib.check(lib.orbit_op_bn_reduce_plan(M, C, *[ctypes.byref(x) for x in v]), "orbit_op_bn_reduce_plan")
    return dict(zip(("G", "R", "ygroups", "nblk", "rpb"), (x.value for x in v)))


def pool_chunks(lib, B, HW, C):
    chunks, rpc = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(lib.orbit_op_se_pool_chunks(B, HW, C, ctypes.byref(chunks), ctypes.byref(rpc)), "orbit_op_se_pool_chunks")
    return chunks.value, rpc.value


def block_rows(M, rpb):
    return [min(rpb, M - r) for r in range(0, M, rpb)]


# name, M, C, claimed layout: G quad lanes x R row lanes (idle = 256 - G R threads), column groups, row blocks, rows of the first
# and of the last block
STATS_CASES = [
    ("one_row", 1, 8, dict(G=2, R=128, idle=0, ygroups=1, nblk=1, rpb=1, last=1)),
    ("idle4_one_block", 37, 24, dict(G=6, R=42, idle=4, ygroups=1, nblk=1, rpb=37, last=37)),
    ("four_blocks_last32", 131, 100, dict(G=25, R=10, idle=6, ygroups=1, nblk=4, rpb=33, last=32)),
    ("six_blocks_last82", 517, 40, dict(G=10, R=25, idle=6, ygroups=1, nblk=6, rpb=87, last=82)),
    ("r128_three_blocks", 1025, 8, dict(G=2, R=128, idle=0, ygroups=1, nblk=3, rpb=342, last=341)),
    ("two_groups_last2", 130, 1028, dict(G=256, R=1, idle=0, ygroups=2, nblk=33, rpb=4, last=2)),
    ("two_groups_513_blocks_last1", 2049, 1028, dict(G=256, R=1, idle=0, ygroups=2, nblk=513, rpb=4, last=1)),
]
STATS_IDS = [c[0] for c in STATS_CASES]


def assert_reduce_plan(lib, M, C, claim):
    p = reduce_plan(lib, M, C)
    rows = block_rows(M, p["rpb"])
    got = dict(p, idle=256 - p["G"] * p["R"], last=rows[-1])
    assert got == claim and len(rows) == p["nblk"] and sum(rows) == M, (got, claim)


# ---- a. statistics sweep ------------------------------------------------------------------------------------------------------------
def run_bn_train_forward(lib, device, y, gamma, beta, momentum, rm0, rv0, res, act):
    M, C = y.shape
    d = _lib.dptr
    dev = [None if t is None else t.to(device).contiguous() for t in (y, gamma, beta, res)]
    out, sm, si = Guarded((M, C), device), Guarded((C,), device), Guarded((C,), device)
    rm = rv = None
    if rm0 is not None:
        rm, rv = guarded_from(rm0, device), guarded_from(rv0, device)
    _lib.check(lib.orbit_op_bn_train_forward(d(dev[0]), M, C, d(dev[1]), d(dev[2]), EPS, momentum, d(rm.t) if rm else None,
                                             d(rv.t) if rv else None, d(dev[3]), act, d(out.t), d(sm.t), d(si.t), _st()),
               "orbit_op_bn_train_forward")
    torch.cuda.synchronize()
    return (out.cpu("out"), sm.cpu("save_mean"), si.cpu("save_invstd"), rm.cpu("running_mean") if rm else None,
            rv.cpu("running_var") if rv else None)


# (a one-row batch is a constant channel: outside the Gaussian family, module docstring)
SWEEP_PARAMS = [c + (f,) for c in STATS_CASES for f in ("exact", "gauss") if not (f == "gauss" and c[1] == 1)]


@pytest.mark.parametrize("name,M,C,claim,family", SWEEP_PARAMS, ids=["%s-%s" % (c[0], c[4]) for c in SWEEP_PARAMS])
def test_statistics_sweep(lib, device, name, M, C, claim, family):
    assert_reduce_plan(lib, M, C, claim)
    y = y_input(family, M, C, 1, M, C)
    gamma, beta = affine_input(C, 2, M, C)
    g = _gen(3, M, C)
    res = torch.randn(M, C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    nan = torch.full((C,), float("nan"))
    S64, mean64, var64 = stats64(y)
    xh64 = (y.double() - mean64) / torch.sqrt(var64 + EPS32)
    # the fp32 yardstick evaluates the operation as the chain defines it: statistics, then the FOLDED y * scale + shift (with one
    # row, invstd = 1 / sqrt(eps) = 316 and the fold cancels y * scale against mean * scale: E32 carries that, the 2e-5 floor not)
    mean32 = y.mean(0)
    scale32 = gamma / torch.sqrt(((y - mean32) ** 2).mean(0) + EPS32)
    z32 = y * scale32 + (beta - mean32 * scale32)
    combos = [(act, r, mom) for act in (NONE, RELU) for r in (False, True) for mom in (None, 0.1)] + [(NONE, False, 1.0)]
    for act, with_res, mom in combos:
        what = "%s/%s act=%s res=%d momentum=%s" % (name, family, ACT_NAMES[act], with_res, mom)
        start = (None, None) if mom is None else (nan, nan) if mom >= 1.0 else (rm0, rv0)
        out, sm, si, rm, rv = run_bn_train_forward(lib, device, y, gamma, beta, mom or 0.0, start[0], start[1],
                                                   res if with_res else None, act)
        check_stats(family, what, M, S64, mean64, var64, sm, si)
        if mom is not None:  # (momentum 1: the NaN-prefilled slots came back finite - Guarded.cpu - and equal the batch statistics)
            check_running(family, what, mean64, var64, M, mom, rm0, rv0, None, rm, rv)
        want64 = act_fn(act, xh64 * gamma.double() + beta.double() + (res.double() if with_res else 0.0))
        want32 = act_fn(act, z32 + res if with_res else z32)
        _egate(family + "_out", what, out, want64, want32)


# ---- b. finalize from a producer's partials, with the compaction stage ----------------------------------------------------------------
# nblk -> (group size, compacted blocks, blocks of the last group); no entry: no compaction (nblk <= 2048)
COMPACTION = {2049: (3, 683, 3), 2050: (3, 684, 1), 4099: (5, 820, 4)}
PARTIAL_NBLK = [1, 64, 2048, 2049, 2050, 4099]
ROWS_PER_PARTIAL = 2  # the CPU stand-in of a producer sums blocks of two rows, the last block one row


def partial_rows(nblk):
    return ROWS_PER_PARTIAL * nblk - 1 if nblk > 1 else 5


def block_sums(t, nblk):
    """float64 sums of t [M][C] over the producer's row blocks: [nblk][C]."""
    M, C = t.shape
    if nblk == 1:
        return t.double().sum(0, keepdim=True)
    pad = torch.zeros(ROWS_PER_PARTIAL * nblk - M, C, dtype=torch.float64)
    return torch.cat([t.double(), pad]).view(nblk, ROWS_PER_PARTIAL, C).sum(1)


@functools.lru_cache(maxsize=2)
def stats_partials(family, C, nblk):
    """(y [M][C], partial [nblk][2][C] fp32: block sums of y and y^2 - exact in the exact family, rounded once in the Gaussian)."""
    y = y_input(family, partial_rows(nblk), C, 4, C, nblk)
    return y, torch.stack([block_sums(y, nblk), block_sums(y.double() ** 2, nblk)], 1).float().contiguous()


def run_stats_from_partials(lib, device, pd, nblk, M, C, gamma, beta, cb, momentum, rm0, rv0, fold=True):
    d = _lib.dptr
    dev = [None if t is None else t.to(device).contiguous() for t in (gamma, beta, cb)]
    mean, invstd = Guarded((C,), device), Guarded((C,), device)
    scale, shift = (Guarded((C,), device), Guarded((C,), device)) if fold else (None, None)
    rm, rv = (guarded_from(rm0, device), guarded_from(rv0, device)) if rm0 is not None else (None, None)
    _lib.check(lib.orbit_op_bn_stats_from_partials(d(pd), nblk, M, C, d(dev[0]), d(dev[1]), d(dev[2]), EPS, momentum,
                                                   d(rm.t) if rm else None, d(rv.t) if rv else None, d(mean.t), d(invstd.t),
                                                   d(scale.t) if fold else None, d(shift.t) if fold else None, _st()),
               "orbit_op_bn_stats_from_partials")
    torch.cuda.synchronize()
    return (mean.cpu("mean"), invstd.cpu("invstd"), scale.cpu("scale") if fold else None, shift.cpu("shift") if fold else None,
            rm.cpu("running_mean") if rm else None, rv.cpu("running_var") if rv else None)


@pytest.mark.parametrize("family", ["exact", "gauss"])
@pytest.mark.parametrize("nblk", PARTIAL_NBLK)
@pytest.mark.parametrize("C", [8, 1028])
def test_stats_from_partials(lib, device, C, nblk, family):
    y, partial = stats_partials(family, C, nblk)
    M = y.shape[0]
    pd = partial.to(device)
    before = pd.clone()
    # the reference reads the partials the kernel is given: float64 sums of them (exact family: the sums of y and y^2 themselves)
    S64, SS64 = partial[:, 0].double().sum(0), partial[:, 1].double().sum(0)
    mean64 = S64 / M
    var64 = (SS64 / M - mean64 * mean64).clamp_min(0.0)
    if family == "exact":
        assert torch.equal(S64, y.double().sum(0)) and torch.equal(SS64, (y.double() ** 2).sum(0))
    gamma, beta = affine_input(C, 5, C, nblk)
    g = _gen(6, C, nblk)
    cb, rm0, rv0 = torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    for with_cb in (False, True):
        for affine in (False, True):
            what = "C%d nblk%d/%s conv_bias=%d affine=%d" % (C, nblk, family, with_cb, affine)
            ga, be = (gamma, beta) if affine else (None, None)
            mean, invstd, scale, shift, rm, rv = run_stats_from_partials(lib, device, pd, nblk, M, C, ga, be, cb if with_cb else None,
                                                                         0.1, rm0, rv0)
            check_stats(family, what, M, S64, mean64, var64, mean, invstd)
            check_running(family, what, mean64, var64, M, 0.1, rm0, rv0, cb if with_cb else None, rm, rv)
            if family == "exact":
                check_fold("exact", what, mean64, 1.0 / torch.sqrt(var64 + EPS32), ga, be, scale, shift)
            else:
                check_fold("gauss", what, mean.double(), invstd.double(), ga, be, scale, shift)
    # statistics only (no fold, no running statistics), then momentum 1 onto NaN slots with the conv bias
    bare = run_stats_from_partials(lib, device, pd, nblk, M, C, None, None, None, 0.1, None, None, fold=False)
    assert torch.equal(bare[0], mean) and torch.equal(bare[1], invstd)
    nan = torch.full((C,), float("nan"))
    what = "C%d nblk%d/%s momentum=1" % (C, nblk, family)
    _, _, _, _, rm, rv = run_stats_from_partials(lib, device, pd, nblk, M, C, gamma, beta, cb, 1.0, nan, nan)
    check_running(family, what, mean64, var64, M, 1.0, rm0, rv0, cb, rm, rv)
    assert torch.equal(pd, before), "the caller's partials were modified"


@pytest.mark.parametrize("nblk", [1, 2050])
def test_stats_from_partials_clamps_a_negative_variance(lib, device, nblk):
    """Every block: 64 rows of the constant 3 with a sum of squares one part in 2^18 short (576 (1 - 2^-18) and three times it, a
    compaction group's sum, are fp32 numbers): ss / M - mean^2 = -9 * 2^-18 exactly. The clamp must give invstd = 1 / sqrt(eps),
    variance 0, and no NaN."""
    C, M = 8, 64 * nblk
    partial = torch.empty(nblk, 2, C)
    partial[:, 0], partial[:, 1] = 192.0, 576.0 * (1.0 - 2.0 ** -18)
    S64, SS64 = partial[:, 0].double().sum(0), partial[:, 1].double().sum(0)
    assert ((SS64 / M - (S64 / M) ** 2) == -9.0 * 2.0 ** -18).all()
    nan = torch.full((C,), float("nan"))
    mean, invstd, scale, shift, rm, rv = run_stats_from_partials(lib, device, partial.to(device), nblk, M, C, None, None, None, 1.0,
                                                                 nan, nan)
    zero = torch.zeros(C, dtype=torch.float64)
    what = "negative variance nblk%d" % nblk
    check_stats("exact", what, M, S64, S64 / M, zero, mean, invstd)
    check_fold("exact", what, S64 / M, 1.0 / torch.sqrt(zero + EPS32), None, None, scale, shift)
    bit_equal("exact_running", what + " mean", rm, S64 / M)
    bit_equal("exact_running", what + " var", rv, zero)


# ---- c. Gram statistics, exact family ------------------------------------------------------------------------------------------------
GRAM_P = [1, 255, 256, 257, 8193, 31337]  # one block / several; a clamped last pixel; a last block shorter than a thread round


def gram_inputs(Cin, P):
    g = _gen(7, Cin, P)
    x = torch.randint(-2, 3, (P, Cin), generator=g).float()
    w = torch.randint(-8, 9, (6 * Cin, Cin), generator=g).float() / 8.0
    return x, w


@pytest.mark.parametrize("P", GRAM_P)
@pytest.mark.parametrize("Cin", [16, 24])
def test_gram_statistics_exact(lib, device, Cin, P):
    x, w = gram_inputs(Cin, P)
    C = w.shape[0]
    y = x.double() @ w.double().t()  # multiples of 1/8, exact
    S64, mean64, var64 = stats64(y)
    xd, wd = x.to(device), w.to(device)
    mean, invstd = Guarded((C,), device), Guarded((C,), device)
    _lib.check(lib.orbit_op_bn_stats_from_gram(_lib.dptr(xd), P, Cin, _lib.dptr(wd), C, EPS, _lib.dptr(mean.t), _lib.dptr(invstd.t),
                                               _st()), "orbit_op_bn_stats_from_gram")
    torch.cuda.synchronize()
    check_stats("exact", "gram Cin%d P%d" % (Cin, P), P, S64, mean64, var64, mean.cpu("mean"), invstd.cpu("invstd"))


# ---- d. pooled apply ----------------------------------------------------------------------------------------------------------------
# name, B, HW, C, rows of every chunk
POOL_CASES = [
    ("one_pixel", 2, 1, 8, [1]),
    ("one_chunk_idle4", 3, 35, 24, [35]),
    ("two_chunks_32_31", 5, 63, 100, [32, 31]),
    ("two_chunks_98_97", 1, 195, 40, [98, 97]),
    ("two_groups_13_chunks_last1", 2, 49, 1028, [4] * 12 + [1]),
    ("two_groups_36_chunks_last3", 3, 143, 1280, [4] * 35 + [3]),
]
POOL_IDS = [c[0] for c in POOL_CASES]
SE_R = 4


def pool_inputs(family, B, HW, C, act):
    y = y_input(family, B * HW, C, 8, B, HW, C).view(B, HW, C)
    if family == "exact":
        return y, torch.ones(C), torch.zeros(C)
    g = _gen(9, B, HW, C)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    if act == RELU:
        y = relu_margin(y, scale, shift)
    return y, scale, shift


def check_pool_partials(family, what, out, pool, rows):
    """pool[b][k][c] against the float64 sum of the outputs the kernel wrote over chunk k's rows: 2 n u A."""
    od = out.double()
    worst, r0 = 0.0, 0
    for k, nr in enumerate(rows):
        blk = od[:, r0:r0 + nr]
        S, A = blk.sum(1), blk.abs().sum(1)
        bound = 2.0 * nr * U * A
        err = (pool[:, k].double() - S).abs()
        worst = max(worst, torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0)).max().item())
        assert not (err > bound).any(), (what, "chunk %d" % k, err.max().item())
        r0 += nr
    _report(family + "_pool_partial", what, worst, 1.0)


@pytest.mark.parametrize("family", ["exact", "gauss"])
@pytest.mark.parametrize("act", [NONE, RELU, SILU], ids=["none", "relu", "silu"])
@pytest.mark.parametrize("name,B,HW,C,rows", POOL_CASES, ids=POOL_IDS)
def test_pooled_apply(lib, device, name, B, HW, C, rows, act, family):
    chunks, rpc = pool_chunks(lib, B, HW, C)
    assert block_rows(HW, rpc) == rows and chunks == len(rows) and sum(rows) == HW, (chunks, rpc)
    y, scale, shift = pool_inputs(family, B, HW, C, act)
    what = "%s/%s act=%s" % (name, family, ACT_NAMES[act])
    d = _lib.dptr
    dev = [t.to(device).contiguous() for t in (y, scale, shift)]
    out, pool = Guarded((B, HW, C), device), Guarded((B, chunks, C), device)
    _lib.check(lib.orbit_op_scale_shift_act_pool(d(dev[0]), d(dev[1]), d(dev[2]), act, B, HW, C, d(out.t), d(pool.t), _st()),
               "orbit_op_scale_shift_act_pool")
    se = SE.se_inputs(B, C, SE_R, chunks, HW, seed=C + HW)
    sed = [se[k].to(device).contiguous() for k in ("w1", "b1", "w2", "b2")]
    gate, pooled = Guarded((B, C), device), Guarded((B, C), device)
    _lib.check(lib.orbit_op_se_gate2(d(pool.t), chunks, HW, d(sed[0]), d(sed[1]), d(sed[2]), d(sed[3]), B, C, SE_R, d(gate.t), d(pooled.t),
                                     _st()), "orbit_op_se_gate2")
    torch.cuda.synchronize()
    out, pool, pooled = out.cpu("out"), pool.cpu("pool"), pooled.cpu("pooled")
    gate.cpu("gate")
    want64 = apply_ref(y, scale, shift, None, act, False, torch.float64)
    _egate(family + "_pool_out", what, out, want64, apply_ref(y, scale, shift, None, act, False, torch.float32))
    if family == "exact" and act != SILU:  # integers: the outputs and every sum of them are exact
        assert torch.equal(out.double(), want64)
        starts = [sum(rows[:k]) for k in range(len(rows))]
        bit_equal("exact_pool_partial", what, pool, torch.stack([want64[:, r0:r0 + nr].sum(1) for r0, nr in zip(starts, rows)], 1))
    else:
        check_pool_partials(family, what, out, pool, rows)
    bound = 2.0 * (chunks + 1) * U * pool.double().abs().sum(1) / HW
    bounded(family + "_pooled_mean", what, pooled, pool.double().sum(1) / HW, bound)
    if family == "exact" and act != SILU:  # ... so the pooled means are those of the reference, to the same bound
        bounded("exact_pooled_mean", what + " vs reference", pooled, want64.mean(1), bound)


# ---- e. apply and backward forms ------------------------------------------------------------------------------------------------------
FORM_SHAPES = [(37, 24), (131, 100), (130, 1028)]


def form_inputs(M, C, act, post, pre_res):
    """Gaussian-family inputs of an apply / backward form: y, the statistics of y as given mean / invstd, gamma, the folded scale /
    shift, a residual (None unless the form has one), dout and a prefill for dres. ReLU keeps its margin at the mask's input."""
    y = y_input("gauss", M, C, 10, M, C)
    gamma, beta = affine_input(C, 11, M, C)
    _, mean64, var64 = stats64(y)
    mean, invstd = mean64.float(), (1.0 / torch.sqrt(var64 + EPS32)).float()
    scale = gamma * invstd
    shift = beta - mean * scale
    g = _gen(12, M, C)
    res = torch.randn(M, C, generator=g) if (post or pre_res) else None
    dout, dres0 = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    if act == RELU:
        y = relu_margin(y, scale, shift, None if post else res)
    return dict(y=y, mean=mean, invstd=invstd, gamma=gamma, scale=scale, shift=shift, res=res, dout=dout, dres0=dres0)


def run_scale_shift_act(lib, device, y, scale, shift, res, act, flags):
    M, C = y.shape
    d = _lib.dptr
    dev = [None if t is None else t.to(device).contiguous() for t in (y, scale, shift, res)]
    out = Guarded((M, C), device)
    _lib.check(lib.orbit_op_scale_shift_act(d(dev[0]), d(dev[1]), d(dev[2]), d(dev[3]), act, M, C, flags, d(out.t), _st()),
               "orbit_op_scale_shift_act")
    torch.cuda.synchronize()
    return out.cpu("out")


@pytest.mark.parametrize("form", ["plain", "pre_residual", "post_residual"])
@pytest.mark.parametrize("act", [NONE, RELU, SILU], ids=["none", "relu", "silu"])
@pytest.mark.parametrize("M,C", FORM_SHAPES)
def test_apply_forms(lib, device, M, C, act, form):
    post = form == "post_residual"
    t = form_inputs(M, C, act, post, form == "pre_residual")
    out = run_scale_shift_act(lib, device, t["y"], t["scale"], t["shift"], t["res"], act, POST if post else 0)
    _egate("gauss_apply", "%dx%d act=%s %s" % (M, C, ACT_NAMES[act], form), out,
           apply_ref(t["y"], t["scale"], t["shift"], t["res"], act, post, torch.float64),
           apply_ref(t["y"], t["scale"], t["shift"], t["res"], act, post, torch.float32))


def run_bn_backward_ex(lib, device, t, out, train, act, flags, dres_mode, with_fold=True, gamma=True):
    """dres_mode: None (no dres), "write" or "accumulate" (onto t["dres0"])."""
    M, C = t["y"].shape
    d = _lib.dptr
    names = ("dout", "y", "mean", "invstd", "gamma", "scale", "shift")
    dev = {k: t[k].to(device).contiguous() for k in names}
    outd = None if out is None else out.to(device).contiguous()
    dy, dgamma, dbeta = Guarded((M, C), device), Guarded((C,), device), Guarded((C,), device)
    dres = None if dres_mode is None else guarded_from(t["dres0"], device) if dres_mode == "accumulate" else Guarded((M, C), device)
    _lib.check(lib.orbit_op_bn_backward_ex(d(dev["dout"]), d(outd), d(dev["y"]), M, C, d(dev["gamma"]) if gamma else None, d(dev["mean"]),
                                           d(dev["invstd"]), d(dev["scale"]) if with_fold else None,
                                           d(dev["shift"]) if with_fold else None, train, act, flags, d(dy.t),
                                           d(dres.t) if dres else None, int(dres_mode == "accumulate"), d(dgamma.t), d(dbeta.t), _st()),
               "orbit_op_bn_backward_ex")
    torch.cuda.synchronize()
    return dy.cpu("dy"), dres.cpu("dres") if dres else None, dgamma.cpu("dgamma"), dbeta.cpu("dbeta")


@pytest.mark.parametrize("post", [0, 1], ids=["pre", "post"])
@pytest.mark.parametrize("act", [NONE, RELU, SILU], ids=["none", "relu", "silu"])
@pytest.mark.parametrize("M,C", FORM_SHAPES)
def test_backward_forms(lib, device, M, C, act, post):
    """The full cross with train / eval and dres {none, written, accumulated} inside. Without the post-activation skip ReLU takes its
    mask from the forward output (of act(z + residual), fp32 CPU evaluation; the margin holds at z + residual)."""
    t = form_inputs(M, C, act, bool(post), act == RELU and not post)
    out = apply_ref(t["y"], t["scale"], t["shift"], t["res"], act, bool(post), torch.float32)
    for train in (1, 0):
        for mode in (None, "write", "accumulate"):
            what = "%dx%d act=%s post=%d train=%d dres=%s" % (M, C, ACT_NAMES[act], post, train, mode)
            dres0 = t["dres0"] if mode == "accumulate" else None
            ref = [bwd_ref(t["dout"], t["y"], out, t["mean"], t["invstd"], t["gamma"], t["scale"], t["shift"], train, act, bool(post),
                           dres0, dt) for dt in (torch.float64, torch.float32)]
            dy, dres, dgamma, dbeta = run_bn_backward_ex(lib, device, t, out, train, act, POST if post else 0, mode)
            _egate("gauss_dy", what, dy, ref[0][0], ref[1][0])
            if mode is not None:
                _egate("gauss_dres", what, dres, ref[0][1], ref[1][1])
            check_sum_gate("gauss_dgamma", what, dgamma, ref[0][2], ref[1][2])
            check_sum_gate("gauss_dbeta", what, dbeta, ref[0][3], ref[1][3])


def exact_backward_inputs(M, C):
    g = _gen(13, M, C)
    return dict(y=exact_ints((M, C), 3, g), dout=exact_ints((M, C), 3, g), mean=torch.randint(-2, 3, (C,), generator=g).float(),
                invstd=torch.full((C,), 0.5), gamma=affine_input(C, 14, M, C)[0], scale=torch.ones(C), shift=torch.zeros(C),
                dres0=exact_ints((M, C), 3, g))


@pytest.mark.parametrize("post", [0, 1], ids=["pre", "post"])
@pytest.mark.parametrize("name,M,C,claim", STATS_CASES, ids=STATS_IDS)
def test_backward_exact(lib, device, name, M, C, claim, post):
    """Exact family through bn_bwd_partial_kernel's layouts: integer g = dout (no activation), xhat = (y - mean) / 2 a multiple of
    1/2 - dgamma and dbeta bit-equal. dres: written plain and accumulated onto integers, both exact."""
    assert_reduce_plan(lib, M, C, claim)
    t = exact_backward_inputs(M, C)
    for train in (1, 0):
        for mode in ("write", "accumulate"):
            what = "%s post=%d train=%d dres=%s" % (name, post, train, mode)
            dres0 = t["dres0"] if mode == "accumulate" else None
            ref = [bwd_ref(t["dout"], t["y"], None, t["mean"], t["invstd"], t["gamma"], t["scale"], t["shift"], train, NONE, bool(post),
                           dres0, dt) for dt in (torch.float64, torch.float32)]
            dy, dres, dgamma, dbeta = run_bn_backward_ex(lib, device, t, None, train, NONE, POST if post else 0, mode)
            bit_equal("exact_dgamma", what, dgamma, ref[0][2])
            bit_equal("exact_dbeta", what, dbeta, ref[0][3])
            bit_equal("exact_dres", what, dres, ref[0][1])
            _egate("exact_dy", what, dy, ref[0][0], ref[1][0])


def test_apply_and_backward_refusals(lib, device):
    """Every ORBIT_REQUIRE of orbit_op_scale_shift_act and orbit_op_bn_backward_ex: refused, outputs untouched."""
    M, C = 37, 24
    t = form_inputs(M, C, SILU, True, False)
    dv = {k: v.to(device).contiguous() for k, v in t.items()}
    d = _lib.dptr
    out = Guarded((M, C), device)
    y, sc, sh, res = d(dv["y"]), d(dv["scale"]), d(dv["shift"]), d(dv["res"])
    bad_apply = {
        "missing y": (None, sc, sh, res, SILU, M, C, 0, d(out.t)),
        "missing scale": (y, None, sh, res, SILU, M, C, 0, d(out.t)),
        "missing shift": (y, sc, None, res, SILU, M, C, 0, d(out.t)),
        "missing out": (y, sc, sh, res, SILU, M, C, 0, None),
        "unknown flag": (y, sc, sh, res, SILU, M, C, 2, d(out.t)),
        "unknown activation": (y, sc, sh, res, 3, M, C, 0, d(out.t)),
        "empty batch": (y, sc, sh, res, SILU, 0, C, 0, d(out.t)),
        "C % 4": (y, sc, sh, res, SILU, M, 22, 0, d(out.t)),
        "post-activation skip without its residual": (y, sc, sh, None, SILU, M, C, POST, d(out.t)),
    }
    for what, args in bad_apply.items():
        assert lib.orbit_op_scale_shift_act(*args, _st()) != 0, what
        assert "scale_shift_act" in _lib.last_error(), (what, _lib.last_error())
    torch.cuda.synchronize()
    assert untouched(out), "a refused orbit_op_scale_shift_act wrote its output"

    dy, dres, dgamma, dbeta = Guarded((M, C), device), Guarded((M, C), device), Guarded((C,), device), Guarded((C,), device)
    good = dict(dout=d(dv["dout"]), out=d(dv["y"]), y=y, M=M, C=C, gamma=d(dv["gamma"]), mean=d(dv["mean"]), invstd=d(dv["invstd"]),
                scale=sc, shift=sh, train=1, act=SILU, flags=0, dy=d(dy.t), dres=d(dres.t), acc=0, dgamma=d(dgamma.t), dbeta=d(dbeta.t))
    bad_bwd = {
        "missing dout": dict(dout=None), "missing y": dict(y=None), "missing mean": dict(mean=None),
        "missing invstd": dict(invstd=None), "missing dy": dict(dy=None),
        "unknown flag": dict(flags=2), "unknown activation": dict(act=3), "empty batch": dict(M=0), "C % 4": dict(C=22),
        "ReLU without the forward output": dict(act=RELU, out=None),
        "SiLU without scale": dict(scale=None), "SiLU without shift": dict(shift=None),
        "post-activation ReLU without scale / shift": dict(act=RELU, flags=POST, out=None, scale=None, shift=None),
    }
    for what, change in bad_bwd.items():
        a = dict(good, **change)
        assert lib.orbit_op_bn_backward_ex(*[a[k] for k in good], _st()) != 0, what
        assert "bn_backward" in _lib.last_error(), (what, _lib.last_error())
    torch.cuda.synchronize()
    for g in (dy, dres, dgamma, dbeta):
        assert untouched(g), "a refused orbit_op_bn_backward_ex wrote an output"


# ---- f. the backward behind a producer's partial sums ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def reduced_inputs(C, nblk):
    """Exact-family g and y over partial_rows(nblk) rows, and the producer's partial [nblk][2][C] of g and g * xhat, summed on the CPU."""
    t = exact_backward_inputs(partial_rows(nblk), C)
    xh = (t["y"].double() - t["mean"].double()) * 0.5
    t["partial"] = torch.stack([block_sums(t["dout"], nblk), block_sums(t["dout"].double() * xh, nblk)], 1).float().contiguous()
    return t


@pytest.mark.parametrize("nblk", [1, 2048, 2050, 4099])
@pytest.mark.parametrize("C", [8, 1028])
def test_backward_reduced(lib, device, C, nblk):
    t = reduced_inputs(C, nblk)
    M = t["y"].shape[0]
    d = _lib.dptr
    dev = {k: t[k].to(device).contiguous() for k in ("dout", "y", "mean", "invstd", "gamma", "partial")}
    before = dev["partial"].clone()
    for train in (1, 0):
        what = "C%d nblk%d train=%d" % (C, nblk, train)
        ref = [bwd_ref(t["dout"], t["y"], None, t["mean"], t["invstd"], t["gamma"], None, None, train, NONE, False, None, dt)
               for dt in (torch.float64, torch.float32)]
        dy, dgamma, dbeta = Guarded((M, C), device), Guarded((C,), device), Guarded((C,), device)
        _lib.check(lib.orbit_op_bn_backward_reduced(d(dev["dout"]), d(dev["y"]), d(dev["mean"]), d(dev["invstd"]), d(dev["gamma"]), train, M,
                                                    C, d(dev["partial"]), nblk, d(dy.t), d(dgamma.t), d(dbeta.t), _st()),
                   "orbit_op_bn_backward_reduced")
        torch.cuda.synchronize()
        bit_equal("exact_dgamma", "reduced " + what, dgamma.cpu("dgamma"), ref[0][2])
        bit_equal("exact_dbeta", "reduced " + what, dbeta.cpu("dbeta"), ref[0][3])
        _egate("exact_dy", "reduced " + what, dy.cpu("dy"), ref[0][0], ref[1][0])
    assert torch.equal(dev["partial"], before), "the caller's partials were modified"


# ---- g. the second and third grid trip of the streaming kernels ------------------------------------------------------------------------
GRID_STRIDE = 8192 * 256  # float4 elements per trip (grid_for caps the grid at 8192 blocks of 256 threads)
# name, M, C, stride_mod = GRID_STRIDE % (C / 4)
TRIP_CASES = {"apply": (470_000, 36, 8), "backward": (170_000, 100, 2)}


def test_apply_grid_stride_trips(lib, device):
    """scale_shift_act_kernel past its first grid trip: 4,230,000 float4 elements = two full trips and a partial third, the channel
    quad walked incrementally with stride_mod = 8 of C / 4 = 9."""
    M, C, _ = TRIP_CASES["apply"]
    y = y_input("gauss", M, C, 15)
    g = _gen(16)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    out = run_scale_shift_act(lib, device, y, scale, shift, None, SILU, 0)
    _egate("gauss_apply", "grid trips %dx%d silu" % (M, C), out, apply_ref(y, scale, shift, None, SILU, False, torch.float64),
           apply_ref(y, scale, shift, None, SILU, False, torch.float32))


def test_backward_grid_stride_trips(lib, device):
    """bn_bwd_apply_kernel past its first grid trip (4,250,000 float4 elements, stride_mod = 2 of C / 4 = 25): SiLU, train mode, dres
    written. Closed-form reference."""
    M, C, _ = TRIP_CASES["backward"]
    t = form_inputs(M, C, SILU, False, False)
    ref = [bwd_ref(t["dout"], t["y"], None, t["mean"], t["invstd"], t["gamma"], t["scale"], t["shift"], 1, SILU, False, None, dt)
           for dt in (torch.float64, torch.float32)]
    dy, dres, dgamma, dbeta = run_bn_backward_ex(lib, device, t, None, 1, SILU, 0, "write")
    what = "grid trips %dx%d silu train" % (M, C)
    _egate("gauss_dy", what, dy, ref[0][0], ref[1][0])
    _egate("gauss_dres", what, dres, ref[0][1], ref[1][1])
    check_sum_gate("gauss_dgamma", what, dgamma, ref[0][2], ref[1][2])
    check_sum_gate("gauss_dbeta", what, dbeta, ref[0][3], ref[1][3])
