"""The 197-token attention backward of csrc/vit.hip alone (orbit_op_vit_attention_bwd_tokens -> vit_attention197_bwd_kernel)
against torch float64 autograd of the four-line attention of tests/vit_pin.py on the same fp32 inputs, as
tests/test_gpu_vit_bwd_ops.py::test_attention_bwd does for 50 tokens; and the two shared backward kernels (data-gradient GEMM,
LayerNorm backward) at the row counts 197 tokens bring.

dqkv is NaN-filled before each call and followed by guard rows holding a sentinel; qkv and dout are followed by NaN rows, so a
read past token 196 of the last frame poisons the result. The gate is the one of tests/test_gpu_vit16_ops.py, unchanged:

    max |got - ref64|  <=  max(4 * e32, 8 * 2**-24 * max |ref64|)

with e32 the error against float64 of torch's fp32 CPU autograd on the same inputs, measured inside each case - on the whole
tensor and on the dq, dk and dv thirds each against their own scale. The kernel pads 197 tokens to 224: the one-hot dO cases at
token 191 (last row of a full tile) and 196 (the last valid token, inside the padded tile) and the dO = 1 on token 196 case over
uniform attention (dV = 1/197 in every row; a padded query that re-read query 196 would double it) are there for that.

Largest err / e32 seen on the MI355X (every case prints its ratio; run with -s):
  attention197_bwd   2.95  (dq, uniform keys, D = 768, B = 3: 5.7e-9 on a gradient that is exactly zero; dv 2.66, uniform, random dO;
                           dk 1.80, peaked, one-hot dO at token 191 - 4.25 with the scores in one 64-product chain)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from test_gpu_vit16_ops import ATTN_FAMILIES, GUARD, NAN, SENTINEL, T16, attention_inputs, gate  # noqa: E402
from test_gpu_vit_bwd_ops import dgrad_reference, ln_autograd, run_attention_bwd, run_dgrad, run_ln_bwd  # noqa: E402
from test_gpu_vit_ops import _prof_rows, attention_ref, layernorm_inputs  # noqa: E402

SHAPES = [(384, 6), (768, 12)]


def _st():
    return _lib.stream_handle()


def attention_grad(qkv, dout, heads, dtype):
    leaf = qkv.detach().to(dtype).clone().requires_grad_(True)
    attention_ref(leaf, heads).backward(dout.to(dtype))
    return leaf.grad


def run_bwd197(lib, device, qkv, dout, heads, tokens=T16):
    B, D = qkv.shape[0], heads * 64
    rows = B * tokens
    dqkv = torch.full((rows + GUARD, 3 * D), NAN, device=device)
    dqkv[rows:] = SENTINEL
    qd = torch.full((rows + GUARD, 3 * D), NAN, device=device)
    qd[:rows] = qkv.reshape(rows, 3 * D)
    dd = torch.full((rows + GUARD, D), NAN, device=device)
    dd[:rows] = dout.reshape(rows, D)
    rc = lib.orbit_op_vit_attention_bwd_tokens(_lib.dptr(qd), _lib.dptr(dd), _lib.dptr(dqkv), B, tokens, D, heads, _st())
    _lib.check(rc, "orbit_op_vit_attention_bwd_tokens")
    torch.cuda.synchronize()
    assert bool((dqkv[rows:] == SENTINEL).all()), "rows past B * %d were written" % tokens
    return dqkv[:rows].cpu().reshape(B, tokens, 3 * D)


def check_grad(got, qkv, dout, heads, what):
    """The gate on the whole of dqkv and on each third; returns ref64."""
    D = heads * 64
    ref64 = attention_grad(qkv, dout, heads, torch.float64)
    ref32 = attention_grad(qkv, dout, heads, torch.float32).double()
    gate(got, ref64, (ref32 - ref64).abs().max().item(), what)
    for j, name in enumerate("qkv"):
        sl = slice(j * D, (j + 1) * D)
        gate(got[..., sl], ref64[..., sl], (ref32[..., sl] - ref64[..., sl]).abs().max().item(), what + " d" + name)
    return ref64


def one_hot(B, D, token):
    hot = torch.zeros(B, T16, D)
    hot[B - 1, token, D - 59] = 1.0  # one element of the last head's output, in the last frame
    return hot


@pytest.mark.parametrize("family", ATTN_FAMILIES)
@pytest.mark.parametrize("D,heads", SHAPES)
def test_attention_bwd_197(lib, device, D, heads, family):
    for B in (1, 3):
        qkv = attention_inputs(B, heads, family, 2200 + D + B)
        g = torch.Generator().manual_seed(2300 + D + B)
        cases = [("random", torch.randn(B, T16, D, generator=g))] + [("one_hot@%d" % t, one_hot(B, D, t)) for t in (0, 191, 196)]
        for kind, dout in cases:
            what = "attention197_bwd D=%d %s B=%d dO %s" % (D, family, B, kind)
            got = run_bwd197(lib, device, qkv, dout, heads)
            check_grad(got, qkv, dout, heads, what)
            if kind != "random":  # only the last head of the last frame receives a gradient
                mask = torch.ones(B, T16, 3, heads, 64, dtype=torch.bool)
                mask[B - 1, :, :, heads - 1] = False
                assert bool((got.reshape(B, T16, 3, heads, 64)[mask] == 0).all()), what + ": a gradient leaked into another head or frame"


@pytest.mark.parametrize("D,heads", SHAPES)
def test_padded_queries_add_nothing(lib, device, D, heads):
    """Uniform attention (P = 1/197 in every row), dO = 1 on token 196 of the last frame and 0 elsewhere: dV = P^T dO is 1/197 in
    every row of that frame. Query 196 sits in the padded tile beside 27 phantom queries; were they to re-read it (as the forward's
    do, harmlessly) dV would be 2/197 or more."""
    B = 2
    qkv = attention_inputs(B, heads, "uniform", 2400 + D)
    dout = torch.zeros(B, T16, D)
    dout[B - 1, T16 - 1] = 1.0
    got = run_bwd197(lib, device, qkv, dout, heads)
    ref64 = check_grad(got, qkv, dout, heads, "attention197_bwd D=%d uniform dO = 1 on token 196" % D)
    dv64 = ref64[..., 2 * D:]
    assert (dv64[B - 1] - 1.0 / 197).abs().max().item() < 1e-12 and bool((dv64[0] == 0).all())
    assert (got[B - 1, :, 2 * D:] - 1.0 / 197).abs().max().item() < 1e-8
    assert bool((got[0] == 0).all())


@pytest.mark.parametrize("D,heads", SHAPES)
def test_repeatable_and_independent_of_the_batch(lib, device, D, heads):
    qkv = attention_inputs(3, heads, "gaussian", 2500 + D)
    dout = torch.randn(3, T16, D, generator=torch.Generator().manual_seed(2600 + D))
    a = run_bwd197(lib, device, qkv, dout, heads)
    b = run_bwd197(lib, device, qkv, dout, heads)
    assert torch.equal(a, b), "two runs differ"
    for f in range(3):
        one = run_bwd197(lib, device, qkv[f:f + 1], dout[f:f + 1], heads)
        assert torch.equal(one[0], a[f]), "frame %d depends on the frames that share its launch" % f


@pytest.mark.parametrize("D,heads", SHAPES)
def test_the_two_entries(lib, device, D, heads):
    """tokens = 50 through the new entry is the existing kernel, bit for bit and by its profiler row; 197 is the new one."""
    qkv = attention_inputs(3, heads, "gaussian", 2700 + D, tokens=50)
    g = torch.Generator().manual_seed(2800 + D)
    dout = torch.randn(3, 50, D, generator=g)
    lib.orbit_prof_enable(1)
    try:
        new = run_bwd197(lib, device, qkv, dout, heads, tokens=50)
        old = run_attention_bwd(lib, device, qkv, dout, heads)
        rows = {k: n for k, n in _prof_rows(lib).items() if k.startswith("vit_")}
    finally:
        lib.orbit_prof_enable(0)
    assert rows == {"vit_attention_bwd": 2}, rows
    assert torch.equal(new, old)
    qkv = attention_inputs(1, heads, "gaussian", 2900 + D)
    dout = torch.randn(1, T16, D, generator=g)
    lib.orbit_prof_enable(1)
    try:
        run_bwd197(lib, device, qkv, dout, heads)
        rows = {k: n for k, n in _prof_rows(lib).items() if k.startswith("vit_")}
    finally:
        lib.orbit_prof_enable(0)
    assert rows == {"vit_attention197_bwd": 1}, rows


def test_other_token_counts_are_refused_on_the_device(lib, device):
    dqkv = torch.full((4 * 224, 3 * 384), SENTINEL, device=device)
    qkv = torch.zeros(4 * 224, 3 * 384, device=device)
    dout = torch.zeros(4 * 224, 384, device=device)
    lib.orbit_prof_enable(1)
    try:
        for tokens in (49, 196, 198, 224):
            rc = lib.orbit_op_vit_attention_bwd_tokens(_lib.dptr(qkv), _lib.dptr(dout), _lib.dptr(dqkv), 1, tokens, 384, 6, _st())
            assert rc == -1 and "tokens" in _lib.last_error()
        assert not any(_prof_rows(lib).values()), "a refused call launched something"
    finally:
        lib.orbit_prof_enable(0)
    torch.cuda.synchronize()
    assert bool((dqkv == SENTINEL).all())


# ---- the shared backward kernels at 197-token row counts (coverage: they pass without the 197-token backward) -----------
@pytest.mark.parametrize("epilogue", ["plain", "gelu"])
def test_linear_dgrad_at_197_token_rows(lib, device, epilogue):
    """One 384-wide layer (fc1's data gradient: dy [M][1536] . w [1536][384]) at M = 197 and 591 = 3 * 197 - tails of 5 and 15 rows
    against 64-row tiles, 69 and 79 against 128 - at both tile heights."""
    K, N, M_MAX = 384, 1536, 591
    g = torch.Generator().manual_seed(3000)
    dy = torch.randn(M_MAX, N, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    u = torch.randn(M_MAX, K, generator=g) if epilogue == "gelu" else None
    ref64 = dgrad_reference(dy, w, u, None, torch.float64)
    ref32 = dgrad_reference(dy, w, u, None, torch.float32)
    wd, dyd = w.to(device), dy.to(device)
    ud = None if u is None else u.to(device)
    wt = torch.empty(K, N, device=device)
    out = {}
    for M in (197, M_MAX):
        e32 = (ref32[:M].double() - ref64[:M]).abs().max().item()
        for tile in (64, 128):
            out[M, tile] = run_dgrad(lib, device, dyd, wd, wt, ud, None, M, tile, in_place=True)
            gate(out[M, tile], ref64[:M], e32, "dgrad %dx%d %s M=%d tile=%d" % (N, K, epilogue, M, tile))
    for (M, tile), got in out.items():
        assert torch.equal(got, out[M_MAX, 64][:M]), "rows depend on M or on the tile height (M=%d, tile=%d)" % (M, tile)


@pytest.mark.parametrize("D", [384, 768])
def test_layernorm_bwd_at_197_rows(lib, device, D):
    rows, eps = 197, 1e-6  # 4 blocks of 64 rows with a 5-row tail
    x, gamma, beta = layernorm_inputs(D, rows, "normal", 3100 + D)
    dy = torch.randn(rows, D, generator=torch.Generator().manual_seed(3200 + D))
    dx64, dg64, db64 = ln_autograd(x, dy, gamma, beta, eps, torch.float64)
    e_dx = e_dg = e_db = 0.0
    gp = torch.Generator().manual_seed(rows + D)
    for t in range(4):  # the fp32 yardstick in 4 row / channel orders, as tests/test_gpu_vit_bwd_ops.py
        pr = torch.arange(rows) if t == 0 else torch.randperm(rows, generator=gp)
        pc = torch.arange(D) if t == 0 else torch.randperm(D, generator=gp)
        a, b, c = ln_autograd(x[pr][:, pc].contiguous(), dy[pr][:, pc].contiguous(), gamma[pc], beta[pc], eps, torch.float32)
        e_dx = max(e_dx, (a.double() - dx64[pr][:, pc]).abs().max().item())
        e_dg = max(e_dg, (b.double() - dg64[pc]).abs().max().item())
        e_db = max(e_db, (c.double() - db64[pc]).abs().max().item())
    dx, dg, db = run_ln_bwd(lib, device, x.to(device), dy.to(device), gamma.to(device), eps, "plain")
    gate(dx, dx64, e_dx, "layernorm_bwd D=%d rows=197 dx" % D)
    gate(dg, dg64, e_dg, "layernorm_bwd D=%d rows=197 dgamma" % D)
    gate(db, db64, e_db, "layernorm_bwd D=%d rows=197 dbeta" % D)
