"""The backward kernels of csrc/vit.hip one by one (orbit_op_vit_linear_dgrad / _layernorm_bwd / _attention_bwd) against torch
float64 autograd of the same operation on the same fp32 inputs (F.linear, F.gelu, F.layer_norm, the four-line attention of
tests/vit_pin.py).

Outputs are NaN-filled before each call and followed by guard rows holding a sentinel, as in tests/test_gpu_vit_ops.py, whose
gate is used unchanged:

    max |got - ref64|  <=  max(4 * e32, 8 * 2**-24 * max |ref64|)

e32 is the error against float64 of the fp32 CPU torch autograd evaluation of the same quantity, measured inside each case (for
LayerNorm in 4 row and channel orders: dgamma / dbeta are sums over the rows, and a row's error at mean >> std is one draw).

Largest err / e32 seen on the MI355X (every case prints its ratio; run with -s):
  linear_dgrad    2.03  (384x384 times GELU', exact zeros in u, M = 129)
  layernorm_bwd   dx 1.57, dgamma 2.22 (one row), dbeta 1.18
  attention_bwd   2.02  (dk, a 1e6 entry in V, one-hot dO)
(torch's cache-blocked sgemm is the yardstick of the GEMM cases; a single k-ordered chain over K = 1152 reached 4.12, which is
why the data-gradient instantiations of vit_gemm_kernel fold their accumulator every 256 k.)
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from test_gpu_vit_ops import (ATTN_FAMILIES, GUARD, LAYER_IDS, LAYERS, NAN, SENTINEL, TILES, attention_inputs,  # noqa: E402
                              attention_ref, gate, layernorm_inputs)

M_MAX = 275
MS = (1, 50, 129, 275)
EPILOGUES = ("plain", "accumulate", "gelu")


def _st():
    return _lib.stream_handle()


# ---- data-gradient GEMM ----------------------------------------------------------------------------------------------
def dgrad_reference(dy, w, u, res, dtype):
    """dx of rows of dy in `dtype` by torch autograd: dy . w, times GELU'(u) through F.gelu, or + residual."""
    dy, w = dy.to(dtype), w.to(dtype)
    if u is not None:
        leaf = u.detach().to(dtype).clone().requires_grad_(True)
        F.linear(F.gelu(leaf), w).backward(dy)
        return leaf.grad
    leaf = torch.zeros(dy.shape[0], w.shape[1], dtype=dtype, requires_grad=True)
    F.linear(leaf, w).backward(dy)
    return leaf.grad if res is None else res.to(dtype) + leaf.grad


def u_family(M, K, family, g):
    u = torch.randn(M, K, generator=g)
    if family == "wide":      # |u| up to 6: both tails of Phi, where 1 + erf cancels
        u = 12.0 * torch.rand(M, K, generator=g) - 6.0
        u[0, 0], u[-1, -1] = 6.0, -6.0
    elif family == "zeros":   # exact zeros: GELU'(0) = 1/2
        u[torch.rand(M, K, generator=g) < 0.25] = 0.0
        u[0, 0] = 0.0
    return u


def run_dgrad(lib, device, dy, w, wt, u, res, M, tile, in_place):
    N, K = w.shape
    dyp = torch.full((M + GUARD, N), NAN, device=device)
    dyp[:M] = dy[:M]
    dx = torch.full((M + GUARD, K), NAN, device=device)
    dx[M:] = SENTINEL
    up = rp = None
    if u is not None:
        up = torch.full((M + GUARD, K), NAN, device=device)
        up[:M] = u[:M]
    if res is not None:
        if in_place:
            dx[:M] = res[:M]
            rp = dx
        else:
            rp = torch.zeros(M + GUARD, K, device=device)
            rp[:M] = res[:M]
    wt.fill_(NAN)
    rc = lib.orbit_op_vit_linear_dgrad(_lib.dptr(dyp), _lib.dptr(w), _lib.dptr(wt), _lib.dptr(up), _lib.dptr(rp), _lib.dptr(dx),
                                       M, N, K, tile, _st())
    _lib.check(rc, "orbit_op_vit_linear_dgrad")
    torch.cuda.synchronize()
    assert bool((dx[M:] == SENTINEL).all()), "rows past M were written (M=%d N=%d K=%d tile=%d)" % (M, N, K, tile)
    return dx[:M].cpu()


@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("K,N,_epi", LAYERS, ids=LAYER_IDS)
def test_linear_dgrad(lib, device, K, N, _epi, epilogue):
    """dx [M][K] = dy [M][N] . w [N][K] for the eight layer shapes, M = 1, 50, 129, 275 at both tile heights; plain, accumulated
    in place into a residual-gradient stream, and times GELU'(u) for three families of u. Rows are bitwise the same whatever M
    and the tile height."""
    g = torch.Generator().manual_seed(900 + K + N)
    dy = torch.randn(M_MAX, N, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    res = torch.randn(M_MAX, K, generator=g) if epilogue == "accumulate" else None
    wd, dyd = w.to(device), dy.to(device)
    wt = torch.empty(K, N, device=device)
    for fam in (("normal", "wide", "zeros") if epilogue == "gelu" else (None,)):
        u = u_family(M_MAX, K, fam, g) if fam else None
        ref64 = dgrad_reference(dy, w, u, res, torch.float64)
        ref32 = dgrad_reference(dy, w, u, res, torch.float32)
        ud = None if u is None else u.to(device)
        rd = None if res is None else res.to(device)
        out = {}
        for M in MS:
            e32 = (ref32[:M].double() - ref64[:M]).abs().max().item()
            for tile in TILES:
                got = run_dgrad(lib, device, dyd, wd, wt, ud, rd, M, tile, in_place=True)
                gate(got, ref64[:M], e32, "dgrad %dx%d %s%s M=%d tile=%d" % (N, K, epilogue, "-" + fam if fam else "", M, tile))
                out[M, tile] = got
        assert torch.equal(wt.cpu(), w.t()), "wt_scratch is not the transposed weight"
        for (M, tile), got in out.items():
            assert torch.equal(got, out[M_MAX, 64][:M]), "rows depend on M or on the tile height (M=%d, tile=%d)" % (M, tile)


# ---- LayerNorm backward ----------------------------------------------------------------------------------------------
LNB_ROWS = (1, 50, 257, 1031)  # blocks hold 64 rows: a partial block, 5 blocks with a 1-row tail, 17 with a 7-row tail
LNB_FAMILIES = ("normal", "offset", "near_constant", "constant", "outlier")


def ln_autograd(x, dy, gamma, beta, eps, dtype):
    xl, gl, bl = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    F.layer_norm(xl, (x.shape[1],), gl, bl, eps).backward(dy.to(dtype))
    return xl.grad, gl.grad, bl.grad


def run_ln_bwd(lib, device, x, dy, gamma, eps, form, res=None):
    """form: 'plain', 'residual' (dres aliasing dx), 'no_dx', 'strided' (x and dx rows at stride 50 D: token 0 of every frame)."""
    rows, D = x.shape
    tail = 2 * D
    dg = torch.full((D + tail,), NAN, device=device)
    db = torch.full((D + tail,), NAN, device=device)
    dg[D:], db[D:] = SENTINEL, SENTINEL
    nblk = -(-rows // 64)
    partial = torch.full((nblk * 2 * D + tail,), NAN, device=device)
    partial[nblk * 2 * D:] = SENTINEL
    dyp = torch.full((rows + GUARD, D), NAN, device=device)
    dyp[:rows] = dy
    dx = dres = None
    if form == "strided":
        xb = torch.full((rows, 50, D), NAN, device=device)
        xb[:, 0] = x
        xs = dxs = 50 * D
        dx = torch.full((rows + 1, 50, D), NAN, device=device)
        dx[rows:] = SENTINEL
    else:
        xb = torch.full((rows + GUARD, D), NAN, device=device)
        xb[:rows] = x
        xs = dxs = D
        if form != "no_dx":
            dx = torch.full((rows + GUARD, D), NAN, device=device)
            dx[rows:] = SENTINEL
        if form == "residual":
            dx[:rows] = res
            dres = dx
    rc = lib.orbit_op_vit_layernorm_bwd(_lib.dptr(xb), xs, _lib.dptr(dyp), D, _lib.dptr(gamma), eps, _lib.dptr(dres),
                                        _lib.dptr(dx), dxs, rows, D, _lib.dptr(dg), _lib.dptr(db), _lib.dptr(partial),
                                        nblk * 2 * D, _st())
    _lib.check(rc, "orbit_op_vit_layernorm_bwd")
    torch.cuda.synchronize()
    for t, n in ((dg, D), (db, D), (partial, nblk * 2 * D)):
        assert bool((t[n:] == SENTINEL).all()), "floats past the end of dgamma / dbeta / partial were written (%s)" % form
    if dx is not None:
        assert bool((dx[rows:] == SENTINEL).all()), "rows past the last were written (rows=%d, %s)" % (rows, form)
    if form == "strided":
        assert bool((dx[:rows, 1:] == 0).all()), "token rows 1..49 of the gradient stream are not exactly zero"
        dx = dx[:rows, 0]
    return (None if dx is None else dx[:rows].cpu()), dg[:D].cpu(), db[:D].cpu()


@pytest.mark.parametrize("family", LNB_FAMILIES)
@pytest.mark.parametrize("D", [384, 768])
def test_layernorm_bwd(lib, device, D, family):
    x, gamma, beta = layernorm_inputs(D, max(LNB_ROWS), family, 1000 + D)
    g = torch.Generator().manual_seed(1100 + D)
    dy = torch.randn(max(LNB_ROWS), D, generator=g)
    res = torch.randn(max(LNB_ROWS), D, generator=g)
    gd = gamma.to(device)
    for eps in (1e-6, 1e-5):
        for rows in LNB_ROWS:
            xr, dyr, rr = x[:rows], dy[:rows], res[:rows]
            dx64, dg64, db64 = ln_autograd(xr, dyr, gamma, beta, eps, torch.float64)
            # the fp32 yardstick in 4 row / channel orders (LayerNorm is equivariant under both)
            e_dx = e_dg = e_db = e_res = 0.0
            gp = torch.Generator().manual_seed(rows + D)
            for t in range(4):
                pr = torch.arange(rows) if t == 0 else torch.randperm(rows, generator=gp)
                pc = torch.arange(D) if t == 0 else torch.randperm(D, generator=gp)
                a, b, c = ln_autograd(xr[pr][:, pc].contiguous(), dyr[pr][:, pc].contiguous(), gamma[pc], beta[pc], eps,
                                      torch.float32)
                e_dx = max(e_dx, (a.double() - dx64[pr][:, pc]).abs().max().item())
                e_res = max(e_res, ((a + rr[pr][:, pc]).double() - (dx64 + rr.double())[pr][:, pc]).abs().max().item())
                e_dg = max(e_dg, (b.double() - dg64[pc]).abs().max().item())
                e_db = max(e_db, (c.double() - db64[pc]).abs().max().item())
            xd, dyd = xr.to(device), dyr.to(device)
            what = "layernorm_bwd D=%d %s eps=%g rows=%d " % (D, family, eps, rows)
            forms = ("plain", "residual", "no_dx") + (("strided",) if rows <= 257 else ())
            first = None
            for form in forms:
                dx, dg, db = run_ln_bwd(lib, device, xd, dyd, gd, eps, form, rr.to(device))
                if form == "residual":
                    gate(dx, dx64 + rr.double(), e_res, what + "residual dx")
                elif form == "no_dx":
                    assert dx is None
                else:
                    gate(dx, dx64, e_dx, what + form + " dx")
                gate(dg, dg64, e_dg, what + form + " dgamma")
                gate(db, db64, e_db, what + form + " dbeta")
                if form == "plain":
                    first = (dx, dg, db)
                else:  # the sums do not depend on the form
                    assert torch.equal(dg, first[1]) and torch.equal(db, first[2])
            again = run_ln_bwd(lib, device, xd, dyd, gd, eps, "plain")
            assert all(torch.equal(p, q) for p, q in zip(first, again)), "two runs differ"


# ---- attention backward ----------------------------------------------------------------------------------------------
def attention_grad(qkv, dout, heads, dtype):
    leaf = qkv.detach().to(dtype).clone().requires_grad_(True)
    attention_ref(leaf, heads).backward(dout.to(dtype))
    return leaf.grad


def run_attention_bwd(lib, device, qkv, dout, heads):
    B, D = qkv.shape[0], heads * 64
    dqkv = torch.full((B * 50 + GUARD, 3 * D), NAN, device=device)
    dqkv[B * 50:] = SENTINEL
    qd, dd = qkv.to(device), dout.to(device)
    rc = lib.orbit_op_vit_attention_bwd(_lib.dptr(qd), _lib.dptr(dd), _lib.dptr(dqkv), B, D, heads, _st())
    _lib.check(rc, "orbit_op_vit_attention_bwd")
    torch.cuda.synchronize()
    assert bool((dqkv[B * 50:] == SENTINEL).all()), "rows past B * 50 were written"
    return dqkv[:B * 50].cpu().reshape(B, 50, 3 * D)


@pytest.mark.parametrize("family", ATTN_FAMILIES)
@pytest.mark.parametrize("D,heads", [(384, 6), (768, 12)])
def test_attention_bwd(lib, device, D, heads, family):
    for B in (1, 3):
        qkv = attention_inputs(B, heads, family, 1200 + D + B)
        g = torch.Generator().manual_seed(1300 + D + B)
        hot = torch.zeros(B, 50, D)
        hot[B - 1, 23, D - 59] = 1.0  # one element of the last head's output
        for kind, dout in (("random", torch.randn(B, 50, D, generator=g)), ("one_hot", hot)):
            ref64 = attention_grad(qkv, dout, heads, torch.float64)
            ref32 = attention_grad(qkv, dout, heads, torch.float32).double()
            e32 = (ref32 - ref64).abs().max().item()
            got = run_attention_bwd(lib, device, qkv, dout, heads)
            gate(got, ref64, e32, "attention_bwd D=%d %s B=%d dO %s" % (D, family, B, kind))
            # q, k and v gradients each against their own scale as well (dv is O(1) where dq, dk can be tiny)
            for j, name in enumerate("qkv"):
                sl = slice(j * D, (j + 1) * D)
                e = (ref32[..., sl] - ref64[..., sl]).abs().max().item()
                gate(got[..., sl], ref64[..., sl], e, "attention_bwd D=%d %s B=%d dO %s d%s" % (D, family, B, kind, name))
            if kind == "one_hot":  # only the last head of the last frame receives a gradient
                mask = torch.ones(B, 50, 3, heads, 64, dtype=torch.bool)
                mask[B - 1, :, :, heads - 1] = False
                assert bool((got.reshape(B, 50, 3, heads, 64)[mask] == 0).all()), "a gradient leaked into another head or frame"
