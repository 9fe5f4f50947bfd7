"""The weight-gradient kernels of csrc/vit.hip one by one (orbit_op_vit_linear_wgrad, orbit_op_vit_patch_embed_bwd) against a
float64 CPU evaluation of the same operation on the same fp32 inputs.

Gate (tests/test_gpu_vit_ops.py): max |got - ref64| <= max(4 * e32, 8 * 2**-24 * max |ref64|). e32 is measured on the reference
side only: the error against float64 of the same computation in fp32 on the CPU - torch's `dy.t() @ x` (a blocked sgemm) for the
filter gradient, `dy.sum(0)` for the bias gradient, fp32 autograd of F.conv2d(stride=32) + pos_embed + cls_token for the patch
embedding. Inputs are followed by 128 NaN guard rows (rows past M must contribute exactly zero: they are summed here, so a
clamped re-read or a 0 * NaN shows up in every output); outputs and the workspace are NaN-filled with sentinel tails.

Row counts: 1 .. 3350 around the 32-row step and the 128-row tile, plus the two values on either side of every change of the
split count below 3350 rows - the rule (wgrad_splits) doubles the count at M = 225, 481, 993 and 2017.

Largest err / e32 seen on the MI355X (every case prints its ratio; run with -s):
  filter gradient  2.36  (384x1536 one_sign with GELU on load, M = 224)
  bias gradient    1.75  (128x32 normal, M = 63)
  additivity       1.28  (|whole - sum of three parts| / e32, 1152x384 dbias)
  patch embedding  2.46 dw, 1.06 dbias, 1.00 dpos / dcls  (B = 3, D = 384)
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from test_gpu_vit_ops import GUARD, NAN, SENTINEL, U, gate, linear_inputs  # noqa: E402
from orbit_dataset_amd import _lib  # noqa: E402

SHAPES = [(128, 32), (1152, 384), (384, 1536), (1536, 384)]  # (N, K): one tile; the ViT-S/32 qkv, fc2 and fc1 layers
SPLIT_EDGES = (224, 225, 480, 481, 992, 993, 2016, 2017)   # either side of every change of the split count below 3350 rows
M_BIG = 3350
M_SWEEP = tuple(sorted({1, 50, 63, 64, 65, 150, M_BIG} | set(SPLIT_EDGES)))
TAIL = 4096  # sentinel floats behind dw / dbias / the workspace


def _guarded(rows, M, device):
    """the first M rows on the device, followed by 128 NaN rows"""
    out = torch.full((M + GUARD, rows.shape[1]), NAN, device=device)
    out[:M] = rows[:M]
    return out


def _tailed(n, device):
    t = torch.full((n + TAIL,), NAN, device=device)
    t[n:] = SENTINEL
    return t


def run_wgrad(lib, device, dy, x, M, gelu, with_bias):
    """orbit_op_vit_linear_wgrad on the first M rows of the CPU tensors dy [.][N] / x [.][K]: (dw [N][K], dbias [N] or None) on
    the device after the sentinel checks."""
    N, K = dy.shape[1], x.shape[1]
    dyp, xp = _guarded(dy, M, device), _guarded(x, M, device)
    need = lib.orbit_op_vit_linear_wgrad_workspace_floats(M, N, K)
    dw, db, ws = _tailed(N * K, device), _tailed(N, device) if with_bias else None, _tailed(need, device)
    _lib.check(lib.orbit_op_vit_linear_wgrad(_lib.dptr(dyp), _lib.dptr(xp), _lib.dptr(dw), _lib.dptr(db), M, N, K, int(gelu),
                                             _lib.dptr(ws), need, _lib.stream_handle()), "orbit_op_vit_linear_wgrad")
    torch.cuda.synchronize()
    for name, t, n in (("dw", dw, N * K), ("dbias", db, N), ("workspace", ws, need)):
        assert t is None or bool((t[n:] == SENTINEL).all()), "%s: written past its end (M=%d N=%d K=%d)" % (name, M, N, K)
    return dw[:N * K].view(N, K), None if db is None else db[:N]


@pytest.mark.parametrize("family", ["normal", "one_sign"])
@pytest.mark.parametrize("N,K", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_linear_wgrad_every_row_count(lib, device, N, K, family):
    x, _, _, dy = linear_inputs(K, N, M_BIG, family, 300 + N + K)
    for gelu in (0, 1):
        xg64, xg32 = (F.gelu(x.double()), F.gelu(x)) if gelu else (x.double(), x)
        ref64, refb, prev = torch.zeros(N, K, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), 0
        for M in M_SWEEP:
            # float64 references over the first M rows, accumulated over the sweep (float64 addition: 2**-53 per step)
            ref64 = ref64 + dy[prev:M].double().t() @ xg64[prev:M]
            refb = refb + dy[prev:M].double().sum(0)
            prev = M
            e32 = ((dy[:M].t() @ xg32[:M]).double() - ref64).abs().max().item()
            e32b = (dy[:M].sum(0).double() - refb).abs().max().item()
            what = "wgrad %dx%d %s gelu=%d M=%d" % (N, K, family, gelu, M)
            dw, db = run_wgrad(lib, device, dy, x, M, gelu, True)
            gate(dw.cpu(), ref64, e32, what + " dw")
            gate(db.cpu(), refb, e32b, what + " dbias")
            dw0, none = run_wgrad(lib, device, dy, x, M, gelu, False)
            assert none is None and torch.equal(dw0, dw), what + ": dw depends on whether dbias is asked for"
            dw2, db2 = run_wgrad(lib, device, dy, x, M, gelu, True)
            assert torch.equal(dw2, dw) and torch.equal(db2, db), what + ": two runs differ"


@pytest.mark.parametrize("N,K", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_linear_wgrad_adds_over_a_partition_of_the_rows(lib, device, N, K):
    """dW over 3350 rows = the float64 sum of dW over [0, 993), [993, 2017) and [2017, 3350) (8, 8 and 8 or fewer splits against
    16): both sides are within the gate of the float64 gradient, and of each other."""
    x, _, _, dy = linear_inputs(K, N, M_BIG, "one_sign", 300 + N + K)
    ref64, refb = dy.double().t() @ x.double(), dy.double().sum(0)
    e32 = ((dy.t() @ x).double() - ref64).abs().max().item()
    e32b = (dy.sum(0).double() - refb).abs().max().item()
    dw, db = run_wgrad(lib, device, dy, x, M_BIG, 0, True)
    sw, sb = torch.zeros_like(ref64), torch.zeros_like(refb)
    for a, b in ((0, 993), (993, 2017), (2017, M_BIG)):
        pw, pb = run_wgrad(lib, device, dy[a:b], x[a:b], b - a, 0, True)
        sw, sb = sw + pw.cpu().double(), sb + pb.cpu().double()
    gate(sw.float(), ref64, e32, "wgrad %dx%d additivity dw (sum of 3 parts)" % (N, K))
    gate(sb.float(), refb, e32b, "wgrad %dx%d additivity dbias (sum of 3 parts)" % (N, K))
    for got, summed, ref, e in ((dw, sw, ref64, e32), (db, sb, refb, e32b)):
        tol = max(4 * e, 8 * U * ref.abs().max().item())
        diff = (got.cpu().double() - summed).abs().max().item()
        print("[vit-wgrad] additivity %dx%d: |whole - sum of parts| %.3g  e32 %.3g  ratio %.2f" % (N, K, diff, e, diff / e))
        assert diff <= tol


def _patch_case(B, D, bias):
    g = torch.Generator().manual_seed(500 + B + D)
    frames = torch.randn(B, 3, 224, 224, generator=g)
    dtok = torch.randn(B, 50, D, generator=g)
    w = torch.randn(D, 3, 32, 32, generator=g) / 3072 ** 0.5
    params = {"w": w, "pos": 0.1 * torch.randn(1, 50, D, generator=g), "cls": 0.1 * torch.randn(1, 1, D, generator=g)}
    if bias:
        params["b"] = 0.1 * torch.randn(D, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
        tok = F.conv2d(frames.to(dtype), q["w"], q.get("b"), stride=32).flatten(2).transpose(1, 2)
        tok = torch.cat([q["cls"].expand(B, -1, -1), tok], dim=1) + q["pos"]
        (tok * dtok.to(dtype)).sum().backward()
        ref[dtype] = {k: v.grad.double() for k, v in q.items()}
    e32 = {k: (ref[torch.float32][k] - v).abs().max().item() for k, v in ref[torch.float64].items()}
    return frames, dtok, ref[torch.float64], e32


@pytest.mark.parametrize("B,D,bias", [(1, 384, True), (3, 384, True), (1, 768, False)], ids=["B1-D384", "B3-D384", "B1-D768-clip"])
def test_patch_embed_bwd(lib, device, B, D, bias):
    frames, dtok, ref64, e32 = _patch_case(B, D, bias)
    fr = torch.full((B + 1, 3, 224, 224), NAN, device=device)  # one NaN guard frame
    fr[:B] = frames
    dt = _guarded(dtok.reshape(B * 50, D), B * 50, device)
    need = lib.orbit_op_vit_linear_wgrad_workspace_floats(49 * B, D, 3072)
    runs = []
    for _ in range(2):
        dw, db, ws = _tailed(D * 3072, device), _tailed(D, device) if bias else None, _tailed(need, device)
        dpos, dcls = _tailed(50 * D, device), _tailed(D, device)
        _lib.check(lib.orbit_op_vit_patch_embed_bwd(_lib.dptr(fr), _lib.dptr(dt), _lib.dptr(dw), _lib.dptr(db), _lib.dptr(dpos),
                                                    _lib.dptr(dcls), B, D, _lib.dptr(ws), need, _lib.stream_handle()),
                   "orbit_op_vit_patch_embed_bwd")
        torch.cuda.synchronize()
        for name, t, n in (("dw", dw, D * 3072), ("dbias", db, D), ("dpos", dpos, 50 * D), ("dcls", dcls, D), ("workspace", ws, need)):
            assert t is None or bool((t[n:] == SENTINEL).all()), name + ": written past its end"
        runs.append((dw[:D * 3072].cpu(), None if db is None else db[:D].cpu(), dpos[:50 * D].cpu(), dcls[:D].cpu()))
    dw, db, dpos, dcls = runs[0]
    what = "patch_embed_bwd B=%d D=%d " % (B, D)
    gate(dw.view(D, 3, 32, 32), ref64["w"], e32["w"], what + "dw")
    if bias:
        gate(db, ref64["b"], e32["b"], what + "dbias")
    gate(dpos.view(1, 50, D), ref64["pos"], e32["pos"], what + "dpos")
    gate(dcls.view(1, 1, D), ref64["cls"], e32["cls"], what + "dcls")
    assert all(a is None and b is None or torch.equal(a, b) for a, b in zip(*runs)), what + "two runs differ"
