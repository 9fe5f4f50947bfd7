"""The weight-gradient kernels the patch-16 transformers add or feed with new shapes, one by one: orbit_op_vit_patch_embed_bwd_p
at patch = 16 (vit_wgrad_kernel<WX_PATCH16> + vit_token_bwd_kernel at 197 tokens) against float64 autograd of
F.conv2d(stride=16) + pos_embed + cls_token on the same fp32 inputs, and orbit_op_vit_linear_wgrad at the 197-token row counts
(existing code at the row counts the new path feeds it), as tests/test_gpu_vit_wgrad_ops.py for the patch-32 models.

Gate (tests/test_gpu_vit_ops.py): max |got - ref64| <= max(4 * e32, 8 * 2**-24 * max |ref64|). e32 is measured on the reference
side only: the same computation in fp32 on the CPU against float64.

Patch cases: D = 384 with bias at B = 1, 2, 3, 6 and D = 768 without (the CLIP form) at B = 2. M = 196 B = 196, 392, 588 and
1176 patch rows are 1, 2, 4 and 8 splits under wgrad_splits (asserted from the workspace size), and none is a multiple of the
32-row step: the zero-filled tail rows take part in every case. frames and dtokens are followed by NaN guard rows, outputs and
the workspace are NaN-filled with sentinel tails, and token row 0 of every frame of dtokens (the class token's gradient, which
belongs to dpos / dcls alone) is about 1000: one such row read into dw or dbias is hundreds of gates.

Largest err / e32 seen on the MI355X (every case prints its ratio; run with -s):
  patch embedding  1.01 dw (B = 2, D = 384), 1.21 dbias (B = 1), 1.00 dpos / dcls (the fp32 reference's own sums)
  linear wgrad     1.90 dw (384x1536 one_sign with GELU on load and 1152x384 one_sign, M = 197), dbias below that
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from test_gpu_vit_ops import NAN, SENTINEL, gate, linear_inputs  # noqa: E402
from test_gpu_vit_wgrad_ops import _guarded, _tailed, run_wgrad  # noqa: E402
from orbit_dataset_amd import _lib  # noqa: E402

TOKENS, PATCHES, KPATCH = 197, 196, 768
PATCH_CASES = [(1, 384, True, 1), (2, 384, True, 2), (3, 384, True, 4), (6, 384, True, 8), (2, 768, False, 2)]
_CASES = {}


def _patch_case(B, D, bias):
    """fp32 inputs and the float64 gradients of sum(tokens * dtokens), with the fp32 CPU autograd's error per output; once."""
    if (B, D, bias) not in _CASES:
        g = torch.Generator().manual_seed(1600 + B + D)
        frames = torch.randn(B, 3, 224, 224, generator=g)
        dtok = torch.randn(B, TOKENS, D, generator=g)
        dtok[:, 0] = 1000.0 * (1 + 0.1 * torch.randn(B, D, generator=g))
        w = torch.randn(D, 3, 16, 16, generator=g) / KPATCH ** 0.5
        params = {"w": w, "pos": 0.1 * torch.randn(1, TOKENS, D, generator=g), "cls": 0.1 * torch.randn(1, 1, D, generator=g)}
        if bias:
            params["b"] = 0.1 * torch.randn(D, generator=g)
        ref = {}
        for dtype in (torch.float64, torch.float32):
            q = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
            tok = F.conv2d(frames.to(dtype), q["w"], q.get("b"), stride=16).flatten(2).transpose(1, 2)
            tok = torch.cat([q["cls"].expand(B, -1, -1), tok], dim=1) + q["pos"]
            (tok * dtok.to(dtype)).sum().backward()
            ref[dtype] = {k: v.grad.double() for k, v in q.items()}
            # the position table's row 0 (the large class-token gradient) apart from its patch rows: each under its own scale
            ref[dtype]["pos0"], ref[dtype]["pos"] = ref[dtype]["pos"][:, :1], ref[dtype]["pos"][:, 1:]
        e32 = {k: (ref[torch.float32][k] - v).abs().max().item() for k, v in ref[torch.float64].items()}
        _CASES[(B, D, bias)] = (frames, dtok, ref[torch.float64], e32)
    return _CASES[(B, D, bias)]


def _run_patch16(lib, device, frames, dtok, D, with_bias):
    B = frames.shape[0]
    fr = torch.full((B + 1, 3, 224, 224), NAN, device=device)  # one NaN guard frame
    fr[:B] = frames
    dt = _guarded(dtok.reshape(B * TOKENS, D), B * TOKENS, device)
    need = lib.orbit_op_vit_linear_wgrad_workspace_floats(PATCHES * B, D, KPATCH)
    dw, db, ws = _tailed(D * KPATCH, device), _tailed(D, device) if with_bias else None, _tailed(need, device)
    dpos, dcls = _tailed(TOKENS * D, device), _tailed(D, device)
    _lib.check(lib.orbit_op_vit_patch_embed_bwd_p(_lib.dptr(fr), _lib.dptr(dt), _lib.dptr(dw), _lib.dptr(db), _lib.dptr(dpos),
                                                  _lib.dptr(dcls), B, D, 16, _lib.dptr(ws), need, _lib.stream_handle()),
               "orbit_op_vit_patch_embed_bwd_p")
    torch.cuda.synchronize()
    for name, t, n in (("dw", dw, D * KPATCH), ("dbias", db, D), ("dpos", dpos, TOKENS * D), ("dcls", dcls, D),
                       ("workspace", ws, need)):
        assert t is None or bool((t[n:] == SENTINEL).all()), name + ": written past its end"
    return dw[:D * KPATCH].cpu(), None if db is None else db[:D].cpu(), dpos[:TOKENS * D].cpu(), dcls[:D].cpu()


@pytest.mark.parametrize("B,D,bias,splits", PATCH_CASES, ids=["B1-D384", "B2-D384", "B3-D384", "B6-D384", "B2-D768-clip"])
def test_patch16_embed_bwd(lib, device, B, D, bias, splits):
    need = lib.orbit_op_vit_linear_wgrad_workspace_floats(PATCHES * B, D, KPATCH)
    assert need == (splits * (D * KPATCH + D) if splits > 1 else 0), "M = %d: not %d splits" % (PATCHES * B, splits)
    assert (PATCHES * B) % 32 != 0
    frames, dtok, ref64, e32 = _patch_case(B, D, bias)
    runs = [_run_patch16(lib, device, frames, dtok, D, bias) for _ in range(2)]
    dw, db, dpos, dcls = runs[0]
    what = "patch16_embed_bwd B=%d D=%d " % (B, D)
    gate(dw.view(D, 3, 16, 16), ref64["w"], e32["w"], what + "dw")
    if bias:
        gate(db, ref64["b"], e32["b"], what + "dbias")
    dpos = dpos.view(1, TOKENS, D)
    gate(dpos[:, 1:], ref64["pos"], e32["pos"], what + "dpos rows 1..196")
    gate(dpos[:, :1], ref64["pos0"], e32["pos0"], what + "dpos row 0")
    gate(dcls.view(1, 1, D), ref64["cls"], e32["cls"], what + "dcls")
    assert torch.equal(dcls, dpos[0, 0]), what + "dcls is not row 0 of dpos"
    assert all(a is None and b is None or torch.equal(a, b) for a, b in zip(*runs)), what + "two runs differ"
    if bias:
        dw0, none, dpos0, dcls0 = _run_patch16(lib, device, frames, dtok, D, False)
        assert none is None and torch.equal(dw0, dw), what + "dw depends on whether dbias is asked for"
        assert torch.equal(dpos0.view(1, TOKENS, D), dpos) and torch.equal(dcls0, dcls)


def test_patch_32_through_the_new_entry_point_is_the_old_call_bit_for_bit(lib, device):
    B, D = 3, 384
    g = torch.Generator().manual_seed(1632)
    fr = torch.randn(B, 3, 224, 224, generator=g).to(device)
    dt = torch.randn(B * 50, D, generator=g).to(device)
    need = lib.orbit_op_vit_linear_wgrad_workspace_floats(49 * B, D, 3072)
    outs = []
    for new in (False, True):
        dw, db, ws = _tailed(D * 3072, device), _tailed(D, device), _tailed(need, device)
        dpos, dcls = _tailed(50 * D, device), _tailed(D, device)
        head = (_lib.dptr(fr), _lib.dptr(dt), _lib.dptr(dw), _lib.dptr(db), _lib.dptr(dpos), _lib.dptr(dcls), B, D)
        tail = (_lib.dptr(ws), need, _lib.stream_handle())
        if new:
            _lib.check(lib.orbit_op_vit_patch_embed_bwd_p(*head, 32, *tail), "orbit_op_vit_patch_embed_bwd_p")
        else:
            _lib.check(lib.orbit_op_vit_patch_embed_bwd(*head, *tail), "orbit_op_vit_patch_embed_bwd")
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (dw, db, dpos, dcls)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert all(torch.isfinite(t[:n]).all() for t, n in zip(outs[0], (D * 3072, D, 50 * D, D)))


@pytest.mark.parametrize("family", ["normal", "one_sign"])
@pytest.mark.parametrize("N,K", [(1152, 384), (384, 1536)], ids=["1152x384", "384x1536"])
def test_linear_wgrad_at_the_197_token_row_counts(lib, device, N, K, family):
    """M = 197 B for B = 1, 2, 3: one, two and four splits (the count doubles at 225 and 481 rows), none a multiple of 32."""
    x, _, _, dy = linear_inputs(K, N, 591, family, 1970 + N + K)
    for gelu in (0, 1):
        xg64, xg32 = (F.gelu(x.double()), F.gelu(x)) if gelu else (x.double(), x)
        for M, splits in ((197, 1), (394, 2), (591, 4)):
            need = lib.orbit_op_vit_linear_wgrad_workspace_floats(M, N, K)
            assert need == (splits * (N * K + N) if splits > 1 else 0), (M, N, K)
            ref64, refb = dy[:M].double().t() @ xg64[:M], dy[:M].double().sum(0)
            e32 = ((dy[:M].t() @ xg32[:M]).double() - ref64).abs().max().item()
            e32b = (dy[:M].sum(0).double() - refb).abs().max().item()
            what = "wgrad197 %dx%d %s gelu=%d M=%d" % (N, K, family, gelu, M)
            dw, db = run_wgrad(lib, device, dy, x, M, gelu, True)
            gate(dw.cpu(), ref64, e32, what + " dw")
            gate(db.cpu(), refb, e32b, what + " dbias")
            dw0, none = run_wgrad(lib, device, dy, x, M, gelu, False)
            assert none is None and torch.equal(dw0, dw), what + ": dw depends on whether dbias is asked for"
            dw2, db2 = run_wgrad(lib, device, dy, x, M, gelu, True)
            assert torch.equal(dw2, dw) and torch.equal(db2, db), what + ": two runs differ"
