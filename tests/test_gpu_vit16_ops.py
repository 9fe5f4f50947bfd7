"""The two kernels the patch-16 transformer extractors add to csrc/vit.hip, one by one, against a float64 CPU evaluation of the same
operation on the same fp32 inputs: the 197-token attention on the fp32 matrix cores (orbit_op_vit_attention_tokens) and the patch
embedding for 16 x 16 patches (orbit_op_vit_patch_embed_p).

Reference: plain torch in float64 (the four-line attention of tests/vit_pin.py; F.conv2d stride 16 + cat + pos_embed). Outputs
are NaN-filled before each call and followed by guard rows holding a sentinel, which must be intact afterwards.

Tolerance: the gate of tests/test_gpu_vit_ops.py, restated here and not tuned to the kernels. Every case measures its own
yardstick on the reference side only - `e32`, the largest error against float64 of a plain fp32 CPU evaluation of the same
operation on the same inputs (torch fp32 for the attention; the explicit k = 0, 1, 2, ... fp32 multiply-add chain of that file
for the patch GEMM). The gate is

    max |got - ref64|  <=  max(4 * e32, 8 * 2**-24 * max |ref64|)

Largest err / e32 seen on the MI355X (every case prints its ratio; run with -s):
  attention, 197 tokens   2.17  (uniform: err 1.2e-7 on outputs of 0.25, under the 8 * 2**-24 floor too; gaussian 1.27, peaked 1.17,
                                last_token 0 / 0 - exact on both sides)
  patch embedding, p16    2.07  (D = 768, 980 rows: the maximum over 753 k outputs against a sample of 4096)
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from test_gpu_vit_ops import EPI_RESIDUAL, _prof_rows, attention_ref, linear_e32  # noqa: E402

U = 2.0 ** -24
GUARD = 128          # guard rows after the attention output
GUARD_TOKENS = 192   # after the patch embedding's tokens: 127 GEMM rows past the tail reach token row 197 B + 128
SENTINEL = 7777.0
NAN = float("nan")
TILES = (64, 128)
T16, P16, K16 = 197, 196, 768


def _st():
    return _lib.stream_handle()


def gate(got, ref64, e32, what):
    """The module's gate (docstring); returns err / e32 and prints it."""
    assert torch.isfinite(got).all(), "%s: non-finite or unwritten output" % what
    err = (got.double() - ref64).abs().max().item()
    tol = max(4 * e32, 8 * U * ref64.abs().max().item())
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
    print("[vit16-ops] %-58s err %.3g  e32 %.3g  err/e32 %.2f" % (what, err, e32, ratio))
    assert err <= tol, "%s: max |got - ref64| = %.4g > %.4g (e32 = %.4g, err / e32 = %.2f)" % (what, err, tol, e32, ratio)
    return ratio


# ---- attention, 197 tokens ---------------------------------------------------------------------------------------------
ATTN_FAMILIES = ("gaussian", "peaked", "uniform", "last_token")


def attention_inputs(B, heads, family, seed, tokens=T16):
    """qkv [B][tokens][3 * heads * 64] fp32 of one family."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, tokens, heads, 64, generator=g) for _ in range(3))
    unit = torch.full((64,), 0.125)  # |unit| = 1
    if family == "peaked":
        # q and k scaled so that the largest |logit| is 15: rows dominated by one or two keys, exponentials spanning e^-30 .. 1
        top = (torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / 8).abs().max().item()
        s = (15.0 / top) ** 0.5
        q, k = q * s, k * s
    elif family == "uniform":
        # every logit of a row is the same number: P is exactly 1/197, the output is the mean of V; a padded key column counted
        # in the sum would give 1/208 or 1/224
        k = k[:, :1].expand(B, tokens, heads, 64).contiguous()
    elif family == "last_token":
        # only key 196 (the last valid one, in the partly filled key tile) carries weight - logit ~ 50 against ~ 0 - and only value
        # row 196 is non-zero: a tail tile dropped from PV gives zeros
        q = 0.1 * q + 4.0 * unit
        k = 0.1 * k
        k[:, tokens - 1] += 100.0 * unit
        v[:, :tokens - 1] = 0.0
    else:
        assert family == "gaussian"
    return torch.stack((q, k, v), dim=2).reshape(B, tokens, 3 * heads * 64).contiguous()


def run_attention(lib, device, qkv, heads, tokens=T16, entry="tokens"):
    B, D = qkv.shape[0], heads * 64
    out = torch.full((B * tokens + GUARD, D), NAN, device=device)
    out[B * tokens:] = SENTINEL
    qd = qkv.to(device)
    if entry == "tokens":
        rc = lib.orbit_op_vit_attention_tokens(_lib.dptr(qd), _lib.dptr(out), B, tokens, D, heads, _st())
    else:
        rc = lib.orbit_op_vit_attention(_lib.dptr(qd), _lib.dptr(out), B, D, heads, _st())
    _lib.check(rc, "orbit_op_vit_attention_tokens")
    torch.cuda.synchronize()
    assert bool((out[B * tokens:] == SENTINEL).all()), "rows past B * %d were written" % tokens
    return out[:B * tokens].cpu().reshape(B, tokens, D)


@pytest.mark.parametrize("family", ATTN_FAMILIES)
@pytest.mark.parametrize("D,heads", [(384, 6), (768, 12)])
def test_attention_197(lib, device, D, heads, family):
    qkv = attention_inputs(3, heads, family, 1700 + D)
    ref64_all = attention_ref(qkv.double(), heads)
    ref32_all = attention_ref(qkv, heads)
    v = qkv.reshape(3, T16, 3, heads, 64)[:, :, 2].double()
    if family == "peaked":
        q, k = (qkv.reshape(3, T16, 3, heads, 64)[:, :, i].double() for i in (0, 1))
        assert 14.9 < (torch.einsum("bqhd,bkhd->bhqk", q, k) / 8).abs().max().item() < 15.1
    elif family == "uniform":
        assert (ref64_all - v.mean(1, keepdim=True).reshape(3, 1, D)).abs().max().item() < 1e-12
    elif family == "last_token":
        assert (ref64_all - v[:, T16 - 1:].reshape(3, 1, D)).abs().max().item() < 1e-12
        assert ref64_all.abs().min().item() > 0  # a zero output is a dropped tile, not a coincidence
    outs = {}
    for B in (1, 2, 3):
        ref64 = ref64_all[:B]
        e32 = (ref32_all[:B].double() - ref64).abs().max().item()
        outs[B] = run_attention(lib, device, qkv[:B], heads)
        gate(outs[B], ref64, e32, "attention197 D=%d %s B=%d" % (D, family, B))
    assert torch.equal(outs[3][0], outs[1][0]), "frame 0 depends on the frames that share its launch"
    assert torch.equal(outs[3][:2], outs[2])


@pytest.mark.parametrize("D,heads", [(384, 6), (768, 12)])
def test_attention_head_columns_197(lib, device, D, heads):
    """V constant per head: head h's output is h + 1 in columns h * 64 .. h * 64 + 63 of every token row."""
    g = torch.Generator().manual_seed(5)
    q, k = (torch.randn(2, T16, heads, 64, generator=g) for _ in range(2))
    v = (torch.arange(heads) + 1.0)[None, None, :, None].expand(2, T16, heads, 64)
    qkv = torch.stack((q, k, v), dim=2).reshape(2, T16, 3 * D).contiguous()
    got = run_attention(lib, device, qkv, heads)
    want = (torch.arange(heads) + 1.0).repeat_interleave(64)
    assert (got - want).abs().max().item() <= 64 * U * heads


@pytest.mark.parametrize("D,heads", [(384, 6), (768, 12)])
def test_attention_tokens_50_is_the_existing_kernel(lib, device, D, heads):
    qkv = attention_inputs(3, heads, "gaussian", 50 + D, tokens=50)
    lib.orbit_prof_enable(1)
    try:
        new = run_attention(lib, device, qkv, heads, tokens=50)
        old = run_attention(lib, device, qkv, heads, tokens=50, entry="plain")
        rows = {k: n for k, n in _prof_rows(lib).items() if k.startswith("vit_")}
    finally:
        lib.orbit_prof_enable(0)
    assert rows == {"vit_attention": 2}, rows
    assert torch.equal(new, old)


def test_attention_other_token_counts_are_refused(lib, device):
    out = torch.full((4 * 224, 384), SENTINEL, device=device)
    qkv = torch.zeros(4 * 224, 3 * 384, device=device)
    lib.orbit_prof_enable(1)
    try:
        for tokens in (49, 196, 198):
            assert lib.orbit_op_vit_attention_tokens(_lib.dptr(qkv), _lib.dptr(out), 1, tokens, 384, 6, _st()) == -1
            assert "tokens" in _lib.last_error()
        assert not any(_prof_rows(lib).values()), "a refused call launched something"
    finally:
        lib.orbit_prof_enable(0)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- patch embedding, 16 x 16 patches -----------------------------------------------------------------------------------
PATCH_BS = (1, 2, 3, 5)  # 196, 392, 588, 980 GEMM rows: tails of 68, 8, 76 and 84 rows against 128-row tiles


def patch_inputs(D, B, seed):
    """Frames in which every (channel, row, column) position has its own value (a ramp over c, h, w plus per-frame noise): a
    swapped kh / kw or a c * 256 vs c * 16 slip in the gather then moves the result by far more than rounding."""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(-1.0, 1.0, 3 * 224 * 224).reshape(1, 3, 224, 224)
    frames = ramp + 0.25 * torch.randn(B, 3, 224, 224, generator=g)
    w = torch.randn(D, 3, 16, 16, generator=g) / K16 ** 0.5
    bias = 0.5 * torch.randn(D, generator=g)
    pos = torch.randn(T16, D, generator=g)
    cls = torch.randn(D, generator=g)
    return frames, w, bias, pos, cls


def patch_ref64(frames, w, bias, pos, cls):
    t = F.conv2d(frames.double(), w.double(), None if bias is None else bias.double(), stride=16).flatten(2).transpose(1, 2)
    return torch.cat((cls.double().expand(t.shape[0], 1, -1), t), dim=1) + pos.double()


def run_patch_embed(lib, device, frames, w, bias, pos, cls, B, tile, patch=16, tokens=T16, entry="p"):
    D = w.shape[0]
    out = torch.full((B * tokens + GUARD_TOKENS, D), NAN, device=device)
    out[B * tokens:] = SENTINEL
    fr = frames[:B].contiguous()
    if entry == "p":
        rc = lib.orbit_op_vit_patch_embed_p(_lib.dptr(fr), _lib.dptr(w), _lib.dptr(bias), _lib.dptr(pos), _lib.dptr(cls),
                                            _lib.dptr(out), B, D, patch, tile, _st())
    else:
        rc = lib.orbit_op_vit_patch_embed(_lib.dptr(fr), _lib.dptr(w), _lib.dptr(bias), _lib.dptr(pos), _lib.dptr(cls),
                                          _lib.dptr(out), B, D, tile, _st())
    _lib.check(rc, "orbit_op_vit_patch_embed_p")
    torch.cuda.synchronize()
    assert bool((out[B * tokens:] == SENTINEL).all()), "token rows past B * %d were written (B=%d tile=%d)" % (tokens, B, tile)
    return out[:B * tokens].cpu().reshape(B, tokens, D)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("D", [384, 768])
def test_patch_embed_16(lib, device, D, with_bias):
    frames, w, bias, pos, cls = patch_inputs(D, max(PATCH_BS), 1600 + D)
    if not with_bias:
        bias = None
    ref64 = patch_ref64(frames, w, bias, pos, cls)
    # the same GEMM, k = c * 256 + kh * 16 + kw (F.unfold's order is the OIHW filter's), for the sequential-k yardstick and the
    # textbook bound gamma_(K+3) (|x| |w|^T + |bias| + |pos|) of any correct fp32 evaluation
    rows = F.unfold(frames, 16, stride=16).transpose(1, 2).reshape(-1, K16).contiguous()
    w2 = w.reshape(D, K16)
    posr = pos[1:].repeat(max(PATCH_BS), 1)
    gamma = (K16 + 3) * U / (1 - (K16 + 3) * U)
    mag = rows.double().abs() @ w2.double().abs().t() + posr.double().abs()
    if bias is not None:
        mag = mag + bias.double().abs()
    bound = gamma * mag
    dev = [None if t is None else t.to(device) for t in (frames, w, bias, pos, cls)]
    row0 = cls + pos[0]
    out = {}
    lib.orbit_prof_enable(1)
    try:
        for B in PATCH_BS:
            patches64 = ref64[:B, 1:].reshape(B * P16, D)
            e32 = linear_e32(rows, w2, bias, posr, EPI_RESIDUAL, patches64, B * P16, seed=B)
            for tile in TILES:
                got = run_patch_embed(lib, device, *dev, B, tile)
                what = "patch_embed16 D=%d %s B=%d tile=%d" % (D, "bias" if with_bias else "no bias", B, tile)
                gate(got, ref64[:B], e32, what)
                over = ((got[:, 1:].reshape(B * P16, D).double() - patches64).abs() / bound[:B * P16]).max().item()
                assert over <= 1.0, "%s: an element is %.3g x the worst-case fp32 bound" % (what, over)
                assert torch.equal(got[:, 0], row0.expand(B, D)), "%s: class-token row is not cls_token + pos_embed[0]" % what
                out[B, tile] = got
        prof = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    for tile in TILES:
        assert prof.get("vit_op_patch_embed<%d>" % tile, 0) == len(PATCH_BS), prof
    for (B, tile), got in out.items():
        assert torch.equal(got, out[max(PATCH_BS), 64][:B]), "tokens depend on the batch or the tile height (B=%d, tile=%d)" % (B, tile)


@pytest.mark.parametrize("D", [384, 768])
def test_patch_embed_16_single_pixel(lib, device, D):
    """A frame that is zero except pixel (c, y, x) = (2, 17, 209): it lies in patch (1, 13) at (py, px) = (1, 1) - the SECOND
    frame row of a 32-deep K step - so token row 1 + 1 * 14 + 13 = 28 is w[:, 2, 1, 1] * value + bias + pos and every other patch
    row is bias + pos, bit for bit. A swapped py / px lands in patch (13, 1); a wrong second half of the K step in another k."""
    _, w, bias, pos, cls = patch_inputs(D, 1, 1650 + D)
    frames = torch.zeros(2, 3, 224, 224)
    frames[1, 2, 17, 209] = 1.5
    dev = [t.to(device) for t in (frames, w, bias, pos, cls)]
    ref64 = patch_ref64(frames, w, bias, pos, cls)
    for tile in TILES:
        got = run_patch_embed(lib, device, *dev, 2, tile)
        rest = (bias + pos[1:]).expand(2, P16, D).clone()
        hit = got[1, 28].clone()
        got_rest = got[:, 1:].clone()
        got_rest[1, 27] = rest[1, 27]
        assert torch.equal(got_rest, rest), "a patch row other than (1, 13) of frame 1 moved"
        want = 1.5 * w[:, 2, 1, 1].double() + bias.double() + pos[28].double()
        assert (ref64[1, 28] - want).abs().max().item() < 1e-12
        assert (hit.double() - want).abs().max().item() <= 8 * U * want.abs().max().item()
        assert (hit - rest[1, 27]).abs().max().item() > 1e-3  # the pixel reaches its row


@pytest.mark.parametrize("D", [384, 768])
def test_patch_embed_p_32_is_the_existing_kernel(lib, device, D):
    g = torch.Generator().manual_seed(32 + D)
    frames = torch.randn(3, 3, 224, 224, generator=g)
    w = torch.randn(D, 3, 32, 32, generator=g) / 3072 ** 0.5
    bias, pos, cls = torch.randn(D, generator=g), torch.randn(50, D, generator=g), torch.randn(D, generator=g)
    dev = [t.to(device) for t in (frames, w, bias, pos, cls)]
    for tile in TILES:
        new = run_patch_embed(lib, device, *dev, 3, tile, patch=32, tokens=50)
        old = run_patch_embed(lib, device, *dev, 3, tile, tokens=50, entry="plain")
        assert torch.equal(new, old)
