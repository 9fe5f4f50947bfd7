"""Every kernel form csrc/head.hip dispatches to, called through the C ABI (the Python layer always passes n_tasks = 1),
against fp64 references computed on the CPU from the same fp32 inputs, plus the linear head's parameter gradients.

Forms of orbit_proto_predict (the launcher's rule is restated by _form below, and every case asserts the form it means):
  stream   head_stream = 1, T = 1, D in {512, 1280}, D % 4 == 0, (C D + C) 4 B <= 60 KB, M n_tasks >= 64
           proto_predict_stream_kernel<8, 2, 5> / <8, 2, 2>, and <8, 2, 5, LEAN> for D = 1280, euclidean, no argmax
  lds      the same launches with head_stream = 0, any T and any D % 4 == 0: proto_predict_lds_kernel<5, 4> / <10, 4>
  generic  everything else (weights over the LDS limit, D % 4 != 0, fewer than 64 rows): proto_predict_kernel<5, 1> / <10, 1>
The R > 1 generic instantiations (proto_predict_kernel<5, 4> / <10, 2>) are only chosen from 2^30 blocks of 16 rows on:
no test can reach them, they stay untested.

Error bounds, with u = 2^-24 and gamma_k = k u. A lane accumulates D / 64 products, the wave reduction adds 6 levels, bias
and scale one rounding each: k = D / 64 + 8 (plus T + 1 where T frames are averaged on load).
  euclidean   |got - want| <= 2 k u |scale| (sum_d |q_d| |w_d| + |b_c|)
  cosine      |got - want| <= 2 |scale| (k u sum |q| |w| / (|q| |w|) + (D / 64 + 16) u |cos|)   (norms, sqrtf, division)
The factor 2 is the only slack. Each test prints its largest error / bound ratio (pytest -s).
"""
import contextlib
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from oracle import blocks  # noqa: E402
from orbit_dataset_amd import _lib  # noqa: E402

U = 2.0 ** -24
ERR_ARG = -1
SCALE = {0: 1.5, 1: 20.0}  # logit_scale per distance (euclidean, cosine)


def _st():
    return _lib.stream_handle()


@contextlib.contextmanager
def _option(lib, name, value):
    prev = lib.orbit_get_option(name.encode())
    assert prev >= 0, name
    try:
        assert lib.orbit_set_option(name.encode(), value) == 0
        yield
    finally:
        lib.orbit_set_option(name.encode(), prev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _form(n_tasks, M, T, D, C, head_stream):
    """proto_predict_impl's dispatch rule (csrc/head.hip), restated."""
    if D % 4 == 0 and (C * D + C) * 4 <= 60 * 1024 and M * n_tasks >= 64:
        return "stream" if head_stream and T == 1 and D in (512, 1280) else "lds"
    return "generic"


# ---- predict: data, fp64 reference and bound, once per shape ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _predict_case(n_tasks, M, T, D, C, cosine, tie=None):
    """Clustered non-negative features (as _task of test_gpu_head.py): class centres, prototypes near them, every query
    near the centre of a random class, different data in every task. tie = (lo, hi): prototype hi is a copy of lo and every
    other query sits at that pair."""
    g = torch.Generator().manual_seed(100000 * cosine + 1000 * C + 10 * D + 3 * n_tasks + T + (7 if tie else 0))
    centres = torch.randn(n_tasks, C, D, generator=g) * 0.3
    mu = torch.relu(centres + 0.1 * torch.randn(n_tasks, C, D, generator=g))
    qc = torch.randint(0, C, (n_tasks, M), generator=g)
    if tie:
        mu[:, tie[1]] = mu[:, tie[0]]
        qc[:, ::2] = tie[0]
    W = (2.0 * mu).contiguous()
    b = -(mu * mu).sum(-1)
    if tie:
        b[:, tie[1]] = b[:, tie[0]]
    cq = torch.gather(centres, 1, qc[:, :, None].expand(-1, -1, D))
    Q = torch.relu(cq.repeat_interleave(T, 1) + 0.5 * torch.randn(n_tasks, M * T, D, generator=g)).contiguous()
    scale = SCALE[cosine]
    q = Q.double().view(n_tasks, M, T, D).mean(2)
    Wd = W.double()
    dot = q @ Wd.transpose(1, 2)
    absdot = q.abs() @ Wd.abs().transpose(1, 2)
    k = D / 64 + 8 + (T + 1 if T > 1 else 0)
    if cosine:
        qn, wn = q.norm(dim=2)[:, :, None], Wd.norm(dim=2)[:, None, :]
        assert qn.min().item() > 0 and wn.min().item() > 0  # the all-zero row has its own check
        cos = dot / (qn.clamp_min(1e-8) * wn.clamp_min(1e-8))
        want = scale * cos
        bound = 2 * abs(scale) * (k * U * absdot / (qn * wn) + (D / 64 + 16) * U * cos.abs())
    else:
        want = scale * (dot + b.double()[:, None, :])
        bound = 2 * k * U * abs(scale) * (absdot + b.double().abs()[:, None, :])
    top2 = want.topk(2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) > 2 * bound.max(-1).values  # rows whose fp64 argmax the bound cannot flip
    return types.SimpleNamespace(n_tasks=n_tasks, M=M, T=T, D=D, C=C, cosine=cosine, scale=scale, Q=Q, W=W, b=b, want=want,
                                 bound=bound, sure=sure, skip_share=1.0 - sure.double().mean().item())


def _launch(lib, Q, W, b, M, T, cosine, scale, with_argmax=True):
    """One orbit_proto_predict launch over CPU tensors Q [n][M T][D], W [n][C][D], b [n][C]; outputs start as NaN / -1."""
    n_tasks, C, D = W.shape
    dev = torch.device("cuda", 0)
    Qd, Wd = Q.contiguous().to(dev), W.contiguous().to(dev)
    bd = None if cosine else b.contiguous().to(dev)  # the cosine head has no bias: NULL
    logits = torch.full((n_tasks, M, C), float("nan"), device=dev)
    amax = torch.full((n_tasks, M), -1, dtype=torch.int32, device=dev) if with_argmax else None
    _lib.check(lib.orbit_proto_predict(_lib.dptr(Qd), _lib.dptr(Wd), _lib.dptr(bd), n_tasks, M, T, D, C, scale, cosine,
                                       _lib.dptr(logits), _lib.dptr(amax), _st()), "orbit_proto_predict")
    torch.cuda.synchronize()
    return logits.cpu(), (amax.cpu() if with_argmax else None)


@functools.lru_cache(maxsize=None)
def _gpu_result(key, with_argmax, head_stream):
    """The case's main launch (shared between the per-form test and the stream == LDS comparison)."""
    lib = _lib.load()
    c = _predict_case(*key)
    with _option(lib, "head_stream", head_stream):
        return _launch(lib, c.Q, c.W, c.b, c.M, c.T, c.cosine, c.scale, with_argmax)


def _check_against_fp64(c, logits, amax, what):
    err = (logits.double() - c.want).abs()
    ratio = (err / c.bound).max().item()
    print("%s: max error / bound = %.3f" % (what, ratio))
    assert bool((err <= c.bound).all()), (what, ratio)  # (a NaN left from the pre-fill fails here)
    if amax is not None:
        assert torch.equal(amax.long(), logits.argmax(-1)), what  # the fused argmax is the argmax of its own logits
        assert c.skip_share <= 0.05, (what, c.skip_share)
        assert torch.equal(amax.long()[c.sure], c.want.argmax(-1)[c.sure]), what


def _check_predict(lib, key, with_argmax, head_stream, form):
    c = _predict_case(*key)
    what = "%s n=%d M=%d T=%d D=%d C=%d %s%s" % (form, c.n_tasks, c.M, c.T, c.D, c.C, "cosine" if c.cosine else "euclidean",
                                                 "" if with_argmax else " no-argmax")
    assert _form(c.n_tasks, c.M, c.T, c.D, c.C, head_stream) == form
    logits, amax = _gpu_result(key, with_argmax, head_stream)
    _check_against_fp64(c, logits, amax, what)
    with _option(lib, "head_stream", head_stream):
        # passing or omitting the argmax pointer leaves the logits alone
        other, _ = _launch(lib, c.Q, c.W, c.b, c.M, c.T, c.cosine, c.scale, not with_argmax)
        assert _same_bits(other, logits), what
        # a task's logits do not depend on its place in the batch (same kernel, other task offsets and block mapping)
        if c.n_tasks > 1:
            rl, ra = _launch(lib, c.Q.flip(0), c.W.flip(0), c.b.flip(0), c.M, c.T, c.cosine, c.scale, with_argmax)
            assert _same_bits(rl.flip(0), logits), what
            assert amax is None or torch.equal(ra.flip(0), amax), what
        # ... nor on the batch: the task launched alone, where that launch runs the same kernel
        if c.n_tasks > 1 and _form(1, c.M, c.T, c.D, c.C, head_stream) == form:
            for t in range(c.n_tasks):
                al, aa = _launch(lib, c.Q[t:t + 1], c.W[t:t + 1], c.b[t:t + 1], c.M, c.T, c.cosine, c.scale, with_argmax)
                assert _same_bits(al[0], logits[t]), (what, t)
                assert amax is None or torch.equal(aa[0], amax[t]), (what, t)
        if c.cosine:
            # an all-zero query row scores exactly 0.0 on every column (eps-clamped norm), and disturbs no other row
            Qz = c.Q.clone().view(c.n_tasks, c.M, c.T, c.D)
            rows = [(0, 0), (c.n_tasks - 1, c.M - 1), (c.n_tasks // 2, c.M // 2)]
            for t, m in rows:
                Qz[t, m] = 0
            zl, za = _launch(lib, Qz.view(c.n_tasks, c.M * c.T, c.D), c.W, c.b, c.M, c.T, 1, c.scale, True)
            keep = torch.ones(c.n_tasks, c.M, dtype=torch.bool)
            for t, m in rows:
                keep[t, m] = False
                assert _same_bits(zl[t, m], torch.zeros(c.C)), (what, t, m)  # +0.0
                assert za[t, m].item() == 0
            assert _same_bits(zl[keep], logits[keep]), what


# D, C, cosine, argmax buffer: n_tasks = 5, M = 37 -> 3 row blocks per task (the last with 5 of its 16 rows), a grid of 15
# blocks, on which xcd_remap is not the identity
STREAM_CASES = [(1280, 5, 0, False),  # the LEAN instantiation
                (1280, 5, 0, True), (1280, 5, 1, True), (512, 10, 0, True), (512, 10, 1, True),
                (1280, 11, 0, True),  # the largest LDS fit: 56 KB of dynamic LDS
                (512, 20, 1, True)]
_ids = lambda c: "-".join(map(str, c))  # noqa: E731


@pytest.mark.parametrize("case", STREAM_CASES, ids=_ids)
def test_proto_predict_stream_form(lib, device, case):
    D, C, cosine, with_argmax = case
    _check_predict(lib, (5, 37, 1, D, C, cosine), with_argmax, 1, "stream")


@pytest.mark.parametrize("case", STREAM_CASES, ids=_ids)
def test_proto_predict_lds_form_on_stream_cases(lib, device, case):
    D, C, cosine, with_argmax = case
    _check_predict(lib, (5, 37, 1, D, C, cosine), with_argmax, 0, "lds")


@pytest.mark.parametrize("case", STREAM_CASES, ids=_ids)
def test_proto_predict_stream_agrees_with_lds(lib, device, case):
    """The two forms accumulate in the same order but are NOT bit-equal (measured on an MI355X at 1280 / 5 euclidean: the
    logits differ in their last bits). Each quad x.x w.x + x.y w.y + x.z w.z + x.w w.w is contracted to one rounded product
    and three FMAs, and the compiler picks the rounded product per instantiation (csrc/head.hip says so at the stream
    kernel). What holds: each form is within the fp64 bound (the two tests above), so they differ by at most twice the
    bound, and they name the same class wherever the fp64 gap exceeds that."""
    D, C, cosine, with_argmax = case
    key = (5, 37, 1, D, C, cosine)
    c = _predict_case(*key)
    sl, sa = _gpu_result(key, with_argmax, 1)
    ll, la = _gpu_result(key, with_argmax, 0)
    diff = (sl.double() - ll.double()).abs()
    print("stream vs lds D=%d C=%d %s: max difference / bound = %.3f, %d of %d logits differ"
          % (D, C, "cosine" if cosine else "euclidean", (diff / c.bound).max().item(), int((diff > 0).sum()), diff.numel()))
    assert bool((diff <= 2 * c.bound).all())
    assert sa is None or torch.equal(sa[c.sure], la[c.sure])


# n_tasks, M, T, D, C
LDS_CASES = [(2, 35, 3, 512, 5),   # the pooling loop
             (3, 23, 1, 100, 7),   # CT = 10 with a partial chunk, D no multiple of 256
             (2, 33, 2, 512, 12),  # a second, partial c0 pass
             (4, 17, 1, 64, 23)]   # three c0 passes, one float4 per lane on a quarter of the lanes
GENERIC_CASES = [(3, 30, 1, 1280, 12),  # 12 x 1280 weights are over the LDS limit
                 (3, 30, 2, 130, 7),    # D % 4 != 0: the scalar path, with pooling
                 (2, 5, 1, 97, 5),      # fewer than 64 rows
                 (1, 9, 1, 512, 23)]


@pytest.mark.parametrize("cosine", [0, 1])
@pytest.mark.parametrize("shape", LDS_CASES, ids=_ids)
def test_proto_predict_lds_form(lib, device, shape, cosine):
    _check_predict(lib, shape + (cosine,), True, 0, "lds")


@pytest.mark.parametrize("cosine", [0, 1])
@pytest.mark.parametrize("shape", GENERIC_CASES, ids=_ids)
def test_proto_predict_generic_form(lib, device, shape, cosine):
    _check_predict(lib, shape + (cosine,), True, 1, "generic")


@pytest.mark.parametrize("cosine", [0, 1])
@pytest.mark.parametrize("C,tie", [(5, (1, 3)), (12, (3, 11))])  # (3, 11): across the CT = 10 chunk edge
@pytest.mark.parametrize("form,head_stream,n_tasks,M", [("stream", 1, 5, 37), ("lds", 0, 5, 37), ("generic", 1, 2, 9)])
def test_proto_predict_argmax_ties(lib, device, form, head_stream, n_tasks, M, C, tie, cosine):
    """Two identical prototypes with identical bias: bit-equal logit columns, and the argmax is the lower column (the first
    maximal one, as torch.argmax)."""
    D = 512
    assert _form(n_tasks, M, 1, D, C, head_stream) == form
    c = _predict_case(n_tasks, M, 1, D, C, cosine, tie)
    with _option(lib, "head_stream", head_stream):
        logits, amax = _launch(lib, c.Q, c.W, c.b, M, 1, cosine, c.scale)
    err = (logits.double() - c.want).abs()
    assert bool((err <= c.bound).all())
    lo, hi = tie
    assert _same_bits(logits[..., lo], logits[..., hi])
    assert torch.equal(amax.long(), logits.argmax(-1))
    tied_rows = logits.max(-1).values == logits[..., lo]
    assert tied_rows.double().mean().item() >= 0.4  # every other query sits at the tied pair
    assert bool((amax[tied_rows] == lo).all())


# ---- configure + finalize: batched, over the 1024-label chunk edges -------------------------------------------------------
CFG_TASKS, CFG_SLOTS = 3, 8
# the 7 labels of each task (non-contiguous, negative, above 2^32) and its 8 class_ids slots: one id that no clip carries in
# tasks 0 and 2 (at the end / in the middle), task 1 padded as orbit_label_set pads (the last id again)
CFG_REAL = [[3, 4, 9, 17, 40, 41, 1000], [-5, 0, 2, 7, 8, 2 ** 40, 2 ** 40 + 3], [1, 5, 6, 20, 21, 22, 90]]
CFG_IDS = [CFG_REAL[0] + [2000], CFG_REAL[1] + [CFG_REAL[1][-1]], CFG_REAL[2][:3] + [7] + CFG_REAL[2][3:]]
CFG_KEEP = [[0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 7], [0, 1, 2, 4, 5, 6, 7]]  # finalize input: the absent id left out


@functools.lru_cache(maxsize=None)
def _configure_case(N, T, D):
    g = torch.Generator().manual_seed(N * 7 + T * 3 + D)
    feats = (torch.randn(CFG_TASKS, N * T, D, generator=g) + 0.5).contiguous()
    cls = torch.randint(0, 7, (CFG_TASKS, N), generator=g)
    for lo in range(0, N, 1024):  # every class on both sides of every chunk edge (where the chunk has room for that)
        chunk = cls[:, lo:lo + 1024]
        if chunk.shape[1] >= 50:
            assert all(len(torch.unique(chunk[t])) == 7 for t in range(CFG_TASKS))
    labels = torch.stack([torch.tensor(CFG_REAL[t])[cls[t]] for t in range(CFG_TASKS)]).contiguous()
    pooled = feats.double().view(CFG_TASKS, N, T, D).mean(2)
    pooled_abs = feats.double().abs().view(CFG_TASKS, N, T, D).mean(2)
    sums = torch.zeros(CFG_TASKS, CFG_SLOTS, D, dtype=torch.float64)
    mag = torch.zeros(CFG_TASKS, CFG_SLOTS, D, dtype=torch.float64)
    counts = torch.zeros(CFG_TASKS, CFG_SLOTS, dtype=torch.float64)
    seq = torch.zeros(CFG_TASKS, CFG_SLOTS, D)  # T == 1: the sequential fp32 sum over the class's rows, ascending
    for t in range(CFG_TASKS):
        for s, cid in enumerate(CFG_IDS[t]):
            rows = torch.nonzero(labels[t] == cid).flatten()
            counts[t, s] = len(rows)
            sums[t, s] = pooled[t, rows].sum(0)
            mag[t, s] = pooled_abs[t, rows].sum(0)
            if T == 1:
                acc = torch.zeros(D)
                for i in rows.tolist():
                    acc += feats[t, i]
                seq[t, s] = acc
    return types.SimpleNamespace(feats=feats, labels=labels, ids=torch.tensor(CFG_IDS), sums=sums, mag=mag, counts=counts,
                                 seq=seq)


def _ulp32(x):
    """Spacing of fp32 at |x| (x fp64), not below the smallest normal's."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


@pytest.mark.parametrize("N", [1023, 1024, 1025, 2100])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("D", [100, 512])
def test_proto_configure_finalize_batched_chunked(lib, device, D, T, N):
    c = _configure_case(N, T, D)
    fd, ld, idd = c.feats.to(device), c.labels.to(device), c.ids.to(device)
    sums = torch.full((CFG_TASKS, CFG_SLOTS, D), float("nan"), device=device)
    counts = torch.full((CFG_TASKS, CFG_SLOTS), float("nan"), device=device)
    _lib.check(lib.orbit_proto_configure(_lib.dptr(fd), _lib.dptr(ld), _lib.dptr(idd), CFG_TASKS, N, T, D, CFG_SLOTS,
                                         _lib.dptr(sums), _lib.dptr(counts), _st()), "orbit_proto_configure")
    torch.cuda.synchronize()
    got, cnt = sums.cpu(), counts.cpu()
    assert torch.equal(cnt.double(), c.counts)
    assert cnt[0, 7].item() == 0 and cnt[2, 3].item() == 0
    assert _same_bits(got[0, 7], torch.zeros(D)) and _same_bits(got[2, 3], torch.zeros(D))  # the id without clips
    assert _same_bits(got[1, 7], got[1, 6]) and cnt[1, 7].item() == cnt[1, 6].item()     # the padded slot
    n_c = c.counts[:, :, None]
    bound = (n_c * T + 2) * U * c.mag
    err = (got.double() - c.sums).abs()
    live = bound > 0
    print("configure N=%d T=%d D=%d: max error / bound = %.3f" % (N, T, D, (err[live] / bound[live]).max().item()))
    assert bool((err <= bound).all())
    if T == 1:  # the header's promise: ascending clip order, nothing else (T > 1: acc += s * invT may become an FMA)
        assert _same_bits(got, c.seq)
    # finalize over the same sums / counts without the absent id, both distances
    keep = torch.tensor(CFG_KEEP, device=device)
    sk = torch.gather(sums, 1, keep[:, :, None].expand(-1, -1, D)).contiguous()
    ck = torch.gather(counts, 1, keep).contiguous()
    mu = sk.cpu().double() / ck.cpu().double()[:, :, None]
    want_W, want_b = 2 * mu, -(mu * mu).sum(-1)
    C = keep.shape[1]
    for cosine in (0, 1):
        W = torch.full((CFG_TASKS, C, D), float("nan"), device=device)
        b = None if cosine else torch.full((CFG_TASKS, C), float("nan"), device=device)
        _lib.check(lib.orbit_proto_finalize(_lib.dptr(sk), _lib.dptr(ck), CFG_TASKS, C, D, cosine, _lib.dptr(W), _lib.dptr(b),
                                            _st()), "orbit_proto_finalize")
        torch.cuda.synchronize()
        assert bool(((W.cpu().double() - want_W).abs() <= 2 * _ulp32(want_W)).all())
        if not cosine:
            assert bool(((b.cpu().double() - want_b).abs() <= (D / 256 + 12) * U * want_b.abs()).all())
            W_euclid = W.cpu()
        else:
            assert _same_bits(W.cpu(), W_euclid)


def test_proto_head_chain_matches_oracle(lib, device):
    """orbit_label_set -> configure -> finalize -> predict, three tasks in every launch, against oracle.blocks in fp64 per
    task. Bound: the predict bound, plus the configure and finalize bounds carried through logits = scale (q.W + b):
    |dW_d| <= 2 ((n_c + 2) u mean_c|x_d| + 2 u |mu_d|), |db| <= sum_d |mu_d| |dW_d| + (D / 256 + 12) u sum mu^2."""
    N, T, D, M, C, scale = 1025, 1, 512, 37, 7, 1.5
    c = _configure_case(N, T, D)
    q = _predict_case(CFG_TASKS, M, 1, D, C, 0).Q
    fd, ld, qd = c.feats.to(device), c.labels.to(device), q.to(device)
    ids = torch.full((CFG_TASKS, C), -1, dtype=torch.int64, device=device)
    n_ids = torch.full((CFG_TASKS,), -1, dtype=torch.int32, device=device)
    for t in range(CFG_TASKS):
        _lib.check(lib.orbit_label_set(_lib.dptr(ld[t]), N, _lib.dptr(ids[t]), C, _lib.dptr(n_ids[t:]), _st()), "label_set")
    sums, counts = torch.empty(CFG_TASKS, C, D, device=device), torch.empty(CFG_TASKS, C, device=device)
    W, b = torch.empty(CFG_TASKS, C, D, device=device), torch.empty(CFG_TASKS, C, device=device)
    logits = torch.full((CFG_TASKS, M, C), float("nan"), device=device)
    _lib.check(lib.orbit_proto_configure(_lib.dptr(fd), _lib.dptr(ld), _lib.dptr(ids), CFG_TASKS, N, T, D, C, _lib.dptr(sums),
                                         _lib.dptr(counts), _st()), "orbit_proto_configure")
    _lib.check(lib.orbit_proto_finalize(_lib.dptr(sums), _lib.dptr(counts), CFG_TASKS, C, D, 0, _lib.dptr(W), _lib.dptr(b),
                                        _st()), "orbit_proto_finalize")
    _lib.check(lib.orbit_proto_predict(_lib.dptr(qd), _lib.dptr(W), _lib.dptr(b), CFG_TASKS, M, 1, D, C, scale, 0,
                                       _lib.dptr(logits), None, _st()), "orbit_proto_predict")
    torch.cuda.synchronize()
    assert n_ids.cpu().tolist() == [C] * CFG_TASKS
    worst = 0.0
    for t in range(CFG_TASKS):
        x, lab, qt = c.feats[t].double(), c.labels[t], q[t].double()
        want_ids, W64, b64 = blocks.proto_configure(x, lab, "euclidean")
        assert ids[t].cpu().tolist() == want_ids == CFG_REAL[t]
        want = blocks.proto_predict(qt, W64, b64, scale, "euclidean")
        mu = W64 / 2
        n_c = torch.tensor([(lab == i).sum().item() for i in want_ids], dtype=torch.float64)[:, None]
        mean_abs = torch.stack([x[lab == i].abs().mean(0) for i in want_ids])
        dW = 2 * ((n_c + 2) * U * mean_abs + 2 * U * mu.abs())
        db = (mu.abs() * dW).sum(1) + (D / 256 + 12) * U * (mu * mu).sum(1)
        k = D / 64 + 8
        bound = abs(scale) * (2 * k * U * (qt.abs() @ W64.abs().t() + b64.abs()) + qt.abs() @ dW.t() + db)
        err = (logits[t].cpu().double() - want).abs()
        worst = max(worst, (err / bound).max().item())
        assert bool((err <= bound).all()), t
    print("chain: max error / bound = %.3f" % worst)


# ---- orbit_label_set, directly --------------------------------------------------------------------------------------------
def _label_set(lib, device, labels, cap):
    ld = labels.to(device) if len(labels) else torch.zeros(1, dtype=torch.int64, device=device)  # (N = 0: a valid pointer)
    ids = torch.full((cap,), -77, dtype=torch.int64, device=device)
    count = torch.full((1,), -77, dtype=torch.int32, device=device)
    _lib.check(lib.orbit_label_set(_lib.dptr(ld), len(labels), _lib.dptr(ids), cap, _lib.dptr(count), _st()), "label_set")
    torch.cuda.synchronize()
    return ids.cpu(), count.item()


def _check_label_set(lib, device, labels, cap):
    ids, count = _label_set(lib, device, labels, cap)
    want = torch.unique(labels)  # ascending
    if len(want) > cap:
        assert count == cap + 1
        assert torch.equal(ids, want[:cap])
        return
    assert count == len(want)
    assert torch.equal(ids[:count], want)
    fill = want[-1].item() if count else 0
    assert torch.equal(ids[count:], torch.full((cap - count,), fill, dtype=torch.int64))


def test_label_set_empty_and_single(lib, device):
    _check_label_set(lib, device, torch.zeros(0, dtype=torch.int64), 8)       # count 0, every slot 0
    _check_label_set(lib, device, torch.tensor([-3]), 8)
    _check_label_set(lib, device, torch.tensor([2 ** 40 + 1]), 1)


@pytest.mark.parametrize("N", [63, 64, 65, 1000])
def test_label_set_wave_edges_wide_values(lib, device, N):
    g = torch.Generator().manual_seed(N)
    vals = torch.tensor([-(2 ** 40) - 1, -7, -1, 0, 5, 2 ** 32, 2 ** 40 - 1, 2 ** 40, 2 ** 40 + 1, 2 ** 62])
    labels = vals[torch.randint(0, len(vals), (N,), generator=g)]
    labels[N - 1] = -(2 ** 40) - 1  # the smallest value only in the last position: lane (N - 1) % 64 of the last pass
    labels[:N - 1][labels[:N - 1] == -(2 ** 40) - 1] = -7
    _check_label_set(lib, device, labels, 32)
    _check_label_set(lib, device, labels, len(torch.unique(labels)))  # exactly full


def test_label_set_full_overflow_and_padding(lib, device):
    g = torch.Generator().manual_seed(8)
    for distinct, cap in ((8, 8), (9, 8), (20, 8), (3, 32)):  # exactly full; one too many; many too many; padding
        vals = (torch.randperm(1000, generator=g)[:distinct] - 500) * 3
        labels = vals[torch.randint(0, distinct, (300,), generator=g)]
        labels[:distinct] = vals
        ids, count = _label_set(lib, device, labels, cap)
        assert count == min(distinct, cap + 1)
        _check_label_set(lib, device, labels, cap)
        if distinct == 3:
            assert torch.equal(ids[3:], torch.full((29,), vals.max().item(), dtype=torch.int64))


# ---- poolers: what test_mean_pool_and_set_mean leaves out --------------------------------------------------------------------
def _pool_check(got, x_windows, T, what):
    """x_windows [rows][T][D]: the T inputs of every output row."""
    want = x_windows.double().mean(1)
    bound = (T + 1) * U * x_windows.double().abs().sum(1) / T
    err = (got.double() - want).abs()
    print("%s: max error / bound = %.3f" % (what, (err / bound.clamp_min(1e-300)).max().item()))
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("F,T,D", [(5, 8, 64),       # T > F: every window is clamped at frame 0
                                   (9, 1, 130),      # T = 1: the identity
                                   (20, 4, 130),     # D % 4 != 0
                                   (410, 3, 1280)])  # F D > 2048 x 256: the grid-stride loop iterates
def test_history_mean_pool_forms(lib, device, F, T, D):
    g = torch.Generator().manual_seed(F + T + D)
    x = torch.randn(F, D, generator=g)
    out = torch.full((F, D), float("nan"), device=device)
    xd = x.to(device)
    _lib.check(lib.orbit_history_mean_pool(_lib.dptr(xd), F, T, D, _lib.dptr(out), _st()), "history_mean_pool")
    src = (torch.arange(F)[:, None] - T + 1 + torch.arange(T)[None, :]).clamp_min(0)  # [F][T]
    windows = x[src]
    # the header: bit-identical to orbit_mean_pool over the T-times larger clip tensor
    clips = windows.reshape(F * T, D).contiguous().to(device)
    out2 = torch.full((F, D), float("nan"), device=device)
    _lib.check(lib.orbit_mean_pool(_lib.dptr(clips), F, T, D, _lib.dptr(out2), _st()), "mean_pool")
    torch.cuda.synchronize()
    _pool_check(out.cpu(), windows, T, "history_mean_pool F=%d T=%d D=%d" % (F, T, D))
    assert _same_bits(out.cpu(), out2.cpu())
    if T == 1:
        assert _same_bits(out.cpu(), x)


def test_mean_pool_past_the_block_cap(lib, device):
    N, T, D = 410, 2, 1280  # N D > 2048 blocks x 256 threads
    x = torch.randn(N * T, D, generator=torch.Generator().manual_seed(2))
    out = torch.full((N, D), float("nan"), device=device)
    xd = x.to(device)
    _lib.check(lib.orbit_mean_pool(_lib.dptr(xd), N, T, D, _lib.dptr(out), _st()), "mean_pool")
    torch.cuda.synchronize()
    _pool_check(out.cpu(), x.view(N, T, D), T, "mean_pool N=%d T=%d D=%d" % (N, T, D))


# ---- linear head parameter gradients -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 37])
@pytest.mark.parametrize("D", [100, 512, 1280])
@pytest.mark.parametrize("C", [5, 16, 17, 40])  # 17, 40: a second / third block of 16 classes
def test_linear_head_backward_forms(lib, device, C, D, M):
    """dW, db against fp64 autograd: M products per element in ascending row order, then the scale:
    |got - want| <= (M + 2) u |scale| sum_m |dl| |q|. With dbias = NULL the weight gradient keeps its bits."""
    scale = 1.7
    g = torch.Generator().manual_seed(C * 10000 + D * 10 + M)
    q, dl = torch.randn(M, D, generator=g), torch.randn(M, C, generator=g)
    Wp = torch.zeros(C, D, dtype=torch.float64, requires_grad=True)
    bp = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    (scale * (q.double() @ Wp.t() + bp)).backward(dl.double())
    qd, dld = q.to(device), dl.to(device)
    out = {}
    for with_bias in (True, False):
        dW = torch.full((C, D), float("nan"), device=device)
        db = torch.full((C,), float("nan"), device=device) if with_bias else None
        _lib.check(lib.orbit_linear_head_backward(_lib.dptr(dld), _lib.dptr(qd), M, D, C, scale, _lib.dptr(dW), _lib.dptr(db),
                                                  _st()), "orbit_linear_head_backward")
        torch.cuda.synchronize()
        out[with_bias] = (dW.cpu(), None if db is None else db.cpu())
    dW, db = out[True]
    bound_W = (M + 2) * U * abs(scale) * (dl.double().abs().t() @ q.double().abs())
    bound_b = (M + 2) * U * abs(scale) * dl.double().abs().sum(0)
    err_W, err_b = (dW.double() - Wp.grad).abs(), (db.double() - bp.grad).abs()
    print("linear head backward C=%d D=%d M=%d: max error / bound = %.3f (dW), %.3f (db)"
          % (C, D, M, (err_W / bound_W).max().item(), (err_b / bound_b).max().item()))
    assert bool((err_W <= bound_W).all()) and bool((err_b <= bound_b).all())
    assert _same_bits(out[False][0], dW)


# ---- argument guards ------------------------------------------------------------------------------------------------------------
def test_proto_head_refuses_too_many_tasks(lib, device):
    """n_tasks is a grid.y extent (at most 65535): refused with ORBIT_ERR_ARG before any launch, as configure does."""
    z = torch.zeros(64, device=device)
    zi = torch.zeros(8, dtype=torch.int64, device=device)
    big = 65536
    calls = {
        "proto_predict": lambda: lib.orbit_proto_predict(_lib.dptr(z), _lib.dptr(z), _lib.dptr(z), big, 1, 1, 4, 1, 1.0, 0,
                                                         _lib.dptr(z), None, _st()),
        "proto_finalize": lambda: lib.orbit_proto_finalize(_lib.dptr(z), _lib.dptr(z), big, 1, 4, 0, _lib.dptr(z),
                                                           _lib.dptr(z), _st()),
        "proto_configure": lambda: lib.orbit_proto_configure(_lib.dptr(z), _lib.dptr(zi), _lib.dptr(zi), big, 1, 1, 4, 1,
                                                             _lib.dptr(z), _lib.dptr(z), _st()),
    }
    for name, call in calls.items():
        assert call() == ERR_ARG, name
        msg = _lib.last_error()
        assert name in msg and "n_tasks" in msg, msg
    torch.cuda.synchronize()
    assert bool((z == 0).all())  # nothing ran


def test_head_options_back_at_default(lib, device):
    assert lib.orbit_get_option(b"head_stream") == 1
