"""GPU parity of the prototype head (C-ABI) against the oracle restatement of classifier_heads.py, and the
size-independent properties that hold at BASELINE.json's full sizes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from oracle import blocks  # noqa: E402
from orbit_dataset_amd.model.classifier_heads import PrototypicalClassifier  # noqa: E402


def _task(N, M, D, way, seed, label_values=None, T=1):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(way, D, generator=g) * 0.3
    cls = torch.arange(way).repeat_interleave(N // way)[torch.randperm(N // way * way, generator=g)]
    feats = torch.relu(centers[cls].repeat_interleave(T, 0) + torch.randn(len(cls) * T, D, generator=g) * 0.5)
    qc = torch.randint(0, way, (M,), generator=g)
    q = torch.relu(centers[qc].repeat_interleave(T, 0) + torch.randn(M * T, D, generator=g) * 0.5)
    vals = torch.arange(way) if label_values is None else torch.tensor(label_values)
    return feats, vals[cls], q, vals[qc]


@pytest.mark.parametrize("D", [512, 1280, 100])
@pytest.mark.parametrize("way,label_values", [(5, None), (10, None), (3, (3, 7, 9))])
@pytest.mark.parametrize("dist,scale", [("euclidean", 1.0), ("cosine", 32.0)])
def test_head_matches_oracle(device, D, way, label_values, dist, scale):
    feats, labels, q, qlab = _task(200 // way * way, 200, D, way, seed=D + way, label_values=label_values)
    head = PrototypicalClassifier(scale, dist)
    head.configure(feats.to(device), labels.to(device))
    logits, amax = head.predict(q.to(device), return_argmax=True)
    ids, W, b = blocks.proto_configure(feats, labels, dist)
    want = blocks.proto_predict(q, W, b, scale, dist)
    assert head.class_ids.cpu().tolist() == ids
    assert (head.weight.cpu() - W).abs().max().item() < 1e-5
    if dist == "euclidean":
        assert (head.bias.cpu() - b).abs().max().item() < 1e-4 * max(1.0, b.abs().max().item())
    err = (logits.cpu() - want).abs().max().item()
    assert err < 1e-3, err
    assert torch.equal(logits.cpu().argmax(1), want.argmax(1))          # identical frame accuracy
    assert torch.equal(amax.cpu().long(), logits.cpu().argmax(1))       # fused argmax == argmax of its logits


@pytest.mark.parametrize("T", [1, 8])
def test_head_fused_pooling(device, T):
    """T frames per clip averaged inside the kernels == MeanPooler followed by the head (poolers.py:13-16)."""
    feats, labels, q, _ = _task(25, 40, 512, 5, seed=T, T=T)
    head = PrototypicalClassifier(1.0, "euclidean")
    head.configure(feats.to(device), labels.to(device), frames_per_clip=T)
    logits = head.predict(q.to(device), frames_per_clip=T).cpu()
    ids, W, b = blocks.proto_configure(blocks.mean_pool(feats, T), labels)
    want = blocks.proto_predict(blocks.mean_pool(q, T), W, b)
    assert (logits - want).abs().max().item() < 1e-3


def test_head_edge_cases(device):
    # zero query row under cosine -> exactly 0 (SURVEY §8c G1 edge), 1-shot (N == C), predict before configure
    head = PrototypicalClassifier(1.0, "cosine")
    with pytest.raises(AttributeError):
        head.predict(torch.zeros(2, 8, device=device))
    feats = torch.eye(5, 64)[:, :64] + 0.1
    labels = torch.arange(5)
    head.configure(feats.to(device), labels.to(device))
    q = torch.zeros(3, 64)
    q[1] = feats[2]
    logits = head.predict(q.to(device)).cpu()
    assert torch.all(logits[0] == 0) and torch.all(logits[2] == 0)
    assert logits[1].argmax().item() == 2 and abs(logits[1, 2].item() - 1.0) < 1e-6
    head.reset()
    with pytest.raises(AttributeError):
        head.predict(q.to(device))
    with pytest.raises(AssertionError):
        PrototypicalClassifier().configure(feats.to(device), labels[:4].to(device))


def test_head_full_size_properties(device):
    """At full size (ONE task with M = 64 x 200 query rows, D = 1280; batched launches: test_gpu_head_forms.py) check
    properties instead of an oracle run:
    (i) a query equal to prototype c scores highest on column c with logit mu.mu (euclidean: 2 mu.mu - mu.mu);
    (ii) logits are linear in logit_scale; (iii) permuting the support set leaves W, b unchanged up to fp32
    summation order."""
    g = torch.Generator().manual_seed(0)
    D, way, N = 1280, 10, 200
    feats = torch.rand(N, D, generator=g).to(device)
    labels = torch.arange(way).repeat_interleave(N // way).to(device)
    h1, h2 = PrototypicalClassifier(1.0), PrototypicalClassifier(4.0)
    h1.configure(feats, labels)
    h2.configure(feats, labels)
    mu = h1.weight / 2
    logits = h1.predict(mu)
    assert torch.equal(logits.argmax(1).cpu(), torch.arange(way))
    assert (logits.diagonal() + h1.bias).abs().max().item() < 1e-2      # mu.mu == -b
    q = torch.rand(64 * 200, D, generator=g).to(device)
    a, b = h1.predict(q), h2.predict(q)
    assert (4.0 * a - b).abs().max().item() < 1e-3
    perm = torch.randperm(N, generator=g).to(device)
    h3 = PrototypicalClassifier(1.0)
    h3.configure(feats[perm], labels[perm])
    assert (h3.weight - h1.weight).abs().max().item() < 1e-5


# ---- Versa / Mahalanobis heads -----------------------------------------------------------------
import os  # noqa: E402

import numpy as np  # noqa: E402

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold(name):
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" and v.ndim > 0 else v)
            for k, v in np.load(os.path.join(_GOLD, name + ".npz"), allow_pickle=False).items()}


@pytest.mark.parametrize("tag,D", [("w5", 64), ("single", 96)])
def test_G10_versa_head(device, tag, D):
    from orbit_dataset_amd import synthetic
    from orbit_dataset_amd.model.classifier_heads import VersaClassifier
    g = _gold("G10_heads_versa_mahalanobis")
    head = VersaClassifier(D, logit_scale=2.0)
    synthetic.init_parameters_(head, prefix="classifier.")
    head = head.to(device)
    head.configure(g[tag + "_features"].to(device), g[tag + "_labels"].to(device))
    assert (head.weight.cpu() - g[tag + "_versa_weight"]).abs().max().item() < 2e-5
    assert (head.bias.cpu() - g[tag + "_versa_bias"]).abs().max().item() < 2e-5
    logits = head.predict(g[tag + "_query"].to(device)).cpu()
    want = g[tag + "_versa_logits"]
    assert (logits - want).abs().max().item() < 1e-3
    assert torch.equal(logits.argmax(1), want.argmax(1))


@pytest.mark.parametrize("tag", ["w5", "single"])
def test_G10_mahalanobis_head(device, tag):
    from orbit_dataset_amd.model.classifier_heads import MahalanobisClassifier
    g = _gold("G10_heads_versa_mahalanobis")
    head = MahalanobisClassifier(1.0)
    head.configure(g[tag + "_features"].to(device), g[tag + "_labels"].to(device))
    assert (head.means.cpu() - g[tag + "_maha_means"]).abs().max().item() < 1e-5
    P = g[tag + "_maha_precisions"]
    assert (head.precisions.cpu() - P).abs().max().item() < 1e-4 * P.abs().max().item()
    TP = g[tag + "_maha_task_precision"]
    assert (head.task_precision.cpu() - TP).abs().max().item() < 1e-4 * TP.abs().max().item()
    logits = head.predict(g[tag + "_query"].to(device)).cpu()
    want = g[tag + "_maha_logits"]
    assert (logits - want).abs().max().item() < 1e-3 * want.abs().max().item()
    assert torch.equal(logits.argmax(1), want.argmax(1))


@pytest.mark.parametrize("D,way,shots,M", [(512, 5, 40, 200), (1280, 5, 40, 200), (512, 10, 7, 33)])
def test_versa_mahalanobis_at_extractor_width(device, D, way, shots, M):
    """Both heads at the extractors' feature widths (resnet18 512, efficientnet_b0 1280) against the oracle in fp64."""
    from oracle import blocks
    from orbit_dataset_amd import synthetic
    from orbit_dataset_amd.model.classifier_heads import MahalanobisClassifier, VersaClassifier
    g = torch.Generator().manual_seed(D + way)
    lab = torch.arange(way).repeat_interleave(shots)[torch.randperm(way * shots, generator=g)]
    centres = torch.randn(way, D, generator=g)
    feats = centres[lab] + 0.7 * torch.randn(way * shots, D, generator=g)
    q = centres[torch.randint(0, way, (M,), generator=g)] + 0.7 * torch.randn(M, D, generator=g)
    # Versa
    head = VersaClassifier(D, 1.0)
    synthetic.init_parameters_(head, prefix="classifier.")
    ref_w, ref_b = blocks.DenseResidualBlock(D, D), blocks.DenseResidualBlock(D, 1)
    ref_w.load_state_dict(head.weight_processor.state_dict()), ref_b.load_state_dict(head.bias_processor.state_dict())
    head = head.to(device)
    head.configure(feats.to(device), lab.to(device))
    with torch.no_grad():
        ids, W, b = blocks.versa_configure(feats.double(), lab, ref_w.double(), ref_b.double())
        want = q.double() @ W.t() + b
    assert (head.weight.cpu().double() - W).abs().max().item() < 1e-4 * W.abs().max().item()
    got = head.predict(q.to(device)).cpu().double()
    assert (got - want).abs().max().item() < 1e-4 * want.abs().max().item()
    assert torch.equal(got.argmax(1), want.argmax(1))
    # Mahalanobis
    maha = MahalanobisClassifier(1.0)
    maha.configure(feats.to(device), lab.to(device))
    ids, means, precisions, task_mean, task_precision = blocks.mahalanobis_configure(feats.double(), lab)
    assert (maha.precisions.cpu().double() - precisions).abs().max().item() < 1e-4 * precisions.abs().max().item()
    assert (maha.task_mean.cpu().double() - task_mean).abs().max().item() < 1e-5
    want = blocks.mahalanobis_predict(q.double(), means, precisions)
    got = maha.predict(q.to(device)).cpu().double()
    assert (got - want).abs().max().item() < 1e-3 * want.abs().max().item()
    assert torch.equal(got.argmax(1), want.argmax(1))


def test_spd_inverse(device):
    from orbit_dataset_amd import _lib
    lib = _lib.load()
    for n, batch in ((64, 3), (100, 2), (512, 2)):
        g = torch.Generator().manual_seed(n)
        a = torch.randn(batch, n, 2 * n, generator=g, dtype=torch.float64)
        A = a @ a.transpose(1, 2) / (2 * n) + torch.eye(n, dtype=torch.float64)
        t = A.float().to(device).contiguous()
        out = torch.empty_like(t)
        _lib.check(lib.orbit_spd_inverse(_lib.dptr(t), _lib.dptr(out), n, batch, _lib.stream_handle()), "orbit_spd_inverse")
        torch.cuda.synchronize()
        # the fp64 reference inverse on ONE thread (with the suite's 16 intra-op threads the host LAPACK of this image returned
        # a wrong batched inverse: diagonal entries below 1 / lambda_max) and, independently of any host inverse, the residual
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            want = torch.linalg.inv(A)
        finally:
            torch.set_num_threads(threads)
        assert (want @ A - torch.eye(n, dtype=torch.float64)).abs().max().item() < 1e-9
        assert (out.cpu().double() - want).abs().max().item() < 1e-5 * want.abs().max().item()
        assert (out.cpu().double() @ A - torch.eye(n, dtype=torch.float64)).abs().max().item() < 2e-5


def test_mahalanobis_predict_backward(device):
    from oracle import blocks
    from orbit_dataset_amd.model.classifier_heads import MahalanobisClassifier
    g = torch.Generator().manual_seed(5)
    D, way, shots, M = 512, 5, 12, 37
    lab = torch.arange(way).repeat_interleave(shots)
    feats = torch.randn(way, D, generator=g)[lab] + 0.7 * torch.randn(way * shots, D, generator=g)
    q = torch.randn(M, D, generator=g)
    dl = torch.randn(M, way, generator=g)
    head = MahalanobisClassifier(2.0)
    head.configure(feats.to(device), lab.to(device))
    qd = q.to(device).requires_grad_(True)
    head.predict(qd).backward(dl.to(device))
    qr = q.double().requires_grad_(True)
    blocks.mahalanobis_predict(qr, head.means.cpu().double(), head.precisions.cpu().double(), 2.0).backward(dl.double())
    assert (qd.grad.cpu().double() - qr.grad).abs().max().item() < 2e-5 * qr.grad.abs().max().item()


def test_many_pending_label_sets_keep_their_own_count(device):
    """label sets resolved on the side stream carried their class count through a shared ring of 64 pinned slots;
    with more than 64 of them pending, an earlier one read a later one's count. Each PendingLabelSet now owns a slot from a
    free list: 150 pending sets with class counts 1..9 all resolve to their own ids, dropped (never resolved) sets give their
    slot back, and a head configured on a pending set still exposes the exact weight / class_ids."""
    from orbit_dataset_amd.model.classifier_heads import PendingLabelSet
    dev = torch.device(device)
    g = torch.Generator().manual_seed(3)
    labels = []
    for i in range(150):
        c = 1 + i % 9
        vals = torch.randperm(40, generator=g)[:c].sort().values
        labels.append((vals, vals[torch.randint(0, c, (30,), generator=g)].scatter_(0, torch.arange(c), vals)))
    pend = [PendingLabelSet(lab.to(dev), dev) for _, lab in labels]
    slots = {(id(p.slot[0]), p.slot[1]) for p in pend}
    assert len(slots) == 150  # distinct slots while all are pending
    for (vals, _), p in zip(reversed(labels), reversed(pend)):  # resolve in the opposite order they were issued
        assert p.resolve().cpu().tolist() == vals.tolist()
        assert p.slot is None  # given back
    free_before = len(PendingLabelSet._free[str(dev)])
    dropped = [PendingLabelSet(lab.to(dev), dev) for _, lab in labels[:10]]
    assert len(PendingLabelSet._free[str(dev)]) == free_before - 10
    del dropped
    import gc
    gc.collect()
    assert len(PendingLabelSet._free[str(dev)]) == free_before
    # a head configured on a pending set, with 70 other sets issued before it is read
    feats, lab, q, _ = _task(60, 20, 64, 6, seed=11, label_values=(1, 4, 5, 8, 13, 21))
    head = PrototypicalClassifier(1.0, "euclidean")
    lab_dev = lab.to(dev)
    head.configure(feats.to(dev), lab_dev, class_ids=PrototypicalClassifier.label_set(lab_dev, dev))
    later = [PendingLabelSet(l.to(dev), dev) for _, l in labels[:70]]
    assert head.class_ids.cpu().tolist() == [1, 4, 5, 8, 13, 21] and head.weight.shape == (6, 64)
    ids, W, b = blocks.proto_configure(feats, lab, "euclidean")
    assert (head.weight.cpu() - W).abs().max().item() < 1e-5
    del later


# ---- orbit_dense_rows on its own, and the Mahalanobis head at widths that are no multiple of 32 --------------------------
_ACTS = {"none": 0, "relu": 1, "elu": 3}  # ORBIT_ACT_*


def _dense_ref(x, W, b, res, act, dtype):
    """act(x W^T + b) + res in plain torch at `dtype`."""
    y = torch.nn.functional.linear(x.to(dtype), W.to(dtype), None if b is None else b.to(dtype))
    y = {"none": y, "relu": torch.relu(y), "elu": torch.nn.functional.elu(y)}[act]
    return y if res is None else y + res.to(dtype)


def _dense_emulation(x, W, b, res, act):
    """dense_rows_kernel of csrc/heads_extra.hip restated in float32 in its own summation order: lane l of the wave of an
    output unit runs the fused multiply-add chain over k = l, l + 64, ..., then the 64 partial sums meet in the xor butterfly
    of wave_sum_xor (offsets 32, 16, ..., 1); bias, activation and residual follow in float32. A float32 fma is the float64
    product and sum rounded once more (the product of two float32 is exact in float64)."""
    xn, Wn = x.numpy().astype(np.float64), W.numpy().astype(np.float64)
    R, n_in = xn.shape
    acc = np.zeros((R, Wn.shape[0], 64), np.float32)
    for k0 in range(0, n_in, 64):
        n = min(64, n_in - k0)
        acc[:, :, :n] = (Wn[None, :, k0:k0 + n] * xn[:, None, k0:k0 + n] + acc[:, :, :n].astype(np.float64)).astype(np.float32)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, :, lanes ^ off]).astype(np.float32)
    v = acc[:, :, 0]
    if b is not None:
        v = (v + b.numpy()[None, :]).astype(np.float32)
    if act == "elu":
        v = np.where(v > 0, v, np.expm1(v)).astype(np.float32)
    elif act == "relu":
        v = np.maximum(v, np.float32(0))
    if res is not None:
        v = (v + res.numpy()).astype(np.float32)
    return torch.from_numpy(v)


@pytest.mark.parametrize("act", list(_ACTS))
def test_dense_rows_matches_fp64(device, act):
    """The few-rows dense layer of the Versa hyper-networks by itself, at row counts up to its limit of 16, input widths below,
    at and off the wave's 64 lanes and output counts that leave the last block of four waves partly empty, with and without
    bias and residual, against float64 under the gate of tests/test_gpu_vit_ops.py: max |got - ref64| <= max(4 e32, 8 * 2**-24
    max |ref64|), e32 the error of the plain float32 torch run on the CPU. x W^T ~ N(0, 1), so ELU and ReLU see both signs.
    The output is followed by a guard band. A case over its bound is reported with the same figures for _dense_emulation.
    On the MI355X (torch 2.10 CPU reference, 16 threads) the largest err / e32 is 1.11 where 4 e32 sets the bound; where the
    floor does, e32 is the rounding error of few numbers and the ratio says little: 2.67 at most, but for four cases of a single
    number (R = out = 1, in = 64) at 5.20, 12.48, 25.44 and 84.56 with err at most 1.5e-7. Every case meets the gate as it
    stands, so no factor is widened."""
    from orbit_dataset_amd import _lib
    from test_gpu_vit_ops import gate
    _lib.require_gpu()
    lib = _lib.load()
    g = torch.Generator().manual_seed(17)
    worst, guard, failures = [0.0, 0.0], 64, []
    for R in (1, 7, 16):
        for n_in in (5, 64, 193):
            for n_out in (1, 6, 129):
                x, W = torch.randn(R, n_in, generator=g), torch.randn(n_out, n_in, generator=g) / n_in ** 0.5
                bias, resid = 0.5 * torch.randn(n_out, generator=g), torch.randn(R, n_out, generator=g)
                xd, Wd = x.to(device), W.to(device)
                for b, res in ((bias, resid), (bias, None), (None, resid), (None, None)):
                    ref64 = _dense_ref(x, W, b, res, act, torch.float64)
                    pre = _dense_ref(x, W, b, None, "none", torch.float64)
                    assert R * n_out < 8 or pre.min().item() < 0 < pre.max().item()  # both branches of the activation
                    e32 = (_dense_ref(x, W, b, res, act, torch.float32).double() - ref64).abs().max().item()
                    y = torch.full((R * n_out + guard,), 7777.0, device=device)
                    bd, rd = (None if b is None else b.to(device)), (None if res is None else res.to(device))
                    _lib.check(lib.orbit_dense_rows(_lib.dptr(xd), R, n_in, _lib.dptr(Wd), _lib.dptr(bd), n_out, _ACTS[act],
                                                    _lib.dptr(rd), _lib.dptr(y), _lib.stream_handle()), "orbit_dense_rows")
                    torch.cuda.synchronize()
                    y = y.cpu()
                    assert torch.all(y[R * n_out:] == 7777.0) and not (y[:R * n_out] == 7777.0).any()
                    got = y[:R * n_out].view(R, n_out)
                    what = "dense_rows %s R %d in %d out %d%s%s" % (act, R, n_in, n_out, " bias" if b is not None else "",
                                                                    " residual" if res is not None else "")
                    floor = 8 * 2.0 ** -24 * ref64.abs().max().item()
                    try:
                        ratio = gate(got, ref64, e32, what)
                        worst[4 * e32 < floor] = max(worst[4 * e32 < floor], ratio)
                    except AssertionError as e:
                        emu = _dense_emulation(x, W, b, res, act)
                        failures.append("%s (the emulation of the kernel's summation order: err %.4g, |kernel - emulation| %.4g)"
                                        % (str(e).split("\n")[0], (emu.double() - ref64).abs().max().item(),
                                           (got - emu).abs().max().item()))
    print("[head] dense_rows %s largest err / e32: %.2f where 4 e32 is the bound, %.2f where the floor is" % (act, *worst))
    assert not failures, "\n".join(failures)


def test_dense_rows_refuses_17_rows(device):
    from orbit_dataset_amd import _lib
    _lib.require_gpu()
    lib = _lib.load()
    x, W, y = torch.zeros(17, 8, device=device), torch.zeros(4, 8, device=device), torch.full((17 * 4,), 7777.0, device=device)
    assert lib.orbit_dense_rows(_lib.dptr(x), 17, 8, _lib.dptr(W), None, 4, 0, None, _lib.dptr(y), _lib.stream_handle()) != 0
    assert "dense_rows: bad sizes (rows must be 1..16)" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.all(y == 7777.0)


@pytest.mark.parametrize("D", [36, 100])
def test_mahalanobis_at_widths_off_the_32_tile(device, D):
    """configure -> predict -> predict_backward at feature widths that are multiples of 4 but not of 32: the covariance kernel's
    column guards and the ragged last block of the blocked Gauss-Jordan inverse run together. 37 examples in five classes with
    non-contiguous label values, one class with a single example (the reference's scalar 'covariance'). Tolerances: those of
    test_G10_mahalanobis_head, test_versa_mahalanobis_at_extractor_width and test_mahalanobis_predict_backward."""
    from oracle import blocks
    from orbit_dataset_amd.model.classifier_heads import MahalanobisClassifier
    g = torch.Generator().manual_seed(D)
    values = torch.tensor([2, 5, 11, 12, 40])
    cls = torch.tensor([0] * 10 + [1] * 9 + [2] * 1 + [3] * 9 + [4] * 8)[torch.randperm(37, generator=g)]
    assert cls.numel() == 37 and (cls == 2).sum().item() == 1
    lab = values[cls]
    centres = torch.randn(5, D, generator=g)
    feats = centres[cls] + 0.7 * torch.randn(37, D, generator=g)
    M = 23
    q = centres[torch.randint(0, 5, (M,), generator=g)] + 0.7 * torch.randn(M, D, generator=g)
    dl = torch.randn(M, 5, generator=g)
    head = MahalanobisClassifier(2.0)
    head.configure(feats.to(device), lab.to(device))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (the float64 inverses: see test_spd_inverse)
    try:
        ids, means, precisions, task_mean, task_precision = blocks.mahalanobis_configure(feats.double(), lab)
    finally:
        torch.set_num_threads(threads)
    assert head.class_ids.cpu().tolist() == ids.tolist() == values.tolist()
    assert (head.means.cpu().double() - means).abs().max().item() < 1e-5
    assert (head.task_mean.cpu().double() - task_mean).abs().max().item() < 1e-5
    assert (head.precisions.cpu().double() - precisions).abs().max().item() < 1e-4 * precisions.abs().max().item()
    assert (head.task_precision.cpu().double() - task_precision).abs().max().item() < 1e-4 * task_precision.abs().max().item()
    want = blocks.mahalanobis_predict(q.double(), means, precisions, 2.0)
    got = head.predict(q.to(device)).cpu().double()
    assert got.shape == (M, 5)
    assert (got - want).abs().max().item() < 1e-3 * want.abs().max().item()
    assert torch.equal(got.argmax(1), want.argmax(1))
    qd = q.to(device).requires_grad_(True)
    head.predict(qd).backward(dl.to(device))
    qr = q.double().requires_grad_(True)
    blocks.mahalanobis_predict(qr, head.means.cpu().double(), head.precisions.cpu().double(), 2.0).backward(dl.double())
    assert (qd.grad.cpu().double() - qr.grad).abs().max().item() < 2e-5 * qr.grad.abs().max().item()
