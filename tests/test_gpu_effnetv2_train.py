"""The opt-in FiLM backward through the frozen efficientnet_v2_s end to end (ORBIT_PLAN_RES_POST_BACKWARD,
orbit_extractor_train_forward / orbit_extractor_backward, autograd.ExtractorFunction, EfficientNetV2S.native_backward) against the
float64 CPU pin (tests/effnetv2_pin.py with the FiLM dict through torch.func.functional_call and torch autograd).

Gradient gate, per FiLM tensor (tests/test_gpu_vit_ops.gate): max |got - ref64| <= max(4 * e32, 8 * 2**-24 * max |ref64|), e32 = the
fp32 pin's own gradient error against the float64 pin on the same inputs, measured here. Feature gate: that of
tests/test_gpu_effnetv2.py. The operators one by one: tests/test_gpu_effnetv2_train_ops.py.

Largest err / e32 seen on the MI355X (run with -s): 2.34 (70 x 54, B = 2); 2.30 at 64 x 64, 1.83 at 224 x 224; both call forms alike.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.func import functional_call

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import effnetv2_pin  # noqa: E402
from test_gpu_effnetv2 import FEAT_TOL, LOGIT_TOL, NAME, feat_err  # noqa: E402
from test_gpu_vit_ops import gate  # noqa: E402
from oracle.recogniser import OracleRecogniser  # noqa: E402
from orbit_dataset_amd import _lib, synthetic  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor  # noqa: E402
from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser  # noqa: E402

CASES = {"64x64": (64, 64, 3), "70x54": (70, 54, 2), "224x224": (224, 224, 1)}  # H, W, frames (70x54: both padding parities)
_CACHE = {}


def _pair():
    """(frozen HIP extractor on cuda:0 with FiLM tagging and native_backward = True, float32 CPU pin, float64 CPU pin, FiLM
    names): tests/test_gpu_effnetv2._pair with the opt-in."""
    if "pair" not in _CACHE:
        pin = effnetv2_pin.EfficientNet().eval()
        synthetic.init_parameters_(pin)
        pin64 = effnetv2_pin.EfficientNet().eval().double()
        pin64.load_state_dict(pin.state_dict())
        fe, film_names = create_feature_extractor(NAME, True, True, False)
        fe.load_state_dict(pin.state_dict(), strict=True)
        fe.cuda().eval()
        fe.native_backward = True
        for m in (pin, pin64):
            m.requires_grad_(False)
        _CACHE["pair"] = (fe, pin, pin64, film_names)
    return _CACHE["pair"]


def _case(key):
    """Frames, R, the 84 perturbed FiLM tensors and the pin's features / FiLM gradients of sum(feats * R) in float64, with the
    fp32 pin's errors against them; computed once per case."""
    if key not in _CACHE:
        fe, pin, pin64, film_names = _pair()
        H, W, B = CASES[key]
        g = torch.Generator().manual_seed(H * 1000 + W + 7)
        frames = torch.randn(B, 3, H, W, generator=g)
        R = torch.randn(B, 1280, generator=g)
        own = dict(pin.named_parameters())
        amp = 0.03
        film = {}
        for n in film_names:  # every one of the 84 tensors perturbed
            p = own[n].detach()
            film[n] = p * (1 + amp * torch.randn(p.shape, generator=g)) + 0.25 * amp * torch.randn(p.shape, generator=g)
        ref = {}
        for net, dtype in ((pin64, torch.float64), (pin, torch.float32)):
            leaves = {n: t.to(dtype).clone().requires_grad_(True) for n, t in film.items()}
            feats = functional_call(net, leaves, (frames.to(dtype),))
            (feats * R.to(dtype)).sum().backward()
            ref[dtype] = (feats.detach(), {n: t.grad.double() for n, t in leaves.items()})
        feats64, grads64 = ref[torch.float64]
        assert torch.isfinite(feats64).all() and feats64.abs().max().item() < 50, "pin features left the calibrated regime"
        e32 = {n: (ref[torch.float32][1][n] - grads64[n]).abs().max().item() for n in film_names}
        _CACHE[key] = dict(frames=frames, R=R, film=film, feats64=feats64, grads64=grads64, e32=e32,
                           feat_e32=feat_err(ref[torch.float32][0], feats64))
    return _CACHE[key]


def _slot_vectors(fe, film, device="cuda:0"):
    slots = [n for n, _ in fe.film_slot_modules()]
    gamma = torch.cat([film[s + ".weight"] for s in slots]).to(device)
    beta = torch.cat([film[s + ".bias"] for s in slots]).to(device)
    return slots, gamma, beta


def _split(fe, slots, dgamma, dbeta):
    """per-tensor gradients {name: tensor} from the two concatenated vectors"""
    out, off = {}, 0
    for s, (_, m) in zip(slots, fe.film_slot_modules()):
        C = m.weight.numel()
        out[s + ".weight"], out[s + ".bias"] = dgamma[off:off + C].cpu(), dbeta[off:off + C].cpu()
        off += C
    return out


def _film_form(fe, c, lo=0, hi=None):
    """the `film=` form on frames [lo:hi]: (features, per-tensor gradients of sum(feats * R))"""
    slots, gamma, beta = _slot_vectors(fe, c["film"])
    gamma.requires_grad_(True), beta.requires_grad_(True)
    feats = fe(c["frames"][lo:hi].cuda(), film=(gamma, beta))
    (feats * c["R"][lo:hi].cuda()).sum().backward()
    return feats.detach().cpu(), _split(fe, slots, gamma.grad, beta.grad)


def _gate_all(grads, c, what):
    worst = 0.0
    for n, ref in c["grads64"].items():
        assert grads[n] is not None, n
        worst = max(worst, gate(grads[n], ref, c["e32"][n], "%s %s" % (what, n)))
    print("\n[effnetv2-train] %s: largest err / e32 over the 84 tensors %.2f" % (what, worst))
    return worst


def _check_features(fe, c, feats, what):
    bound = max(FEAT_TOL, 4 * c["feat_e32"])
    slots, gamma, beta = _slot_vectors(fe, c["film"])
    with torch.no_grad():
        inference = fe(c["frames"].cuda(), film=(gamma, beta)).cpu()
    err, agree = feat_err(feats, c["feats64"]), feat_err(feats, inference)
    print("\n[effnetv2-train] %s: taped features err %.3g vs the float64 pin, %.3g vs the inference plan, E32 %.3g, bound %.3g"
          % (what, err, agree, c["feat_e32"], bound))
    assert torch.isfinite(feats).all()
    assert err <= bound and agree <= bound, (what, err, agree, bound)


@pytest.mark.parametrize("key", list(CASES))
def test_film_gradients_film_form(device, key):
    fe, _, _, _ = _pair()
    c = _case(key)
    feats, grads = _film_form(fe, c)
    _check_features(fe, c, feats, key + " film=")
    _gate_all(grads, c, key + " film=")


@pytest.mark.parametrize("key", list(CASES))
def test_film_gradients_functional_call_form(device, key):
    """The reference's mechanism (few_shot_recognisers.py:114-115): the 84 BatchNorm tensors swapped in by name, each a leaf that
    requires a gradient."""
    fe, _, _, _ = _pair()
    c = _case(key)
    leaves = {n: t.cuda().requires_grad_(True) for n, t in c["film"].items()}
    feats = functional_call(fe, leaves, (c["frames"].cuda(),))
    (feats * c["R"].cuda()).sum().backward()
    _check_features(fe, c, feats.detach().cpu(), key + " functional_call")
    _gate_all({n: (None if t.grad is None else t.grad.cpu()) for n, t in leaves.items()}, c, key + " functional_call")
    assert all(p.grad is None for p in fe.parameters())


def test_split_gradients_add_up_to_the_batch(device):
    """frames [0:2] and [2:3] through taped forwards of their own, gradients summed, against the B = 3 gradient: independence
    across the batch and across tapes."""
    fe, _, _, _ = _pair()
    c = _case("64x64")
    _, whole = _film_form(fe, c)
    _, a = _film_form(fe, c, 0, 2)
    _, b = _film_form(fe, c, 2, 3)
    worst = 0.0
    for n, ref in c["grads64"].items():
        summed = a[n].double() + b[n].double()
        tol = max(4 * c["e32"][n], 8 * 2.0 ** -24 * ref.abs().max().item())
        diff = (whole[n].double() - summed).abs().max().item()
        worst = max(worst, diff / tol)
        assert diff <= tol, (n, diff, tol)
    print("\n[effnetv2-train] split: largest |batch - (2 + 1 frames)| / tolerance %.3f" % worst)
    _gate_all({n: (a[n].double() + b[n].double()).float() for n in a}, c, "64x64 split 2 + 1")


def test_two_tapes_alive_at_once(device):
    """Two taped forwards before either backward (what a LITE step does: the subset's tape and the query batch's)."""
    fe, _, _, _ = _pair()
    c = _case("64x64")
    slots, gamma, beta = _slot_vectors(fe, c["film"])
    gamma.requires_grad_(True), beta.requires_grad_(True)
    x, R = c["frames"].cuda(), c["R"].cuda()
    f1 = fe(x[:2], film=(gamma, beta))
    f2 = fe(x[2:], film=(gamma, beta))
    ((f1 * R[:2]).sum() + (f2 * R[2:]).sum()).backward()
    _gate_all(_split(fe, slots, gamma.grad, beta.grad), c, "64x64 two live tapes")


def test_unfreeze_film_path_fills_the_84_batchnorm_grads(device):
    """The multi-step finetuner's route: no film vectors, the FiLM-slot BatchNorm Parameters themselves require a gradient."""
    from orbit_dataset_amd.model.film import unfreeze_film
    _, pin, pin64, _ = _pair()
    c = _case("64x64")
    fe, names = create_feature_extractor(NAME, with_film=True, learn_extractor=False)
    fe.load_state_dict(pin.state_dict(), strict=True)
    fe.cuda().eval()
    unfreeze_film(names, fe)
    fe.native_backward = True
    (fe(c["frames"].cuda()) * c["R"].cuda()).sum().backward()
    ref = {}
    for net, dtype in ((pin64, torch.float64), (pin, torch.float32)):
        leaves = {n: p.detach().clone().requires_grad_(True) for n, p in net.named_parameters() if n in names}
        (functional_call(net, leaves, (c["frames"].to(dtype),)) * c["R"].to(dtype)).sum().backward()
        ref[dtype] = {n: t.grad.double() for n, t in leaves.items()}
    params = dict(fe.named_parameters())
    assert len(names) == 84
    for n in names:
        assert params[n].grad is not None, n
        gate(params[n].grad.cpu(), ref[torch.float64][n], (ref[torch.float32][n] - ref[torch.float64][n]).abs().max().item(),
             "unfreeze_film " + n)
    assert all(p.grad is None for n, p in params.items() if n not in names)


def test_recogniser_lite_step(device):
    """SingleStepFewShotRecogniser(adapt_features, proto), 3-way at 64 x 64: one LITE step leaves finite, non-zero gradients on
    every FiLM-generator parameter and none on the extractor; its loss equals the loss of the same step computed with the float64
    pin injected into the oracle within the project's parity gate."""
    H = 4  # LITE subset: 4 of the 6 context frames re-encoded with a tape, 2 taken from the no-grad cache
    model = SingleStepFewShotRecogniser(NAME, True, "proto", 1, 8, False, H, 1.0)
    synthetic.init_parameters_(model)
    model.feature_extractor.native_backward = True
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(False)
    task = synthetic.make_task(3, way=3, shots=1, frames_per_shot=2, num_query=6, frame_size=64, template="blobs")
    ctx, lab, tgt, tlab = task["context_clips"], task["context_labels"], task["target_clips"], task["target_labels"]
    assert len(ctx) == 6 and len(lab.unique()) == 3
    np.random.seed(7)
    model.personalise_with_lite(ctx.cuda(), lab.cuda())
    loss = F.cross_entropy(model.predict_a_batch(tgt.cuda()), tlab.cuda())
    loss.backward()
    gen = [(n, p) for n, p in model.film_generator.named_parameters() if p.requires_grad]
    assert gen
    for n, p in gen:
        assert p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any()), n
    assert any(p.grad is not None and bool((p.grad != 0).any()) for p in model.set_encoder.parameters())
    assert all(p.grad is None for p in model.feature_extractor.parameters())
    # the same step in float64 on the CPU: the pin as the oracle's extractor
    ref = OracleRecogniser("resnet18", True, "proto", 1, 8, num_lite_samples=H)
    ref.fe = effnetv2_pin.EfficientNet().eval()
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    ref.fe.load_state_dict({k[len("feature_extractor."):]: v for k, v in sd.items() if k.startswith("feature_extractor.")})
    ref.fe.double()
    ref.set_encoder.load_state_dict({k[len("set_encoder."):]: v for k, v in sd.items() if k.startswith("set_encoder.")})
    ref.set_encoder.double()
    gen64 = ref.build_film_generator()
    gen64.load_state_dict({k[len("film_generator."):]: v for k, v in sd.items() if k.startswith("film_generator.")})
    gen64.double()
    np.random.seed(7)
    ref.personalise_with_lite(ctx.double(), lab)
    want = F.cross_entropy(ref.predict(tgt.double()), tlab).item()
    print("\n[effnetv2-train] LITE step loss %.6f, float64 oracle %.6f" % (loss.item(), want))
    assert abs(loss.item() - want) < LOGIT_TOL


def test_c_level_refusals_launch_nothing(device, lib):
    fe, _, _, _ = _pair()
    plan = fe._plan(64, 64, trainable=True)  # ORBIT_PLAN_UNFUSED | ORBIT_PLAN_RES_POST_BACKWARD
    fe.sync(plan)
    assert lib.orbit_extractor_supports_training(plan.handle) == 1
    B, dev = 2, "cuda:0"
    x = torch.zeros(B, 3, 64, 64, device=dev)
    feats, dfeats = torch.zeros(B, 1280, device=dev), torch.zeros(B, 1280, device=dev)
    tape = torch.empty(lib.orbit_extractor_tape_bytes(plan.handle, B), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.orbit_extractor_backward_workspace_bytes(plan.handle, B), dtype=torch.uint8, device=dev)
    flat = torch.zeros(lib.orbit_extractor_grad_floats(plan.handle), device=dev)
    torch.cuda.synchronize()

    def stats():
        a, b = ctypes.c_long(0), ctypes.c_long(0)
        lib.orbit_extractor_train_graph_stats(plan.handle, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    before = stats()
    tp, st = ctypes.c_void_p(tape.data_ptr()), _lib.stream_handle()
    rc = lib.orbit_extractor_train_forward(plan.handle, _lib.dptr(x), B, None, None, 1, 0.1, _lib.dptr(feats), tp, tape.numel(), st)
    assert rc != 0 and NAME in _lib.last_error() and "batch statistics" in _lib.last_error(), _lib.last_error()
    rc = lib.orbit_extractor_train_forward_ex(plan.handle, _lib.dptr(x), B, None, None, 1, 0.1, _lib.dptr(feats), tp, tape.numel(),
                                              1, st)
    assert rc != 0 and NAME in _lib.last_error()
    for bn_train, filter_grads in ((0, 1), (1, 0)):
        rc = lib.orbit_extractor_backward(plan.handle, _lib.dptr(x), B, None, None, bn_train, _lib.dptr(dfeats), tp, tape.numel(),
                                          _lib.dptr(flat), filter_grads, None, None, ctypes.c_void_p(ws.data_ptr()), ws.numel(), st)
        assert rc != 0 and NAME in _lib.last_error() and "filter gradients" in _lib.last_error(), _lib.last_error()
    assert stats() == before, "a refused call reached the training runtime"
    torch.cuda.synchronize()
    assert not feats.any() and not flat.any()
