"""GPU parity of the efficientnet_v2_s extractor (csrc/extractor.hip build_efficientnet_v2_s) against the CPU pin
(tests/effnetv2_pin.py) evaluated in float64: features at even, odd / non-square and 224 x 224 frame sizes and at batch sizes 1,
3 and 37, both plan flags, both FiLM call forms, the recogniser end to end with the pin injected as the oracle's extractor
(logits within 1e-3, identical argmax: the project's parity gate), and the refusal of every use that needs a gradient.

Gate on the features: `feat_err` of tests/test_gpu_extractors.py (absolute on O(1) features, relative to the largest feature
beyond that) at most max(FEAT_TOL, 4 x E32), where E32 is the same measure for the pin run in float32 on the CPU against the
float64 pin on the same inputs and FEAT_TOL = 2e-5 is the project's bound for the convolutional extractors. The factor 4 covers
a different summation order and the hardware exp / rcp in SiLU on a network twice as deep as efficientnet_b0. Each test prints
E32 and the error it observed."""
import pytest
import torch
from torch.func import functional_call

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import effnetv2_pin  # noqa: E402
from test_gpu_vit_ops import _prof_rows  # noqa: E402
from oracle.recogniser import OracleRecogniser  # noqa: E402
from orbit_dataset_amd import _lib, synthetic  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import _Plan, create_feature_extractor  # noqa: E402
from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser  # noqa: E402

NAME = "efficientnet_v2_s"
FEAT_TOL = 2e-5
LOGIT_TOL = 1e-3
SIZES = {"64x64": (64, 64, 37), "70x54": (70, 54, 3), "224x224": (224, 224, 2)}  # H, W, frames


def feat_err(got, want):
    return (got.double() - want.double()).abs().max().item() / max(1.0, want.abs().max().item())


_CACHE = {}


def _pair():
    """(HIP extractor on cuda:0 with FiLM tagging, float32 CPU pin, float64 CPU pin, FiLM names), same synthetic parameters."""
    if "pair" not in _CACHE:
        pin = effnetv2_pin.EfficientNet().eval()
        synthetic.init_parameters_(pin)
        pin64 = effnetv2_pin.EfficientNet().eval().double()
        pin64.load_state_dict(pin.state_dict())
        fe, film_names = create_feature_extractor(NAME, True, True, False)
        fe.load_state_dict(pin.state_dict(), strict=True)
        _CACHE["pair"] = (fe.cuda().eval(), pin, pin64, film_names)
    return _CACHE["pair"]


def _reference(key):
    """frames, the float64 pin's features and E32 for one entry of SIZES; computed once."""
    if key not in _CACHE:
        _, pin, pin64, _ = _pair()
        H, W, n = SIZES[key]
        x = torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
        with torch.no_grad():
            want = pin64(x.double())
            e32 = feat_err(pin(x), want)
        assert torch.isfinite(want).all() and want.abs().max().item() < 50, "pin features left the calibrated regime"
        _CACHE[key] = (x, want, e32)
    return _CACHE[key]


def _bound(e32):
    return max(FEAT_TOL, 4 * e32)


@pytest.mark.parametrize("key", list(SIZES))
def test_features_match_the_float64_pin(device, key):
    fe, _, _, _ = _pair()
    x, want, e32 = _reference(key)
    with torch.no_grad():
        got = fe(x.to(device)).cpu()
    assert got.shape == (len(x), 1280) and torch.isfinite(got).all()
    err = feat_err(got, want)
    print("\n[effnetv2] %s x %d frames: err %.3g, E32 %.3g, bound %.3g (feature max %.3f)"
          % (key, len(x), err, e32, _bound(e32), want.abs().max().item()))
    assert err <= _bound(e32), (key, err, e32)


def test_batch_sizes_1_3_37(device):
    fe, _, _, _ = _pair()
    x, want, e32 = _reference("64x64")
    outs = {}
    with torch.no_grad():
        for B in (1, 3, 37):
            outs[B] = fe(x[:B].to(device)).cpu()
            err = feat_err(outs[B], want[:B])
            print("\n[effnetv2] 64x64 batch %d: err %.3g, E32 %.3g" % (B, err, e32))
            assert err <= _bound(e32), (B, err, e32)
    for B in (1, 3):  # frame i agrees across batches
        assert feat_err(outs[B], outs[37][:B]) <= _bound(e32), B


@pytest.mark.parametrize("key", ["64x64", "70x54"])
def test_plan_unfused_flag_gives_the_same_features(device, key):
    """ORBIT_PLAN_UNFUSED (the flag a tape-recording plan is built with): the plan holds no fused op, so the flag changes
    nothing - same bound against the pin, and the bits of the default plan."""
    fe, _, _, _ = _pair()
    x, want, e32 = _reference(key)
    H, W, n = SIZES[key]
    n = min(n, 3)
    with torch.no_grad():
        default = fe(x[:n].to(device)).cpu()
        saved, fe._plans = fe._plans, {(H, W, False): _Plan(NAME, H, W, trainable=True)}  # create_ex(..., ORBIT_PLAN_UNFUSED)
        try:
            got = fe(x[:n].to(device)).cpu()
        finally:
            for p in fe._plans.values():
                p.destroy()
            fe._plans = saved
    err = feat_err(got, want[:n])
    print("\n[effnetv2] %s ORBIT_PLAN_UNFUSED: err %.3g, E32 %.3g" % (key, err, e32))
    assert err <= _bound(e32)
    assert torch.equal(got, default)


def test_film_both_call_forms_match_functional_call_on_the_pin(device):
    """Per-task FiLM, every one of the 84 tensors perturbed: `functional_call` by name (the reference's mechanism,
    few_shot_recognisers.py:114-115) and the fast `film=` path each match the pin under functional_call."""
    fe, pin, pin64, film_names = _pair()
    amp = 0.03
    g = torch.Generator().manual_seed(11)
    params = dict(pin.named_parameters())
    film = {}
    for n_ in film_names:
        p = params[n_].detach()
        film[n_] = p * (1 + amp * torch.randn(p.shape, generator=g)) + 0.25 * amp * torch.randn(p.shape, generator=g)
    x = _reference("64x64")[0][:4]
    with torch.no_grad():
        want = functional_call(pin64, {k: v.double() for k, v in film.items()}, (x.double(),))
        plain = pin64(x.double())
        e32 = feat_err(functional_call(pin, film, (x,)), want)
    assert (want - plain).abs().max().item() > 1e-2  # FiLM really changes the features
    assert torch.isfinite(want).all() and want.abs().max().item() < 50
    film_dev = {k: v.to(device) for k, v in film.items()}
    with torch.no_grad():
        got_fc = functional_call(fe, film_dev, (x.to(device),)).cpu()
        slots = [n_ for n_, _ in fe.film_slot_modules()]
        gamma = torch.cat([film_dev[s + ".weight"] for s in slots])
        beta = torch.cat([film_dev[s + ".bias"] for s in slots])
        got_fast = fe(x.to(device), film=(gamma, beta)).cpu()
        back = fe(x.to(device)).cpu()
    print("\n[effnetv2] FiLM: functional_call err %.3g, film= err %.3g, E32 %.3g"
          % (feat_err(got_fc, want), feat_err(got_fast, want), e32))
    assert feat_err(got_fc, want) <= _bound(e32)
    assert feat_err(got_fast, want) <= _bound(e32)
    assert feat_err(back, plain) <= _bound(_reference("64x64")[2])  # and the un-FiLMed path is untouched


def _recogniser_pair(adapt, classifier, batch_size=8):
    model = SingleStepFewShotRecogniser(NAME, adapt, classifier, 1, batch_size, False, 16, 1.0)
    synthetic.init_parameters_(model)
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(True)
    ref = OracleRecogniser("resnet18", adapt, classifier, 1, batch_size)  # then the pin replaces its extractor
    ref.fe = effnetv2_pin.EfficientNet().eval()
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    ref.fe.load_state_dict({k[len("feature_extractor."):]: v for k, v in sd.items() if k.startswith("feature_extractor.")})
    if adapt:
        ref.set_encoder.load_state_dict({k[len("set_encoder."):]: v for k, v in sd.items() if k.startswith("set_encoder.")})
        gen = ref.build_film_generator()
        gen.load_state_dict({k[len("film_generator."):]: v for k, v in sd.items() if k.startswith("film_generator.")})
    return model, ref


@pytest.mark.parametrize("classifier", ["proto", "proto_cosine"])
@pytest.mark.parametrize("adapt", [False, True])
def test_recogniser_matches_the_heads_fed_with_the_pins_features(device, classifier, adapt):
    """5-way, 10 support clips, 12 query clips at 64 x 64: personalise -> predict against the oracle recogniser whose extractor
    is the pin (with adapt_features: set encoder -> FiLM generator -> FiLMed extractor on both sides). The task is of the
    low-frequency "blobs" family: "identical argmax" only means something where the oracle's own best and second-best logit
    are further apart than both sides' logit bounds together (2 x LOGIT_TOL), which the test checks on the oracle's logits -
    cosine logits of this uncalibrated network on white-noise frames are 1e-6 apart."""
    if "task" not in _CACHE:
        _CACHE["task"] = synthetic.make_task(5, way=5, shots=1, frames_per_shot=2, num_query=12, frame_size=64, template="blobs")
    t = _CACHE["task"]
    ctx, lab, tgt = t["context_clips"], t["context_labels"], t["target_clips"]
    assert len(ctx) == 10 and len(tgt) == 12 and len(lab.unique()) == 5
    model, ref = _recogniser_pair(adapt, classifier)
    with torch.no_grad():
        model.personalise(ctx.cuda(), lab.cuda())
        logits = model.predict(tgt.cuda()).cpu()
    ref.personalise(ctx, lab)
    want = ref.predict(tgt)
    top2 = want.topk(2, dim=1).values
    assert (top2[:, 0] - top2[:, 1]).min().item() > 2 * LOGIT_TOL, "the oracle's own argmax is not decided on this task"
    err = (logits - want).abs().max().item()
    print("\n[effnetv2] recogniser %s adapt=%s: max |dlogit| %.3g" % (classifier, adapt, err))
    assert err < LOGIT_TOL, "max |dlogit| = %g" % err
    assert torch.equal(logits.argmax(1), want.argmax(1))


def test_grad_requiring_use_is_refused_before_any_launch(device, lib):
    fe, _ = create_feature_extractor(NAME, with_film=True, learn_extractor=True)
    fe.to("cuda:0").eval()
    x = torch.zeros(1, 3, 64, 64, device="cuda:0")
    torch.cuda.synchronize()
    lib.orbit_prof_enable(1)
    try:
        with pytest.raises(NotImplementedError, match=NAME):
            fe(x)  # own parameters require a gradient
        fe.requires_grad_(False)
        g = torch.ones(fe.film_size, device="cuda:0", requires_grad=True)
        with pytest.raises(NotImplementedError, match=NAME):
            fe(x, film=(g, torch.zeros_like(g)))  # FiLM gradients
        fe.train()
        with torch.no_grad(), pytest.raises(NotImplementedError, match=NAME):
            fe(x)  # batch-statistics BatchNorm
        fe.eval()
        torch.cuda.synchronize()
        rows = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    assert sum(rows.values()) == 0, rows
    assert not fe._plans, "a plan was built (parameters uploaded) before the refusal"
    with torch.no_grad():
        assert fe(x).shape == (1, 1280)  # the same module, frozen, in eval() under no_grad runs
