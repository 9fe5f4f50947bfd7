"""GPU parity of the patch-16 transformer extractors (vit_s_16, vit_b_16, vit_b_16_clip; csrc/vit.hip at 197 tokens): features
against the Hugging Face fixture G17 and against the CPU pin (tests/vit16_pin.py) in float64, batch-size independence bit for
bit, the FiLM fast path, the recogniser end to end against OracleRecogniser with the pin injected as its extractor (the
project's parity gate: logits within 1e-3, identical argmax), and the refusal of everything that needs a gradient before any
launch. The two new kernels one by one: tests/test_gpu_vit16_ops.py.

The float64 gate is the stressed-parameter rule of tests/test_gpu_vit.py, min(4 * e32, FEAT_TOL) with e32 the fp32 CPU pin's
own error against the float64 pin on the same inputs. On the parameters of synthetic.init_parameters_ at their own scale
(factor 1: nothing had to be reduced) and the frames used here the fp32 pin is 2.6e-6 (vit_s_16, 5 frames), 2.4e-6 (vit_b_16,
2 frames) and 2.8e-6 (vit_b_16_clip, 2 frames) from the float64 pin, within FEAT_TOL / 4 = 2.5e-5; the test asserts that too."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch.func import functional_call

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import vit16_pin  # noqa: E402
from test_gpu_vit_ops import _prof_rows  # noqa: E402
from oracle import blocks  # noqa: E402
from oracle.recogniser import OracleRecogniser  # noqa: E402
from orbit_dataset_amd import synthetic  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor  # noqa: E402
from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FEAT_TOL = 1e-4   # tests/test_gpu_vit.py
LOGIT_TOL = 1e-3
NAMES = ("vit_s_16", "vit_b_16", "vit_b_16_clip")


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_golden_vit16_hf", os.path.join(HERE, "golden", "make_golden_vit16_hf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_CACHE = {}


def _pair(name):
    """(HIP extractor on cuda:0 with FiLM tagging, CPU pin) holding the same synthetic parameters; built once per model."""
    if name not in _CACHE:
        fe, _ = create_feature_extractor(name, with_film=True, learn_extractor=False)
        pin = vit16_pin.TimmViT16(name).eval()
        synthetic.init_parameters_(pin)
        fe.load_state_dict(pin.state_dict(), strict=True)
        fe.eval().to("cuda:0")
        _CACHE[name] = (fe, pin)
    return _CACHE[name]


def _film_vectors(fe, film):
    g = torch.cat([film[n + ".weight"].reshape(-1) for n, _ in fe.film_slot_modules()])
    b = torch.cat([film[n + ".bias"].reshape(-1) for n, _ in fe.film_slot_modules()])
    return g.cuda(), b.cuda()


@pytest.mark.parametrize("name", NAMES)
def test_G17_features_match_hugging_face(device, name):
    gen = _golden_module()
    g = np.load(os.path.join(HERE, "golden", "G17_vit16_hf.npz"))
    sd, frames, film = gen.inputs(name)
    # inputs regenerated here must be those the fixture was computed from (else this is generator drift, not a kernel error)
    for what, val in (("params", gen.checksum(sd)), ("frames", gen.checksum([frames])), ("film", gen.checksum(film))):
        np.testing.assert_allclose(val, g["%s_sum_%s" % (name, what)], rtol=1e-9, err_msg="G17 input drift: " + what)
    fe, _ = _pair(name)
    with torch.no_grad():
        plain = fe(frames.cuda()).cpu()
        filmed = fe(frames.cuda(), film=_film_vectors(fe, film)).cpu()
    assert (plain - torch.from_numpy(g[name + "_features"])).abs().max().item() <= FEAT_TOL
    assert (filmed - torch.from_numpy(g[name + "_features_film"])).abs().max().item() <= FEAT_TOL


_FRAMES = {}


def _frames():
    if "f" not in _FRAMES:
        _FRAMES["f"] = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(3))
    return _FRAMES["f"]


@pytest.mark.parametrize("name,sizes", [("vit_s_16", (1, 2, 5)), ("vit_b_16", (2,)), ("vit_b_16_clip", (2,))])
def test_features_match_the_float64_pin(device, name, sizes):
    """M = 197 B token rows: B = 1, 2, 5 leave row tails of 69, 10 and 89 rows in the 128-row GEMM tiles. Gate: the module
    docstring's."""
    fe, pin = _pair(name)
    B = max(sizes)
    frames = _frames()[:B]
    ref = vit16_pin.TimmViT16(name).eval()
    ref.load_state_dict(pin.state_dict())
    with torch.no_grad():
        fp32 = pin(frames)
        want = ref.double()(frames.double())
        e32 = (fp32.double() - want).abs().max().item()
        assert e32 <= FEAT_TOL / 4, "the fp32 pin itself is %.3g from the float64 pin: reduce the parameter scale" % e32
        tol = min(4 * e32, FEAT_TOL)
        for n in sizes:
            got = fe(frames[:n].cuda()).cpu()
            assert torch.isfinite(got).all()
            err = (got.double() - want[:n]).abs().max().item()
            print("\n[vit16] %s B=%d: err %.3g, fp32 pin %.3g, err / e32 %.2f" % (name, n, err, e32, err / e32))
            assert err <= tol, "%s B=%d: max |dfeature| = %.3g > %.3g (fp32 pin: %.3g)" % (name, n, err, tol, e32)


def test_features_do_not_depend_on_the_batch_and_film_paths_agree(device):
    """A frame's features are the same bits in batches of 1, 2 and 5; the FiLM fast path equals functional_call with the FiLM
    dict (the reference's mechanism) and the pin with the same dict; train() changes nothing."""
    fe, pin = _pair("vit_s_16")
    frames = _frames()
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        outs = {B: fe(frames[:B].cuda()).cpu() for B in (1, 2, 5)}
        for B in (1, 2):
            assert torch.equal(outs[B], outs[5][:B]), "features depend on the batch size (B=%d)" % B
        assert torch.equal(fe(frames[3:4].cuda()).cpu(), outs[5][3:4])
        film = {}
        for slot in pin.film_slot_names():
            film[slot + ".weight"] = (dict(pin.named_parameters())[slot + ".weight"]
                                      * (1 + 0.1 * torch.randn(pin.output_size, generator=gen)))
            film[slot + ".bias"] = 0.1 * torch.randn(pin.output_size, generator=gen)
        want_film = functional_call(pin, film, (frames[:2],))
        got_film = fe(frames[:2].cuda(), film=_film_vectors(fe, film)).cpu()
        assert (got_film - want_film).abs().max().item() <= FEAT_TOL
        assert (got_film - outs[2]).abs().max().item() > 0.1  # FiLM reaches the features
        via_call = functional_call(fe, {k: v.cuda() for k, v in film.items()}, (frames[:2].cuda(),)).cpu()
        assert torch.equal(via_call, got_film)
        fe.train()
        try:
            assert torch.equal(fe(frames[:2].cuda()).cpu(), outs[2])
        finally:
            fe.eval()


def test_forward_launches_the_197_token_kernels(device, lib):
    """The profiler's rows of one forward: the patch GEMM, the class-token row, 12 x (qkv, the 197-token attention, proj, fc1,
    fc2) and 25 LayerNorms - and no 50-token attention."""
    fe, _ = _pair("vit_s_16")
    x = _frames()[:2].cuda()
    with torch.no_grad():
        fe(x)
        torch.cuda.synchronize()
        lib.orbit_prof_enable(1)
        try:
            fe(x)
            torch.cuda.synchronize()
            rows = {r: n for r, n in _prof_rows(lib).items() if r.startswith("vit_") and n}
        finally:
            lib.orbit_prof_enable(0)
    want = {"vit_patch_embed<64>": 1, "vit_cls_token": 1, "vit_layernorm": 25, "vit_attention197": 12}
    want.update({"vit_%s<64>" % g: 12 for g in ("qkv", "proj", "fc1", "fc2")})
    assert rows == want, rows


def _recogniser_pair(name, adapt, classifier, batch_size=8):
    model = SingleStepFewShotRecogniser(name, adapt, classifier, 1, batch_size, False, 16, 1.0)
    synthetic.init_parameters_(model)
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(True)
    ref = OracleRecogniser("resnet18", adapt, classifier, 1, batch_size)  # then the pin replaces its extractor
    ref.fe = vit16_pin.TimmViT16(name).eval()
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    ref.fe.load_state_dict({k[len("feature_extractor."):]: v for k, v in sd.items() if k.startswith("feature_extractor.")})
    if classifier == "versa":
        D = ref.fe.output_size
        ref.weight_processor = blocks.DenseResidualBlock(D, D).eval()
        ref.bias_processor = blocks.DenseResidualBlock(D, 1).eval()
        ref.weight_processor.load_state_dict({k[len("classifier.weight_processor."):]: v for k, v in sd.items()
                                              if k.startswith("classifier.weight_processor.")})
        ref.bias_processor.load_state_dict({k[len("classifier.bias_processor."):]: v for k, v in sd.items()
                                            if k.startswith("classifier.bias_processor.")})
    if adapt:
        ref.set_encoder.load_state_dict({k[len("set_encoder."):]: v for k, v in sd.items() if k.startswith("set_encoder.")})
        gen = ref.build_film_generator()
        gen.load_state_dict({k[len("film_generator."):]: v for k, v in sd.items() if k.startswith("film_generator.")})
    return model, ref


_TASK = {}


def _task():
    """3-way, 2 context frames per class, 6 query frames"""
    if "t" not in _TASK:
        _TASK["t"] = synthetic.make_task(17, way=3, shots=1, frames_per_shot=2, num_query=6, frame_size=224)
    return _TASK["t"]


def _check(model, ref, host_clips=False, relative=False):
    t = _task()
    ctx, lab, tgt = t["context_clips"], t["context_labels"], t["target_clips"]
    with torch.no_grad():
        if host_clips:
            model.personalise(ctx, lab.cuda())
            logits = model.predict(tgt).cpu()
        else:
            model.personalise(ctx.cuda(), lab.cuda())
            logits = model.predict(tgt.cuda()).cpu()
    ref.personalise(ctx, lab)
    want = ref.predict(tgt)
    err = (logits - want).abs().max().item()
    # (Simple CNAPs logits are squared Mahalanobis distances, O(D): gated relative to their scale, as tests/test_gpu_vit.py)
    tol = LOGIT_TOL * max(1.0, want.abs().max().item()) if relative else LOGIT_TOL
    assert err < tol, "max |dlogit| = %g (tolerance %g)" % (err, tol)
    assert torch.equal(logits.argmax(1), want.argmax(1))
    model._reset()
    ref.reset()
    return logits


@pytest.mark.parametrize("classifier", ["proto", "proto_cosine", "versa", "mahalanobis"])
@pytest.mark.parametrize("adapt", [False, True])
def test_recogniser_vit_s_16_every_head(device, classifier, adapt):
    model, ref = _recogniser_pair("vit_s_16", adapt, classifier)
    assert model.feature_extractor.film_size == 25 * 384
    _check(model, ref, relative=classifier == "mahalanobis")


@pytest.mark.parametrize("name", ["vit_b_16", "vit_b_16_clip"])
def test_recogniser_vit_b_16_proto(device, name):
    model, ref = _recogniser_pair(name, True, "proto")
    _check(model, ref)


def test_overlap_query_matches_serial(device):
    """predict() on the second stream (host clips: overlap_query='auto' takes it) == the serial order, bit for bit."""
    model, ref = _recogniser_pair("vit_s_16", True, "proto")
    assert model.overlap_query == "auto"
    overlapped = _check(model, ref, host_clips=True)
    model.overlap_query = False
    serial = _check(model, ref, host_clips=True)
    assert torch.equal(overlapped, serial)


@pytest.mark.parametrize("opt_in", [(), ("native_backward",), ("native_weight_backward",)])
def test_grad_requiring_use_is_refused_before_any_launch(device, lib, opt_in):
    fe, _ = create_feature_extractor("vit_s_16", with_film=True, learn_extractor=True)
    fe.to("cuda:0")
    for attr in opt_in:
        setattr(fe, attr, True)
    x = torch.zeros(1, 3, 224, 224, device="cuda:0")
    lib.orbit_prof_enable(1)
    try:
        with pytest.raises(NotImplementedError, match="vit_s_16"):
            fe(x)
        assert not fe._plans, "a plan was built (parameters uploaded) before the refusal"
        fe.requires_grad_(False)
        g = torch.ones(fe.film_size, device="cuda:0", requires_grad=True)
        with pytest.raises(NotImplementedError, match="vit_s_16"):
            fe(x, film=(g, torch.zeros_like(g)))
        torch.cuda.synchronize()
        assert not any(n for r, n in _prof_rows(lib).items() if r.startswith("vit_")), "a refused forward launched a kernel"
    finally:
        lib.orbit_prof_enable(0)
    with torch.no_grad():
        assert fe(x).shape == (1, 384)  # the same module under no_grad runs
    with pytest.raises(ValueError, match="224"):
        with torch.no_grad():
            fe(torch.zeros(1, 3, 128, 128, device="cuda:0"))
