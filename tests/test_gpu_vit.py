"""GPU parity of the transformer extractors (csrc/vit.hip): features against the Hugging Face fixture G15 and the live CPU pin
(tests/vit_pin.py), batch-size independence - also across the GEMM tile-height switch, at the 256 / 448 frames where every
128-row instantiation runs - the FiLM fast path, parameters stressed towards a trained ViT (peaked attention, outlier channels,
LayerNorm variance near eps) against the pin in float64, and the recogniser end to end against OracleRecogniser with the pin
injected as its extractor (logits within 1e-3, identical argmax: the project's parity gate). The kernels one by one:
tests/test_gpu_vit_ops.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from torch.func import functional_call

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import vit_pin  # noqa: E402
from test_gpu_vit_ops import _prof_rows  # noqa: E402
from oracle import blocks  # noqa: E402
from oracle.recogniser import OracleRecogniser  # noqa: E402
from orbit_dataset_amd import synthetic  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor  # noqa: E402
from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FEAT_TOL = 1e-4
LOGIT_TOL = 1e-3
NAMES = ("vit_s_32", "vit_b_32", "vit_b_32_clip")


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_golden_vit_hf", os.path.join(HERE, "golden", "make_golden_vit_hf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_CACHE = {}


def _pair(name):
    """(HIP extractor on cuda:0 with FiLM tagging, CPU pin) holding the same synthetic parameters; built once per model."""
    if name not in _CACHE:
        fe, _ = create_feature_extractor(name, with_film=True, learn_extractor=False)
        pin = vit_pin.TimmViT(name).eval()
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
def test_G15_features_match_hugging_face(device, name):
    gen = _golden_module()
    g = np.load(os.path.join(HERE, "golden", "G15_vit_hf.npz"))
    sd, frames, film = gen.inputs(name)
    # inputs regenerated here must be those the fixture was computed from (else this is generator drift, not a kernel error)
    for what, val in (("params", gen.checksum(sd)), ("frames", gen.checksum([frames])), ("film", gen.checksum(film))):
        np.testing.assert_allclose(val, g["%s_sum_%s" % (name, what)], rtol=1e-9, err_msg="G15 input drift: " + what)
    fe, _ = _pair(name)
    with torch.no_grad():
        plain = fe(frames.cuda()).cpu()
        filmed = fe(frames.cuda(), film=_film_vectors(fe, film)).cpu()
    assert (plain - torch.from_numpy(g[name + "_features"])).abs().max().item() <= FEAT_TOL
    assert (filmed - torch.from_numpy(g[name + "_features_film"])).abs().max().item() <= FEAT_TOL


@pytest.mark.parametrize("name,sizes", [("vit_s_32", (1, 3, 67)), ("vit_b_32", (1, 67)), ("vit_b_32_clip", (3, 67))])
def test_features_match_cpu_pin_and_do_not_depend_on_the_batch(device, name, sizes):
    """M = 50 B token rows: B = 1, 3, 67 leave row tails in every GEMM tile height. The token GEMM accumulates every output
    element in the same k order whatever M or the tile height, so a frame's features are BITWISE equal alone and in a batch."""
    fe, pin = _pair(name)
    gen = torch.Generator().manual_seed(3)
    frames = torch.randn(max(sizes), 3, 224, 224, generator=gen)
    with torch.no_grad():
        want = pin(frames)
        film = {}
        for slot in pin.film_slot_names():
            film[slot + ".weight"] = (dict(pin.named_parameters())[slot + ".weight"]
                                      * (1 + 0.1 * torch.randn(pin.output_size, generator=gen)))
            film[slot + ".bias"] = 0.1 * torch.randn(pin.output_size, generator=gen)
        want_film = functional_call(pin, film, (frames[:3],))
        gf = _film_vectors(fe, film)
        outs = {}
        for B in sizes:
            got = fe(frames[:B].cuda()).cpu()
            err = (got - want[:B]).abs().max().item()
            assert err <= FEAT_TOL, (B, err)
            outs[B] = got
        got_film = fe(frames[:3].cuda(), film=gf).cpu()
        assert (got_film - want_film).abs().max().item() <= FEAT_TOL
        big = outs[max(sizes)]
        for B in sizes:
            assert torch.equal(outs[B], big[:B]), "features depend on the batch size (B=%d)" % B
        alone = fe(frames[5:6].cuda()).cpu()
        assert torch.equal(alone, big[5:6])
        # FiLM fast path == functional_call with the FiLM dict (the reference's mechanism)
        film_dev = {k: v.cuda() for k, v in film.items()}
        via_call = functional_call(fe, film_dev, (frames[:3].cuda(),)).cpu()
        assert torch.equal(via_call, got_film)
        # train() changes nothing: no BatchNorm, no dropout
        fe.train()
        try:
            assert torch.equal(fe(frames[:3].cuda()).cpu(), big[:3])
        finally:
            fe.eval()


GEMMS = ("patch_embed", "qkv", "proj", "fc1", "fc2")


@pytest.mark.parametrize("name,B", [("vit_b_32", 256), ("vit_s_32", 448), ("vit_b_32_clip", 256)])
def test_features_across_the_tile_height_switch(device, lib, name, B):
    """At 256 (ViT-B) / 448 (ViT-S) frames every token GEMM and the patch embedding take the 128-row tile; the same frames in
    chunks of 67 take the 64-row tile (but ViT-B's fc1). The profiling rows say which ran, and every chunk's features are
    BITWISE the matching rows of the big run: the 67-frame path is pinned to the CPU reference above, and equality carries
    that to the tall kernels (3 frames of the big run are also compared with the pin directly)."""
    fe, pin = _pair(name)
    frames = torch.randn(B, 3, 224, 224, device=device, generator=torch.Generator(device=device).manual_seed(5))
    with torch.no_grad():
        lib.orbit_prof_enable(1)
        try:
            big = fe(frames)
            torch.cuda.synchronize()
            rows = {r: n for r, n in _prof_rows(lib).items() if r.endswith(">")}
            assert rows == dict([("vit_patch_embed<128>", 1)] + [("vit_%s<128>" % g, 12) for g in GEMMS[1:]]), rows
            lib.orbit_prof_enable(1)
            chunks = [(i, fe(frames[i:i + 67])) for i in range(0, B, 67)]
            torch.cuda.synchronize()
            rows = {r: n for r, n in _prof_rows(lib).items() if r.endswith(">")}
        finally:
            lib.orbit_prof_enable(0)
        n = len(chunks)
        want_rows = {"vit_patch_embed<64>": n}
        for g in GEMMS[1:]:
            want_rows["vit_%s<%d>" % (g, 128 if g == "fc1" and name != "vit_s_32" else 64)] = 12 * n
        assert rows == want_rows, rows
        for i, got in chunks:
            assert torch.equal(got, big[i:i + 67]), "frames %d.. differ between a 67-frame batch and the %d-frame batch" % (i, B)
        err = (big[:3].cpu() - pin(frames[:3].cpu())).abs().max().item()
        assert err <= FEAT_TOL, err


QK_FACTOR, POS_BUMP, POS_CHANNELS, SMALL = 1.75, 8.0, (3, 77, 190, 301), 1e-3


def _stressed(name, sd, case):
    """Parameters edited after init_parameters_. The factors were chosen on the CPU so that 4 x the fp32 pin's own error (the
    gate below) stays within FEAT_TOL on all three models. Case 'peaked': attention logits reach +-15 (mean top probability
    0.47) and four residual channels sit at 8 in a stream of std 1 .. 1.6; the fp32 pin is 0.7e-5 / 1.3e-5 / 1.1e-5 (ViT-S /
    ViT-B / CLIP) from the float64 pin (at a q/k factor of 2 it is 3.2e-5 on ViT-B, at 2.5 above 1e-4: peaked attention
    amplifies rounding, so the factor stops here). Case 'near_eps': token variance ~1e-6 at the first LayerNorms; the fp32 pin is
    0.33e-5 / 0.38e-5 / 0.38e-5 off, and the in21k / CLIP eps exchanged move the features by 1.4 .. 2.1 (5e-4 unstressed)."""
    sd = {k: v.clone() for k, v in sd.items()}
    D = vit_pin.VIT[name][0]
    if case == "peaked":
        for k in sd:
            if k.endswith("attn.qkv.weight") or k.endswith("attn.qkv.bias"):
                sd[k][:2 * D] *= QK_FACTOR  # the q and k rows
        sd["pos_embed"][..., list(POS_CHANNELS)] += POS_BUMP
    else:
        for k in ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"):
            if k in sd:
                sd[k] *= SMALL
    return sd


@pytest.mark.parametrize("case", ["peaked", "near_eps"])
@pytest.mark.parametrize("name", NAMES)
def test_stressed_parameters_match_the_float64_pin(device, name, case):
    """Gate: 4 x the fp32 CPU pin's own error against the float64 pin on the same inputs (the reasoning of
    tests/test_gpu_vit_ops.py), never looser than FEAT_TOL."""
    fe, pin = _pair(name)
    base = {k: v.clone() for k, v in pin.state_dict().items()}
    sd = _stressed(name, base, case)
    frames = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(11))
    ref = vit_pin.TimmViT(name).eval()
    ref.load_state_dict(sd)
    with torch.no_grad():
        fp32 = ref(frames)
        want = ref.double()(frames.double())
        e32 = (fp32.double() - want).abs().max().item()
        tol = min(4 * e32, FEAT_TOL)
        try:
            fe.load_state_dict(sd, strict=True)
            got = fe(frames.cuda()).cpu()
        finally:
            fe.load_state_dict(base, strict=True)
    err = (got.double() - want).abs().max().item()
    print("\n[vit-stress] %s %s: err %.3g, fp32 pin %.3g, err / e32 %.2f" % (name, case, err, e32, err / e32))
    assert torch.isfinite(got).all()
    assert err <= tol, "%s %s: max |dfeature| = %.3g > %.3g (fp32 pin: %.3g)" % (name, case, err, tol, e32)


def _recogniser_pair(name, adapt, classifier, batch_size=8):
    model = SingleStepFewShotRecogniser(name, adapt, classifier, 1, batch_size, False, 16, 1.0)
    synthetic.init_parameters_(model)
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(True)
    ref = OracleRecogniser("resnet18", adapt, classifier, 1, batch_size)  # then the pin replaces its extractor
    ref.fe = vit_pin.TimmViT(name).eval()
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
    if "t" not in _TASK:
        _TASK["t"] = synthetic.make_task(15, way=3, shots=1, frames_per_shot=4, num_query=9, frame_size=224)
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
    # (Simple CNAPs logits are squared Mahalanobis distances, O(D): gated relative to their scale, as the existing
    # end-to-end test of that head does - tests/test_gpu_recogniser.py)
    tol = LOGIT_TOL * max(1.0, want.abs().max().item()) if relative else LOGIT_TOL
    assert err < tol, "max |dlogit| = %g (tolerance %g)" % (err, tol)
    assert torch.equal(logits.argmax(1), want.argmax(1))
    model._reset()
    ref.reset()
    return logits


@pytest.mark.parametrize("classifier", ["proto", "proto_cosine", "versa", "mahalanobis"])
@pytest.mark.parametrize("adapt", [False, True])
def test_recogniser_vit_s_32_every_head(device, classifier, adapt):
    model, ref = _recogniser_pair("vit_s_32", adapt, classifier)
    _check(model, ref, relative=classifier == "mahalanobis")


@pytest.mark.parametrize("name", ["vit_b_32", "vit_b_32_clip"])
def test_recogniser_vit_b_proto(device, name):
    model, ref = _recogniser_pair(name, True, "proto")
    _check(model, ref)


def test_overlap_query_matches_serial(device):
    """predict() on the second stream (host clips: overlap_query='auto' takes it) == the serial order, bit for bit."""
    model, ref = _recogniser_pair("vit_s_32", True, "proto")
    assert model.overlap_query == "auto"
    overlapped = _check(model, ref, host_clips=True)
    model.overlap_query = False
    serial = _check(model, ref, host_clips=True)
    assert torch.equal(overlapped, serial)


def test_grad_requiring_use_is_refused_before_any_launch(device):
    fe, _ = create_feature_extractor("vit_s_32", with_film=True, learn_extractor=True)
    fe.to("cuda:0")
    x = torch.zeros(1, 3, 224, 224, device="cuda:0")
    with pytest.raises(NotImplementedError, match="vit_s_32"):
        fe(x)
    assert not fe._plans, "a plan was built (parameters uploaded) before the refusal"
    with torch.no_grad():
        assert fe(x).shape == (1, 384)  # the same module under no_grad runs
    fe.requires_grad_(False)
    g = torch.ones(fe.film_size, device="cuda:0", requires_grad=True)
    with pytest.raises(NotImplementedError):
        fe(x, film=(g, torch.zeros_like(g)))
    with pytest.raises(ValueError, match="224"):
        with torch.no_grad():
            fe(torch.zeros(1, 3, 128, 128, device="cuda:0"))


def test_learner_test_mode_vit_b_32_clip_over_a_jpeg_directory(device, tmp_path):
    """single-step-learner.py --mode test --feature_extractor vit_b_32_clip --classifier proto --data_root DIR: the test loop
    over a synthetic JPEG tree, with the reference's CLIP frame normalisation (utils/args.py:185-190)."""
    import json
    import subprocess
    import sys
    from orbit_dataset_amd.data import pipeline
    tree = str(tmp_path / "test")
    pipeline.write_synthetic_orbit_directory(tree, users=2, objects_per_user=2, clean_videos=2, clutter_videos=1,
                                             frames_per_video=50, frame_size=224)
    res = tmp_path / "res.json"
    root = os.path.dirname(HERE)
    cmd = [sys.executable, os.path.join(root, "single-step-learner.py"), "--mode", "test", "--feature_extractor",
           "vit_b_32_clip", "--classifier", "proto", "--data_root", tree, "--num_workers", "3", "--subsample_factor", "5",
           "--batch_size", "64", "--results_path", str(res)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(res) as f:
        stats = json.load(f)
    assert stats["num_tasks"] == 2 and stats["target_frames"] == 2 * 2 * 1 * 50
    assert stats["frame_acc"][0] is not None
