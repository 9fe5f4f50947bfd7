"""GPU parity of the transformer extractors at other frame sizes than 224 (orbit_vit_create_sized;
VisionTransformer.resample_pos_embed): features of sized plans, plain and with FiLM vectors, against the sized CPU pin
(tests/vit_sized_pin.py: the existing pins with the position table resampled by torch's bicubic) in float64; a sized plan at 224
against an orbit_vit_create plan bit for bit; the resampled table following a parameter upload; bf16 on a sized plan; the module
and the recogniser end to end. The three new kernels one by one: tests/test_gpu_vit_sized_ops.py.

Gates, imported and unchanged: features min(4 * e32, FEAT_TOL) with the e32 <= FEAT_TOL / 4 precondition (tests/test_gpu_vit16.py;
e32 the fp32 CPU pin's own error against the float64 pin on the same inputs), bf16 16 e32 < err <= 4 e_bf
(tests/test_gpu_vit_bf16.py, tests/vit_bf16_emulation.py applied to the sized pin), logits LOGIT_TOL and identical argmax.

Largest err / e32 seen on the MI355X (every case prints its ratio; run with -s): 2.26 (vit_b_16_clip at 48x48, FiLM); the fp32
pins are 2.4e-6 .. 8.0e-6 from their float64 selves. bf16 at 80x80: err / e_bf 0.99 (err 0.0222), 6 200 x the fp32 pin's error.
"""
import ctypes

import pytest
import torch
from torch.func import functional_call

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import vit_sized_pin  # noqa: E402
from oracle.recogniser import OracleRecogniser  # noqa: E402
from orbit_dataset_amd import _lib, synthetic  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor  # noqa: E402
from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser  # noqa: E402
from test_gpu_vit16 import FEAT_TOL, LOGIT_TOL  # noqa: E402
from test_gpu_vit_ops import _prof_rows  # noqa: E402
from vit_bf16_emulation import emulate_bf16_linears  # noqa: E402


def _st():
    return _lib.stream_handle()


class Plan:
    """an orbit_vit_* plan driven through the C-ABI: orbit_vit_create_sized at S x S, or (S None) orbit_vit_create at 224"""

    def __init__(self, lib, name, S, params=None, bf16=False):
        self.lib, self.h = lib, ctypes.c_void_p()
        if S is None:
            _lib.check(lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(self.h)), "orbit_vit_create")
        else:
            _lib.check(lib.orbit_vit_create_sized(name.encode(), S, S, ctypes.byref(self.h)), "orbit_vit_create_sized")
        self.D = lib.orbit_vit_output_size(self.h)
        if bf16:
            _lib.check(lib.orbit_vit_enable_bf16(self.h), "orbit_vit_enable_bf16")
        if params is not None:
            self.load(params)

    def load(self, params):
        tensors = list(params.values())
        ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        _lib.check(self.lib.orbit_vit_load_all_async(self.h, ptrs, len(tensors), _st()), "orbit_vit_load_all_async")
        _lib.check(self.lib.orbit_vit_finalize(self.h, _st()), "orbit_vit_finalize")

    def features(self, frames, film=None):
        n = frames.shape[0]
        nbytes = self.lib.orbit_vit_workspace_bytes(self.h, n)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=frames.device)
        feats = torch.full((n, self.D), float("nan"), device=frames.device)
        g, b = film if film is not None else (None, None)
        _lib.check(self.lib.orbit_vit_forward(self.h, _lib.dptr(frames), n, _lib.dptr(g), _lib.dptr(b), _lib.dptr(feats),
                                              ctypes.c_void_p(ws.data_ptr()), ws.numel(), _st()), "orbit_vit_forward")
        torch.cuda.synchronize()
        return feats.cpu()

    def close(self):
        if self.h:
            self.lib.orbit_vit_destroy(self.h)
            self.h = None


_PINS = {}


def _pins(name):
    """per model, built once and left unchanged: the sized pin with synthetic parameters, its float64 copy, a FiLM dict"""
    if name not in _PINS:
        pin = vit_sized_pin.SizedViT(name).eval()
        synthetic.init_parameters_(pin)
        ref = vit_sized_pin.SizedViT(name).eval()
        ref.load_state_dict(pin.state_dict())
        ref = ref.double()
        gen = torch.Generator().manual_seed(21)
        own = dict(pin.named_parameters())
        film = {}
        for slot in pin.film_slot_names():
            film[slot + ".weight"] = (own[slot + ".weight"] * (1 + 0.1 * torch.randn(pin.output_size, generator=gen))).detach()
            film[slot + ".bias"] = 0.1 * torch.randn(pin.output_size, generator=gen)
        _PINS[name] = (pin, ref, film)
    return _PINS[name]


def _device_params(pin, scale=None):
    return {k: (v if scale is None else v * scale(k)).float().contiguous().cuda() for k, v in pin.state_dict().items()}


def _film_vectors(pin, film):
    g = torch.cat([film[n + ".weight"].reshape(-1) for n in pin.film_slot_names()])
    b = torch.cat([film[n + ".bias"].reshape(-1) for n in pin.film_slot_names()])
    return g.cuda(), b.cuda()


def _frames(S, B, seed=3):
    return torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(seed + S))


def _feature_gate(got, want, e32, what):
    assert e32 <= FEAT_TOL / 4, "%s: the fp32 pin itself is %.3g from the float64 pin" % (what, e32)
    assert torch.isfinite(got).all(), what
    err = (got.double() - want).abs().max().item()
    print("\n[vit-sized] %s: err %.3g, fp32 pin %.3g, err / e32 %.2f" % (what, err, e32, err / e32))
    tol = min(4 * e32, FEAT_TOL)
    assert err <= tol, "%s: max |dfeature| = %.3g > %.3g (fp32 pin: %.3g)" % (what, err, tol, e32)


CASES = [("vit_s_32", 64, 3), ("vit_s_32", 96, 3), ("vit_s_32", 256, 3), ("vit_s_16", 32, 2), ("vit_s_16", 80, 2),
         ("vit_s_16", 128, 2), ("vit_s_16", 256, 2), ("vit_b_32_clip", 96, 2), ("vit_b_16_clip", 48, 2)]


@pytest.mark.parametrize("name,S,B", CASES, ids=["%s-%d" % c[:2] for c in CASES])
def test_features_of_sized_plans_match_the_float64_pin(lib, device, name, S, B):
    """plain and with FiLM vectors; a frame's features are the same bits alone and in the batch; the kernels a sized forward
    launches"""
    pin, ref, film = _pins(name)
    frames = _frames(S, B)
    tokens = (S // vit_sized_pin.patch_of(name)) ** 2 + 1
    film64 = {k: v.double() for k, v in film.items()}
    with torch.no_grad():
        want, fp32 = ref(frames.double()), pin(frames)
        want_film, fp32_film = functional_call(ref, film64, (frames.double(),)), functional_call(pin, film, (frames,))
    plan = Plan(lib, name, S, _device_params(pin))
    try:
        x = frames.cuda()
        got = plan.features(x)
        lib.orbit_prof_enable(1)
        try:
            again = plan.features(x)
            rows = {r: n for r, n in _prof_rows(lib).items() if r.startswith("vit_") and n}
        finally:
            lib.orbit_prof_enable(0)
        got_film = plan.features(x, _film_vectors(pin, film))
        alone = plan.features(x[:1].contiguous())
    finally:
        plan.close()
    what = "%s %dx%d (%d tokens) B=%d" % (name, S, S, tokens, B)
    _feature_gate(got, want, (fp32.double() - want).abs().max().item(), what)
    _feature_gate(got_film, want_film, (fp32_film.double() - want_film).abs().max().item(), what + " FiLM")
    assert (got_film - got).abs().max().item() > 0.1  # FiLM reaches the features
    assert torch.equal(got, again) and torch.equal(alone, got[:1]), "features depend on the batch"
    # the second forward: no resample (the table is made once per upload), the runtime-geometry patch GEMM, the streaming
    # attention unless the token count is one the specialised kernels own
    attn = {50: "vit_attention", 197: "vit_attention197"}.get(tokens, "vit_attention_n")
    assert rows.get(attn) == 12 and "vit_pos_resample" not in rows, rows
    assert [r for r in rows if "patch_embed" in r] == ["vit_patch_embed_sized<64>"], rows
    assert not ({"vit_attention", "vit_attention197", "vit_attention_n"} - {attn}) & set(rows), rows


@pytest.mark.parametrize("name", ["vit_s_32", "vit_s_16"])
def test_a_sized_plan_at_224_is_the_default_plan(lib, device, name):
    pin, _, film = _pins(name)
    p = _device_params(pin)
    x = _frames(224, 2).cuda()
    sized, plain = Plan(lib, name, 224, p), Plan(lib, name, None, p)
    try:
        a = sized.features(x)
        lib.orbit_prof_enable(1)
        try:
            sized.features(x)
            rows = {r for r, n in _prof_rows(lib).items() if r.startswith("vit_") and n}
        finally:
            lib.orbit_prof_enable(0)
        b = plain.features(x)
        fa, fb = sized.features(x, _film_vectors(pin, film)), plain.features(x, _film_vectors(pin, film))
    finally:
        sized.close()
        plain.close()
    assert torch.equal(a, b) and torch.equal(fa, fb)
    assert "vit_patch_embed<64>" in rows and not any("sized" in r or r in ("vit_attention_n", "vit_pos_resample") for r in rows), rows


def test_parameter_upload_invalidates_the_resampled_table(lib, device):
    """forward, orbit_vit_load_all_async of other weights (another position table among them), forward again == a fresh plan"""
    name, S = "vit_s_32", 96
    pin, _, _ = _pins(name)
    x = _frames(S, 2).cuda()
    old = _device_params(pin)
    new = _device_params(pin, scale=lambda k: 1.5 if k == "pos_embed" else 1.25 if k.endswith("mlp.fc2.weight") else 1.0)
    only_pos = _device_params(pin, scale=lambda k: 1.5 if k == "pos_embed" else 1.0)
    plan, fresh, fresh_pos = Plan(lib, name, S, old), Plan(lib, name, S, new), Plan(lib, name, S, only_pos)
    try:
        first = plan.features(x)
        lib.orbit_prof_enable(1)
        try:
            plan.load(new)
            second = plan.features(x)
            rows = {r: n for r, n in _prof_rows(lib).items() if r.startswith("vit_") and n}
        finally:
            lib.orbit_prof_enable(0)
        want = fresh.features(x)
        plan.load(only_pos)
        third, want_pos = plan.features(x), fresh_pos.features(x)
    finally:
        plan.close()
        fresh.close()
        fresh_pos.close()
    assert rows.get("vit_pos_resample") == 1, rows
    assert not torch.equal(first, second) and not torch.equal(second, third) and not torch.equal(first, third)
    assert torch.equal(second, want) and torch.equal(third, want_pos), "a forward after a parameter upload used a stale table"


def test_bf16_on_a_sized_plan(lib, device):
    """vit_s_16 at 80 x 80 (26 tokens), 3 frames: the two-sided gate of tests/test_gpu_vit_bf16.py on the sized pin"""
    name, S, B = "vit_s_16", 80, 3
    pin, ref, _ = _pins(name)
    emu = vit_sized_pin.SizedViT(name).eval()
    emu.load_state_dict(pin.state_dict())
    emu = emulate_bf16_linears(emu.double())
    frames = _frames(S, B, seed=11)
    with torch.no_grad():
        ref64, emu64, fp32 = ref(frames.double()), emu(frames.double()), pin(frames)
    e_bf, e32 = (emu64 - ref64).abs().max().item(), (fp32.double() - ref64).abs().max().item()
    p = _device_params(pin)
    plan, plain = Plan(lib, name, S, p, bf16=True), Plan(lib, name, S, p)
    try:
        assert lib.orbit_vit_bf16_enabled(plan.h) == 1
        got = plan.features(frames.cuda())
        lib.orbit_prof_enable(1)
        try:
            again = plan.features(frames.cuda())
            rows = {r: n for r, n in _prof_rows(lib).items() if r.startswith("vit_") and n}
        finally:
            lib.orbit_prof_enable(0)
        fp = plain.features(frames.cuda())
    finally:
        plan.close()
        plain.close()
    assert torch.equal(got, again) and torch.isfinite(got).all()
    gemm = {r: n for r, n in rows.items() if "<" in r and "patch_embed" not in r}
    assert gemm == {"vit_%s_bf16<64>" % g: 12 for g in ("qkv", "proj", "fc1", "fc2")}, rows
    assert rows.get("vit_attention_n") == 12 and rows.get("vit_patch_embed_sized<64>") == 1, rows
    err = (got.double() - ref64).abs().max().item()
    print("\n[vit-sized] bf16 %s %dx%d: |got - ref64| %.3g, e_bf %.3g (ratio %.2f), fp32 pin e32 %.3g, fp32 plan %.3g"
          % (name, S, S, err, e_bf, err / e_bf, e32, (fp.double() - ref64).abs().max().item()))
    assert err <= 4 * e_bf, "max |got - ref64| = %.3g > 4 e_bf = %.3g" % (err, 4 * e_bf)
    assert err > 16 * e32, "%.3g from the float64 pin is fp32 accuracy (fp32 pin: %.3g): the flag did nothing" % (err, e32)


def test_module_attribute_runs_the_sized_plan(lib, device):
    """VisionTransformer.resample_pos_embed at 96 x 96 == the C-ABI plan, bit for bit; at 224 == the default; set after plans
    exist; without it the ValueError stands"""
    name, S = "vit_s_32", 96
    pin, _, film = _pins(name)
    fe, _ = create_feature_extractor(name, with_film=True, learn_extractor=False)
    fe.load_state_dict(pin.state_dict(), strict=True)
    fe.eval().to("cuda:0")
    x, x224 = _frames(S, 2).cuda(), _frames(224, 2).cuda()
    with torch.no_grad():
        default = fe(x224).cpu()  # (a plan exists before the attribute is set)
        with pytest.raises(ValueError, match="224"):
            fe(x)
        fe.resample_pos_embed = True
        got = fe(x).cpu()
        got_film = fe(x, film=_film_vectors(pin, film)).cpu()
        assert torch.equal(fe(x224).cpu(), default)
        assert set(fe._plans) == {(224, 224, False), (224, 224, False, "sized"), (S, S, False, "sized")}
        with pytest.raises(ValueError, match="multiple"):
            fe(torch.zeros(1, 3, 80, 80, device="cuda:0"))
        fe.resample_pos_embed = False
        with pytest.raises(ValueError, match="224"):
            fe(x)
    plan = Plan(lib, name, S, _device_params(pin))
    try:
        assert torch.equal(got, plan.features(x)) and torch.equal(got_film, plan.features(x, _film_vectors(pin, film)))
    finally:
        plan.close()
    # a gradient at another size is refused before any launch
    fe.resample_pos_embed = fe.native_backward = True
    g = torch.ones(fe.film_size, device="cuda:0", requires_grad=True)
    lib.orbit_prof_enable(1)
    try:
        with pytest.raises(NotImplementedError, match="resample_pos_embed"):
            fe(x, film=(g, torch.zeros_like(g)))
        torch.cuda.synchronize()
        assert not any(n for r, n in _prof_rows(lib).items() if r.startswith("vit_")), "a refused forward launched a kernel"
    finally:
        lib.orbit_prof_enable(0)


def test_recogniser_at_96(lib, device):
    """SingleStepFewShotRecogniser with vit_s_32 on a 3-way synthetic task of 96 x 96 frames against OracleRecogniser with the
    sized pin injected as its extractor: logits within LOGIT_TOL, identical argmax (tests/test_gpu_vit16.py at 224)."""
    name = "vit_s_32"
    model = SingleStepFewShotRecogniser(name, False, "proto", 1, 8, False, 16, 1.0)
    synthetic.init_parameters_(model)
    model.feature_extractor.resample_pos_embed = True
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(True)
    ref = OracleRecogniser("resnet18", False, "proto", 1, 8)  # then the sized pin replaces its extractor
    ref.fe = vit_sized_pin.SizedViT(name).eval()
    ref.fe.load_state_dict({k[len("feature_extractor."):]: v.cpu() for k, v in model.state_dict().items()
                            if k.startswith("feature_extractor.")})
    t = synthetic.make_task(17, way=3, shots=1, frames_per_shot=2, num_query=6, frame_size=96)
    ctx, lab, tgt = t["context_clips"], t["context_labels"], t["target_clips"]
    with torch.no_grad():
        model.personalise(ctx.cuda(), lab.cuda())
        logits = model.predict(tgt.cuda()).cpu()
    ref.personalise(ctx, lab)
    want = ref.predict(tgt)
    err = (logits - want).abs().max().item()
    print("\n[vit-sized] recogniser at 96x96: max |dlogit| %.3g" % err)
    assert err < LOGIT_TOL, "max |dlogit| = %g" % err
    assert torch.equal(logits.argmax(1), want.argmax(1))
    assert list(model.feature_extractor._plans) == [(96, 96, False, "sized")]
    model._reset()


def test_learner_flag_reaches_the_extractor_and_the_test_stats(lib, device):
    """--vit_resample_pos_embed on both learners: --frame_size goes to the task source, the extractor carries the attribute, the
    test loop runs to its stats, which name the frame size the plan ran at."""
    from orbit_dataset_amd import learner
    argv = ["--feature_extractor", "vit_s_16", "--mode", "test", "--classifier", "proto", "--way", "2", "--shots", "1",
            "--frames_per_shot", "2", "--num_query_videos", "1", "--frames_per_video", "3", "--batch_size", "8", "--num_test_tasks", "1",
            "--frame_size", "64", "--vit_resample_pos_embed"]
    L = learner.Learner(learner.build_parser().parse_args(argv))
    assert L.model.feature_extractor.resample_pos_embed is True
    stats = L.test()
    assert stats["vit_frame_size"] == [64, 64] and stats["num_tasks"] == 1 and stats["vit_precision"] == "fp32"
    assert list(L.model.feature_extractor._plans) == [(64, 64, False, "sized")]
    with pytest.raises(SystemExit, match="needs --frame_size 224"):
        learner.Learner(learner.build_parser().parse_args(argv[:-1]))
    M = learner.MultiStepLearner(learner.build_multistep_parser().parse_args(
        argv[:4] + argv[6:] + ["--personalize_num_grad_steps", "2"]))
    assert M.model.feature_extractor.resample_pos_embed is True and M.test()["vit_frame_size"] == [64, 64]
