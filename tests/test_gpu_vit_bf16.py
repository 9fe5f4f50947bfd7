"""The opt-in bf16 inference plan of the transformer extractors (orbit_vit_enable_bf16; VisionTransformer.bf16_inference) on
vit_s_32, vit_s_16 and vit_b_32_clip (the pre-norm variant), 3 frames each.

Wiring is tested exactly: the forward of a bf16 plan must be torch.equal to the same forward driven from this file through the
single-operator entry points (orbit_op_vit_patch_embed_p, _layernorm, _linear_bf16 on weights packed by orbit_op_vit_pack_bf16,
_attention_tokens), with and without FiLM - a wrong weight offset, a layer left in fp32 or a stale bf16 copy cannot hide in a
tolerance. The operator itself is tests/test_gpu_vit_bf16_ops.py's job.

The SIZE of the precision trade is gated against the pin in float64: ref64 = the pin in float64, emu64 = the same model with
every qkv / proj / fc1 / fc2 weight and input rounded to bf16 (tests/vit_bf16_emulation.py), e_bf = max |emu64 - ref64|, and

    16 e32_model  <  max |got - ref64|  <=  4 e_bf

where e32_model is the pin run in fp32 on the CPU against ref64. The factor 4 is the suite's convention for "another draw of
the same rounding noise" and deliberately not tighter: bf16 rounding flips cascade through 12 blocks, so the rounded network
run in fp32 and in float64 already differ from each other by about 0.6 e_bf (measured on the CPU with these random weights:
e_bf 0.021 / 0.019 and 0.012 / 0.012 between the two emulations, at max |feature| of 4.0 / 4.1, for vit_s_32 /
vit_b_32_clip); an end-to-end bit model does not exist. The lower bound makes a build that silently runs the fp32 kernels
under the flag fail (e32_model was 3e-6 in the same experiment).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import vit16_pin  # noqa: E402
import vit_pin  # noqa: E402
from oracle import blocks  # noqa: E402
from orbit_dataset_amd import _lib, synthetic  # noqa: E402
from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser  # noqa: E402
from test_gpu_vit_ops import _prof_rows  # noqa: E402
from vit_bf16_emulation import emulate_bf16_linears  # noqa: E402

NAMES = ("vit_s_32", "vit_s_16", "vit_b_32_clip")
B = 3
EPI_BIAS, EPI_GELU, EPI_RESIDUAL = 0, 1, 2
LOGIT_TOL = 1e-3  # the fp32 head's own tolerance (tests/test_gpu_vit.py)


def _new_pin(name):
    return (vit16_pin.TimmViT16(name) if name in vit16_pin.VIT16 else vit_pin.TimmViT(name)).eval()


def _spec(name):
    """(D, heads, eps, clip, patch, tokens)"""
    if name in vit16_pin.VIT16:
        return vit16_pin.VIT16[name] + (16, vit16_pin.TOKENS)
    return vit_pin.VIT[name] + (32, vit_pin.TOKENS)


def _st():
    return _lib.stream_handle()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


class Plan:
    """an orbit_vit_* plan driven through the C-ABI"""

    def __init__(self, lib, name, params=None, bf16=False):
        self.lib, self.name = lib, name
        self.h = ctypes.c_void_p()
        _lib.check(lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(self.h)), "orbit_vit_create")
        self.D = lib.orbit_vit_output_size(self.h)
        if bf16:
            self.enable_bf16()
        if params is not None:
            self.load(params)

    def enable_bf16(self):
        _lib.check(self.lib.orbit_vit_enable_bf16(self.h), "orbit_vit_enable_bf16")

    def load(self, params):
        tensors = list(params.values())
        ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        _lib.check(self.lib.orbit_vit_load_all_async(self.h, ptrs, len(tensors), _st()), "orbit_vit_load_all_async")
        _lib.check(self.lib.orbit_vit_finalize(self.h, _st()), "orbit_vit_finalize")

    def features(self, frames, film=None):
        n = frames.shape[0]
        ws = torch.empty(self.lib.orbit_vit_workspace_bytes(self.h, n), dtype=torch.uint8, device=frames.device)
        feats = torch.full((n, self.D), float("nan"), device=frames.device)
        g, b = film if film is not None else (None, None)
        _lib.check(self.lib.orbit_vit_forward(self.h, _lib.dptr(frames), n, _lib.dptr(g), _lib.dptr(b), _lib.dptr(feats), _vp(ws),
                                              ws.numel(), _st()), "orbit_vit_forward")
        torch.cuda.synchronize()
        return feats.cpu()

    def close(self):
        if self.h:
            self.lib.orbit_vit_destroy(self.h)
            self.h = None


_CACHE = {}


def _model(name):
    """per model, computed once and left unchanged: the pin with synthetic parameters, 3 frames, a FiLM pair, the float64
    references of both (ref64, emu64) and the fp32 pin's own error"""
    if name not in _CACHE:
        pin = _new_pin(name)
        synthetic.init_parameters_(pin)
        gen = torch.Generator().manual_seed(11)
        frames = torch.randn(B, 3, 224, 224, generator=gen)
        D = pin.output_size
        own = dict(pin.named_parameters())
        film = {}
        for slot in pin.film_slot_names():
            film[slot + ".weight"] = (own[slot + ".weight"] * (1 + 0.1 * torch.randn(D, generator=gen))).detach()
            film[slot + ".bias"] = 0.1 * torch.randn(D, generator=gen)
        ref = _new_pin(name)
        ref.load_state_dict(pin.state_dict())
        ref = ref.double()
        emu = _new_pin(name)
        emu.load_state_dict(pin.state_dict())
        emu = emulate_bf16_linears(emu.double())
        with torch.no_grad():
            ref64, emu64, fp32 = ref(frames.double()), emu(frames.double()), pin(frames)
        _CACHE[name] = {"pin": pin, "frames": frames, "film": film, "ref64": ref64, "emu64": emu64,
                        "e_bf": (emu64 - ref64).abs().max().item(), "e32": (fp32.double() - ref64).abs().max().item()}
    return _CACHE[name]


def _device_params(pin, scale=None):
    """the pin's state_dict on the device, in state_dict order (contiguous fp32 tensors of their own)"""
    return {k: (v if scale is None else v * scale(k)).float().contiguous().cuda() for k, v in pin.state_dict().items()}


def _film_vectors(pin, film):
    g = torch.cat([film[n + ".weight"].reshape(-1) for n in pin.film_slot_names()])
    b = torch.cat([film[n + ".bias"].reshape(-1) for n in pin.film_slot_names()])
    return g.cuda(), b.cuda()


def _compose(lib, name, p, frames, film):
    """The bf16 forward, operator by operator: the launches of orbit_vit_forward on a bf16 plan, in its order, on buffers of
    this function's own; the weights are packed here, from the fp32 tensors."""
    D, heads, eps, clip, patch, N = _spec(name)
    n = frames.shape[0]
    M = n * N
    dev = frames.device
    x = torch.empty(M, D, device=dev)
    h = torch.empty(M, D, device=dev)
    big = torch.empty(M, 4 * D, device=dev)
    feats = torch.full((n, D), float("nan"), device=dev)

    def ln(src, s_stride, dst, d_stride, rows, key, slot):
        if film is not None and slot is not None:
            g, b = film[0][slot * D:(slot + 1) * D], film[1][slot * D:(slot + 1) * D]
        else:
            g, b = p[key + ".weight"], p[key + ".bias"]
        _lib.check(lib.orbit_op_vit_layernorm(_lib.dptr(src), s_stride, _lib.dptr(dst), d_stride, rows, D, _lib.dptr(g),
                                              _lib.dptr(b), eps, _st()), "orbit_op_vit_layernorm")

    def linear(src, key, res, dst, Nout, K, epi):
        w = p[key + ".weight"]
        wb = torch.empty(w.shape, dtype=torch.int16, device=dev)
        _lib.check(lib.orbit_op_vit_pack_bf16(_lib.dptr(w), _vp(wb), w.numel(), _st()), "orbit_op_vit_pack_bf16")
        _lib.check(lib.orbit_op_vit_linear_bf16(_lib.dptr(src), _vp(wb), _lib.dptr(p[key + ".bias"]), _lib.dptr(res),
                                                _lib.dptr(dst), M, Nout, K, epi, 0, _st()), "orbit_op_vit_linear_bf16")

    _lib.check(lib.orbit_op_vit_patch_embed_p(_lib.dptr(frames), _lib.dptr(p["patch_embed.proj.weight"]),
                                              _lib.dptr(p.get("patch_embed.proj.bias")), _lib.dptr(p["pos_embed"]),
                                              _lib.dptr(p["cls_token"]), _lib.dptr(x), n, D, patch, 0, _st()),
               "orbit_op_vit_patch_embed_p")
    if clip:
        ln(x, D, x, D, M, "norm_pre", None)
    for i in range(12):
        b = "blocks.%d." % i
        ln(x, D, h, D, M, b + "norm1", 2 * i)
        linear(h, b + "attn.qkv", None, big, 3 * D, D, EPI_BIAS)
        _lib.check(lib.orbit_op_vit_attention_tokens(_lib.dptr(big), _lib.dptr(h), n, N, D, heads, _st()),
                   "orbit_op_vit_attention_tokens")
        linear(h, b + "attn.proj", x, x, D, D, EPI_RESIDUAL)
        ln(x, D, h, D, M, b + "norm2", 2 * i + 1)
        linear(h, b + "mlp.fc1", None, big, 4 * D, D, EPI_GELU)
        linear(big, b + "mlp.fc2", x, x, D, 4 * D, EPI_RESIDUAL)
    ln(x, N * D, feats, D, n, "norm", 24)
    torch.cuda.synchronize()
    return feats.cpu()


@pytest.mark.parametrize("name", NAMES)
def test_bf16_forward_is_its_operators_composed_and_sized_as_the_emulation(lib, device, name):
    """Cases 1 and 4 of the module docstring on one plan: exact composition with and without FiLM, the profiler's rows of one
    forward, and the size of the trade against the float64 pin."""
    m = _model(name)
    p = _device_params(m["pin"])
    frames = m["frames"].cuda()
    film = _film_vectors(m["pin"], m["film"])
    plan = Plan(lib, name, p, bf16=True)
    try:
        assert lib.orbit_vit_bf16_enabled(plan.h) == 1
        got = plan.features(frames)
        lib.orbit_prof_enable(1)
        try:
            again = plan.features(frames)
            rows = {r: n for r, n in _prof_rows(lib).items() if r.startswith("vit_") and n}
        finally:
            lib.orbit_prof_enable(0)
        got_film = plan.features(frames, film)
    finally:
        plan.close()
    assert torch.equal(got, again)
    gemm = {r: n for r, n in rows.items() if "<" in r and "patch_embed" not in r}
    assert gemm == {"vit_%s_bf16<64>" % g: 12 for g in ("qkv", "proj", "fc1", "fc2")}, rows  # no fp32 token GEMM, no re-pack
    assert "vit_pack_bf16" not in rows and rows.get("vit_layernorm") == (26 if _spec(name)[3] else 25), rows
    assert torch.equal(got, _compose(lib, name, p, frames, None)), "the bf16 forward is not its operators composed"
    assert torch.equal(got_film, _compose(lib, name, p, frames, film)), "the bf16 forward with FiLM is not its operators composed"
    assert (got_film - got).abs().max().item() > 0.1  # FiLM reaches the features
    err = (got.double() - m["ref64"]).abs().max().item()
    print("\n[vit-bf16] %s: |got - ref64| %.3g, e_bf %.3g (ratio %.2f), |got - emu64| %.3g, fp32 pin e32 %.3g, max |feature| %.2f"
          % (name, err, m["e_bf"], err / m["e_bf"], (got.double() - m["emu64"]).abs().max().item(), m["e32"],
             m["ref64"].abs().max().item()))
    assert torch.isfinite(got).all()
    assert err <= 4 * m["e_bf"], "%s: max |got - ref64| = %.3g > 4 e_bf = %.3g" % (name, err, 4 * m["e_bf"])
    assert err > 16 * m["e32"], "%s: %.3g from the float64 pin is fp32 accuracy (fp32 pin: %.3g): the flag did nothing" % (
        name, err, m["e32"])


def test_parameter_upload_invalidates_the_bf16_copies(lib, device):
    """forward, orbit_vit_load_all_async of other weights, forward again == a fresh bf16 plan loaded with the new weights."""
    name = "vit_s_32"
    m = _model(name)
    frames = m["frames"].cuda()
    old = _device_params(m["pin"])
    new = _device_params(m["pin"], scale=lambda k: 1.25 if k.endswith("mlp.fc2.weight") or k.endswith("attn.qkv.weight") else 1.0)
    plan, fresh = Plan(lib, name, old, bf16=True), Plan(lib, name, new, bf16=True)
    try:
        first = plan.features(frames)
        plan.load(new)
        second = plan.features(frames)
        want = fresh.features(frames)
    finally:
        plan.close()
        fresh.close()
    assert not torch.equal(first, second)
    assert torch.equal(second, want), "a bf16 forward after a parameter upload used stale weight copies"


def test_an_fp32_plan_is_untouched_by_a_bf16_plan_of_the_same_model(lib, device):
    name = "vit_s_32"
    m = _model(name)
    frames = m["frames"].cuda()
    p = _device_params(m["pin"])
    plain, other = Plan(lib, name, p), Plan(lib, name, p)
    try:
        before = plain.features(frames)
        fp32_other = other.features(frames)
        other.enable_bf16()  # after finalize and after an fp32 forward
        other.enable_bf16()  # idempotent
        bf = other.features(frames)
        after = plain.features(frames)
        assert lib.orbit_vit_bf16_enabled(plain.h) == 0 and lib.orbit_vit_bf16_enabled(other.h) == 1
        assert lib.orbit_vit_workspace_bytes(plain.h, B) == lib.orbit_vit_workspace_bytes(other.h, B)
        assert lib.orbit_vit_macs_per_frame(plain.h) == lib.orbit_vit_macs_per_frame(other.h)
    finally:
        plain.close()
        other.close()
    assert torch.equal(before, after) and torch.equal(before, fp32_other)
    assert not torch.equal(bf, before)
    assert (before.double() - m["ref64"]).abs().max().item() <= 1e-4  # (tests/test_gpu_vit.py's feature tolerance)


@pytest.mark.parametrize("name", ["vit_s_32", "vit_s_16"])
def test_training_entry_points_and_enable_order_are_refused(lib, device, name):
    """On a bf16 plan the three training entry points return ORBIT_ERR_ARG naming the flag before any launch; the backward
    opt-ins are refused after orbit_vit_enable_bf16 and orbit_vit_enable_bf16 after either of them; the size queries of a plan
    without the flag are what they were."""
    m = _model(name)
    p = _device_params(m["pin"])
    D, N = _spec(name)[0], _spec(name)[5]
    buf = torch.zeros(1 << 16, device=device)
    q = _lib.dptr(buf)
    plan = Plan(lib, name, p, bf16=True)
    plain, taped, weights = Plan(lib, name), Plan(lib, name), Plan(lib, name)
    lib.orbit_prof_enable(1)
    try:
        calls = (lambda: lib.orbit_vit_train_forward(plan.h, q, 1, None, None, q, q, 1 << 40, q, 1 << 40, _st()),
                 lambda: lib.orbit_vit_backward(plan.h, 1, None, None, q, q, 1 << 40, q, q, q, 1 << 40, _st()),
                 lambda: lib.orbit_vit_backward_params(plan.h, q, 1, None, None, q, q, 1 << 40, q, q, q, q, 1 << 40, _st()))
        for call in calls:
            assert call() == -1
            assert "orbit_vit_enable_bf16" in _lib.last_error(), _lib.last_error()
        for enable in (lib.orbit_vit_enable_backward, lib.orbit_vit_enable_weight_backward):
            assert enable(plan.h) == -1 and "orbit_vit_enable_bf16" in _lib.last_error(), _lib.last_error()
        assert lib.orbit_vit_enable_backward(taped.h) == 0 and lib.orbit_vit_enable_weight_backward(weights.h) == 0
        for other in (taped, weights):
            assert lib.orbit_vit_enable_bf16(other.h) == -1
            assert "orbit_vit_enable_backward" in _lib.last_error() and "bf16" in _lib.last_error(), _lib.last_error()
            assert lib.orbit_vit_bf16_enabled(other.h) == 0
        torch.cuda.synchronize()
        assert not any(n for r, n in _prof_rows(lib).items() if r.startswith("vit_")), "a refused call launched a kernel"
        # a plan without the flag: the documented sizes ((12 * 9 + 1) token-stream slots of align_up(tokens B D 4, 256) bytes)
        md = -(-(N * 2 * D * 4) // 256) * 256
        assert lib.orbit_vit_tape_bytes(taped.h, 2) == 109 * md
        assert lib.orbit_vit_tape_bytes(plain.h, 2) == (109 * md if N == 50 else 0)
        assert lib.orbit_vit_backward_workspace_bytes(taped.h, 2) > 0 and lib.orbit_vit_backward_params_workspace_bytes(weights.h, 2) > 0
    finally:
        lib.orbit_prof_enable(0)
        for x in (plan, plain, taped, weights):
            x.close()


def test_recogniser_with_bf16_inference(lib, device):
    """personalise + predict of a 3-way synthetic task through VisionTransformer(bf16_inference = True), ProtoNets head
    (Euclidean: logit_k = 2 q . mu_k - mu_k . mu_k, mu_k the mean context feature of class k).

    The bound of the feature test mapped through the head: with every feature within eps = 4 e_bf of its float64 value (e_bf
    measured on THIS task's frames), q and mu_k each move by at most eps per coordinate, so
        |dlogit_k| <= 2 (eps |mu_k|_1 + eps |q|_1 + D eps^2) + 2 eps |mu_k|_1 + D eps^2 = eps (4 |mu_k|_1 + 2 |q|_1) + 3 D eps^2,
    evaluated per (query, class) on the float64 features, plus the fp32 head's own 1e-3 tolerance. A worst-case map, loose by
    construction (on the MI355X: max |dlogit| 0.63 against bounds of 202 and more); what it rules out is a head fed other
    features than the bf16 plan's. The sharp checks are the feature tests above."""
    name = "vit_s_32"
    model = SingleStepFewShotRecogniser(name, False, "proto", 1, 8, False, 16, 1.0)
    synthetic.init_parameters_(model)
    fe = model.feature_extractor
    fe.bf16_inference = True
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(True)
    t = synthetic.make_task(17, way=3, shots=1, frames_per_shot=2, num_query=6, frame_size=224)
    ctx, lab, tgt = t["context_clips"], t["context_labels"], t["target_clips"]
    lib.orbit_prof_enable(1)
    try:
        with torch.no_grad():
            model.personalise(ctx.cuda(), lab.cuda())
            logits = model.predict(tgt.cuda()).cpu()
        rows = {r: n for r, n in _prof_rows(lib).items() if r.startswith("vit_") and "<" in r and "patch_embed" not in r and n}
    finally:
        lib.orbit_prof_enable(0)
    assert rows and all("_bf16<" in r for r in rows), rows  # every token GEMM of the task ran on the bf16 kernel
    assert list(fe._plans) == [fe._plan_key(224, 224, False)] and fe._plan_key(224, 224, False)[-1] == "bf16"
    sd = {k[len("feature_extractor."):]: v.cpu() for k, v in model.state_dict().items() if k.startswith("feature_extractor.")}
    ref, emu = _new_pin(name), _new_pin(name)
    ref.load_state_dict(sd)
    emu.load_state_dict(sd)
    ref, emu = ref.double(), emulate_bf16_linears(emu.double())
    frames = torch.cat((ctx.reshape(-1, 3, 224, 224), tgt.reshape(-1, 3, 224, 224))).double()
    with torch.no_grad():
        f64, e64 = ref(frames), emu(frames)
    eps = 4 * (e64 - f64).abs().max().item()
    fc, fq = f64[:ctx.shape[0]], f64[ctx.shape[0]:]
    _, W, b = blocks.proto_configure(fc, lab, "euclidean")
    want = blocks.proto_predict(fq, W, b, 1.0, "euclidean")
    mu1 = (W / 2).abs().sum(1)
    bound = eps * (4 * mu1[None, :] + 2 * fq.abs().sum(1)[:, None]) + 3 * fq.shape[1] * eps * eps + LOGIT_TOL
    err = (logits.double() - want).abs()
    print("\n[vit-bf16] recogniser: max |dlogit| %.3g, smallest bound %.3g, eps %.3g" % (err.max().item(), bound.min().item(), eps))
    assert bool((err <= bound).all()), "max |dlogit| / bound = %.3g" % (err / bound).max().item()
    assert err.max().item() > 0  # not the fp32 path
    model._reset()


def test_learner_flag_reaches_the_extractor_and_the_test_stats(lib, device):
    """--vit_bf16 on both learners: the extractor carries bf16_inference, the test loop runs, and its stats name the precision."""
    from orbit_dataset_amd import learner
    argv = ["--feature_extractor", "vit_s_32", "--mode", "test", "--classifier", "proto", "--way", "2", "--shots", "1",
            "--frames_per_shot", "2", "--num_query_videos", "1", "--frames_per_video", "3", "--batch_size", "8", "--num_test_tasks", "1"]
    L = learner.Learner(learner.build_parser().parse_args(argv + ["--vit_bf16"]))
    assert L.model.feature_extractor.bf16_inference is True
    stats = L.test()
    assert stats["vit_precision"] == "bf16" and stats["num_tasks"] == 1
    assert all(k[-1] == "bf16" for k in L.model.feature_extractor._plans)
    plain = learner.Learner(learner.build_parser().parse_args(argv))
    assert plain.model.feature_extractor.bf16_inference is False and plain.test()["vit_precision"] == "fp32"
    M = learner.MultiStepLearner(learner.build_multistep_parser().parse_args(
        argv[:4] + argv[6:] + ["--vit_bf16", "--personalize_num_grad_steps", "2"]))
    assert M.model.feature_extractor.bf16_inference is True and M.test()["vit_precision"] == "bf16"
