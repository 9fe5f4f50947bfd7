"""The native gradients of every parameter of the patch-16 transformer extractors end to end (orbit_vit_enable_weight_backward,
orbit_vit_train_forward / orbit_vit_backward_params at 197 tokens, autograd.VitFunction,
VisionTransformer.native_weight_backward_patch16, learner --vit16_native_weight_backward) against the float64 CPU pin
(tests/vit16_pin.TimmViT16(name).double()), per state_dict key, as tests/test_gpu_vit_wgrad.py for the patch-32 models.

Gate (tests/test_gpu_vit_ops.py): max |got - ref64| <= max(4 * e32, 8 * 2**-24 * max |ref64|), e32 = the fp32 pin's own gradient
error for that key against the float64 pin on the same inputs, measured here. The kernels one by one:
tests/test_gpu_vit16_wgrad_ops.py (weight gradients) and tests/test_gpu_vit16_bwd_ops.py (the 197-token attention backward).

Largest err / e32 seen on the MI355X (run with -s): 3.37 (vit_b_16_clip B = 2, blocks.8.mlp.fc1.weight, with 3.33 on that
layer's bias - the sum of the same dY rows, so the figure is the data-gradient stream's, not the weight-gradient sum's);
vit_s_16 B = 1: 2.48 (blocks.3.mlp.fc1.bias), B = 3: 2.37 (blocks.0.norm2.bias), with film vectors 2.32.
"""
import ctypes

import pytest
import torch
from torch.func import functional_call

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import vit16_pin  # noqa: E402
from test_gpu_vit_ops import _prof_rows, gate  # noqa: E402
from orbit_dataset_amd import _lib, synthetic  # noqa: E402
from orbit_dataset_amd.data.utils import attach_frame_history  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor  # noqa: E402

_CACHE = {}
CASES = [("vit_s_16", 1), ("vit_s_16", 3), ("vit_b_16_clip", 2)]
SENTINEL = 7777.0


def _pair(name):
    """(HIP extractor on cuda:0, every parameter trainable, native_weight_backward_patch16 = True; CPU pin), same parameters."""
    if name not in _CACHE:
        fe, _ = create_feature_extractor(name, with_film=False, learn_extractor=True)
        pin = vit16_pin.TimmViT16(name).eval()
        synthetic.init_parameters_(pin)
        fe.load_state_dict(pin.state_dict(), strict=True)
        fe.eval().to("cuda:0")
        fe.native_weight_backward_patch16 = True
        _CACHE[name] = (fe, pin)
    return _CACHE[name]


def _film_keys(pin):
    return [s + leaf for s in pin.film_slot_names() for leaf in (".weight", ".bias")]


def _case(name, B, with_film=False):
    """Inputs of one (model, batch) and the pin's gradients of sum(feats * R) per state_dict key in float64, with the fp32 pin's
    error per key; with_film: the 25 LayerNorms take film vectors (their gradients under the slot keys). Computed once."""
    key = ("case", name, B, with_film)
    if key not in _CACHE:
        _, pin = _pair(name)
        g = torch.Generator().manual_seed(160 + B)
        D = pin.output_size
        frames = torch.randn(B, 3, 224, 224, generator=g)
        R = torch.randn(B, D, generator=g)
        slots = pin.film_slot_names()
        own = dict(pin.named_parameters())
        gam = torch.cat([(own[s + ".weight"].detach() * (1 + 0.1 * torch.randn(D, generator=g))) for s in slots])
        bet = torch.cat([0.1 * torch.randn(D, generator=g) for s in slots])
        ref = {}
        for dtype in (torch.float64, torch.float32):
            net = vit16_pin.TimmViT16(name).eval()
            net.load_state_dict(pin.state_dict())
            net = net.to(dtype).requires_grad_(True)
            film = {}
            if with_film:
                for i, s in enumerate(slots):
                    film[s + ".weight"] = gam[i * D:(i + 1) * D].to(dtype).clone().requires_grad_(True)
                    film[s + ".bias"] = bet[i * D:(i + 1) * D].to(dtype).clone().requires_grad_(True)
            (functional_call(net, film, (frames.to(dtype),)) * R.to(dtype)).sum().backward()
            ref[dtype] = {n: (film[n] if n in film else q).grad.double() for n, q in net.named_parameters()}
        e32 = {n: (ref[torch.float32][n] - v).abs().max().item() for n, v in ref[torch.float64].items()}
        _CACHE[key] = dict(frames=frames, R=R, gamma=gam if with_film else None, beta=bet if with_film else None,
                           ref64=ref[torch.float64], e32=e32)
    return _CACHE[key]


def _native(fe, frames, gamma, beta, dfeats):
    """orbit_vit_train_forward + orbit_vit_backward_params through the C-ABI on a plan opted in with
    orbit_vit_enable_weight_backward, on NaN-filled, guarded buffers, and orbit_vit_backward on the same tape: (feats, {key:
    gradient or None (untouched slot)}, dgamma, dbeta, dgamma and dbeta of orbit_vit_backward), on the CPU."""
    lib = _lib.load()
    plan = fe._plan(224, 224)
    fe.sync(plan)
    h = plan.handle
    _lib.check(lib.orbit_vit_enable_weight_backward(h), "orbit_vit_enable_weight_backward")
    B, D, dev = frames.shape[0], fe.output_size, frames.device
    st = _lib.stream_handle()
    assert lib.orbit_vit_tape_bytes(h, B) == 109 * ((B * 197 * D * 4 + 255) // 256 * 256)
    tape = torch.empty(lib.orbit_vit_tape_bytes(h, B), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.orbit_vit_workspace_bytes(h, B), dtype=torch.uint8, device=dev)
    feats = torch.full((B + 1, D), float("nan"), device=dev)
    feats[B:] = SENTINEL
    _lib.check(lib.orbit_vit_train_forward(h, _lib.dptr(frames), B, _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(feats),
                                           ctypes.c_void_p(tape.data_ptr()), tape.numel(), ctypes.c_void_p(ws.data_ptr()),
                                           ws.numel(), st), "orbit_vit_train_forward")
    n, total = fe.film_size, lib.orbit_vit_grad_floats(h)
    out = []
    for with_params in (True, False):
        dg = torch.full((n + D,), float("nan"), device=dev)
        db = torch.full((n + D,), float("nan"), device=dev)
        dg[n:], db[n:] = SENTINEL, SENTINEL
        if with_params:
            flat = torch.full((total + 64,), float("nan"), device=dev)
            flat[total:] = SENTINEL
            nbytes = lib.orbit_vit_backward_params_workspace_bytes(h, B)
            assert nbytes > 0
            bws = torch.full((nbytes // 4 + 64,), float("nan"), device=dev)
            bws[nbytes // 4:] = SENTINEL
            _lib.check(lib.orbit_vit_backward_params(h, _lib.dptr(frames), B, _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(dfeats),
                                                     ctypes.c_void_p(tape.data_ptr()), tape.numel(), _lib.dptr(flat), _lib.dptr(dg),
                                                     _lib.dptr(db), ctypes.c_void_p(bws.data_ptr()), nbytes, st),
                       "orbit_vit_backward_params")
            torch.cuda.synchronize()
            assert bool((flat[total:] == SENTINEL).all()) and bool((bws[nbytes // 4:] == SENTINEL).all())
        else:
            bws = torch.full((lib.orbit_vit_backward_workspace_bytes(h, B) // 4,), float("nan"), device=dev)
            _lib.check(lib.orbit_vit_backward(h, B, _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(dfeats),
                                              ctypes.c_void_p(tape.data_ptr()), tape.numel(), _lib.dptr(dg), _lib.dptr(db),
                                              ctypes.c_void_p(bws.data_ptr()), 4 * bws.numel(), st), "orbit_vit_backward")
            torch.cuda.synchronize()
        assert bool((dg[n:] == SENTINEL).all()) and bool((db[n:] == SENTINEL).all()) and bool((feats[B:] == SENTINEL).all())
        out += [dg[:n].cpu(), db[:n].cpu()]
    flat = flat.cpu()
    grads = {}
    for i, (key, numel) in enumerate(fe._keys):
        off = lib.orbit_vit_param_offset(h, i)
        t = flat[off:off + numel]
        grads[key] = None if bool(torch.isnan(t).all()) else t
    return (feats[:B].cpu(), grads) + tuple(out)


def _native_case(name, B, with_film=False):
    key = ("native", name, B, with_film)
    if key not in _CACHE:
        fe, _ = _pair(name)
        c = _case(name, B, with_film)
        film = (c["gamma"].cuda(), c["beta"].cuda()) if with_film else (None, None)
        _CACHE[key] = _native(fe, c["frames"].cuda(), *film, c["R"].cuda())
    return _CACHE[key]


def _check_against_pin(name, B, with_film):
    c = _case(name, B, with_film)
    fe, pin = _pair(name)
    feats, grads, dg, db, dg0, db0 = _native_case(name, B, with_film)
    film = (c["gamma"].cuda(), c["beta"].cuda()) if with_film else None
    with torch.no_grad():
        assert torch.equal(feats, fe(c["frames"].cuda(), film=film).cpu()), "taped features differ from the inference forward"
    assert torch.equal(dg, dg0) and torch.equal(db, db0), "dgamma / dbeta differ from orbit_vit_backward on the same tape"
    D, slots = pin.output_size, pin.film_slot_names()
    film_keys = set(_film_keys(pin))
    worst, worst_key = 0.0, None
    assert set(grads) == set(c["ref64"])
    for key, ref64 in c["ref64"].items():
        what = "vit16 wgrad %s B=%d%s %s" % (name, B, " film" if with_film else "", key)
        if key in film_keys:  # the 50 FiLM-slot LayerNorm parameters: their slots stay untouched, dgamma / dbeta carry them
            assert grads[key] is None, what + ": FiLM-slot gradient written into param_grads"
            i = slots.index(key.rsplit(".", 1)[0])
            got = (dg if key.endswith(".weight") else db)[i * D:(i + 1) * D]
        else:
            assert grads[key] is not None, what + ": not written"
            got = grads[key]
        ratio = gate(got.view(ref64.shape), ref64, c["e32"][key], what)
        if ratio > worst:
            worst, worst_key = ratio, key
    print("[vit16-wgrad] %s B=%d%s: largest err / e32 over %d keys %.2f (%s)"
          % (name, B, " film" if with_film else "", len(grads), worst, worst_key))


@pytest.mark.parametrize("name,B", CASES)
def test_every_parameter_gradient_matches_the_float64_pin(device, name, B):
    _check_against_pin(name, B, False)


def test_with_film_vectors_the_layernorm_slots_stay_untouched(device):
    _check_against_pin("vit_s_16", 3, True)


def test_two_runs_are_bitwise_equal(device):
    name, B = "vit_s_16", 3
    fe, _ = _pair(name)
    c = _case(name, B)
    first = _native_case(name, B)
    again = _native(fe, c["frames"].cuda(), None, None, c["R"].cuda())
    assert torch.equal(first[0], again[0]) and all(torch.equal(a, b) for a, b in zip(first[2:], again[2:]))
    for key, t in first[1].items():
        assert (t is None and again[1][key] is None) or torch.equal(t, again[1][key]), key


def _fresh(name, learn):
    fe, _ = create_feature_extractor(name, with_film=False, learn_extractor=learn)
    fe.load_state_dict(_pair(name)[1].state_dict(), strict=True)
    fe.eval().to("cuda:0")
    return fe


@pytest.mark.parametrize("name,B", [("vit_s_16", 3), ("vit_b_16_clip", 2)])
def test_module_backward_fills_every_grad(device, name, B):
    c = _case(name, B)
    _, grads, dg, db, _, _ = _native_case(name, B)
    fe = _fresh(name, True)
    frames, R = c["frames"].cuda(), c["R"].cuda()
    with torch.no_grad():
        fe(frames)  # the plan exists and has run inference before either attribute is set
    fe.native_backward_patch16 = True  # the FiLM opt-in alone: weight gradients still refused by name
    with pytest.raises(NotImplementedError, match=r"first: cls_token"):
        fe(frames)
    fe.native_backward_patch16 = False
    fe.native_weight_backward_patch16 = True
    (fe(frames) * R).sum().backward()
    D, slots = fe.output_size, [s for s, _ in fe.film_slot_modules()]
    for key, p in fe.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, key
        gate(p.grad.cpu(), c["ref64"][key], c["e32"][key], "vit16 wgrad module %s B=%d %s" % (name, B, key))
        if grads[key] is None:
            i = slots.index(key.rsplit(".", 1)[0])
            want = (dg if key.endswith(".weight") else db)[i * D:(i + 1) * D]
        else:
            want = grads[key]
        assert torch.equal(p.grad.cpu().reshape(-1), want), key + ": differs from the C-ABI call on the same inputs"


def test_one_trainable_weight_in_a_frozen_network(device):
    name, B, key = "vit_s_16", 3, "patch_embed.proj.weight"
    c = _case(name, B)
    grads = _native_case(name, B)[1]
    fe = _fresh(name, False)
    fe.native_weight_backward_patch16 = True
    params = dict(fe.named_parameters())
    params[key].requires_grad_(True)
    (fe(c["frames"].cuda()) * c["R"].cuda()).sum().backward()
    assert torch.equal(params[key].grad.cpu().reshape(-1), grads[key])
    assert all(p.grad is None for n, p in params.items() if n != key)
    # the patch-32 opt-ins open nothing here
    fe.native_weight_backward_patch16 = False
    fe.native_weight_backward = fe.native_backward = True
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe(c["frames"].cuda())


def test_a_plan_that_did_not_opt_in_refuses_before_any_launch(device, lib):
    fe = _fresh("vit_s_16", False)
    x = torch.zeros(1, 3, 224, 224, device="cuda:0")
    with torch.no_grad():
        fe(x)
    plan = fe._plan(224, 224)
    _lib.check(lib.orbit_vit_enable_backward(plan.handle), "orbit_vit_enable_backward")
    buf = torch.zeros(1 << 16, device="cuda:0")
    p, big = _lib.dptr(buf), 1 << 40
    lib.orbit_prof_enable(1)
    try:
        rc = lib.orbit_vit_backward_params(plan.handle, _lib.dptr(x), 1, None, None, p, ctypes.c_void_p(buf.data_ptr()), big, p, p,
                                           p, ctypes.c_void_p(buf.data_ptr()), big, _lib.stream_handle())
        assert rc == -1 and "vit_s_16" in _lib.last_error() and "weight gradients" in _lib.last_error()
        assert lib.orbit_vit_backward_params_workspace_bytes(plan.handle, 1) == 0
        assert not any(n for k, n in _prof_rows(lib).items() if k.startswith("vit_")), "a refused call launched something"
    finally:
        lib.orbit_prof_enable(0)
    # and the switch after inference forwards on the finalized plan
    assert lib.orbit_vit_enable_weight_backward(plan.handle) == 0
    assert lib.orbit_vit_backward_params_workspace_bytes(plan.handle, 1) > 0


@pytest.mark.parametrize("extra", [[], ["--with_lite"]], ids=["plain", "lite"])
def test_learner_training_smoke(device, lib, extra):
    """learner --mode train --feature_extractor vit_s_16 --learn_extractor --vit16_native_weight_backward: one 2-way task of a
    handful of frames per optimizer step, two steps."""
    from orbit_dataset_amd import learner
    args = learner.build_parser().parse_args(
        ["--mode", "train", "--feature_extractor", "vit_s_16", "--learn_extractor", "--vit16_native_weight_backward"] + extra +
        ["--way", "2", "--shots", "1", "--frames_per_shot", "3", "--num_query_videos", "1", "--frames_per_video", "2",
         "--num_train_tasks", "2", "--tasks_per_batch", "1", "--num_lite_samples", "2", "--batch_size", "4",
         "--learning_rate", "1e-3"])
    learner.verify_args(args)
    L = learner.Learner(args)
    fe = L.model.feature_extractor
    assert fe.native_weight_backward_patch16 is True and fe.native_weight_backward is False and fe._grad_scope == "all"
    watched = {k: p for k, p in fe.named_parameters() if k in ("patch_embed.proj.weight", "pos_embed")}
    assert len(watched) == 2
    snaps, grads = [{k: p.detach().clone() for k, p in watched.items()}], []

    def hook(opt, a, k):
        grads.append({k: None if p.grad is None else p.grad.detach().clone() for k, p in watched.items()})
        snaps.append({k: p.detach().clone() for k, p in watched.items()})

    from torch.optim.optimizer import register_optimizer_step_post_hook
    handle = register_optimizer_step_post_hook(hook)
    lib.orbit_prof_enable(1)
    try:
        stats = L.train()
        rows = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
        handle.remove()
    assert stats["num_tasks"] == 2 and len(snaps) == 3
    assert stats["loss"][0] is not None and torch.isfinite(torch.tensor(stats["loss"][0]))
    for before, after, g in zip(snaps, snaps[1:], grads):
        for k in watched:
            assert g[k] is not None and torch.isfinite(g[k]).all() and bool((g[k] != 0).any()), k + ": no gradient"
            assert not torch.equal(before[k], after[k]) and torch.isfinite(after[k]).all(), k + " did not change"
    wgrad = {k: v for k, v in rows.items() if k.startswith("vit_wgrad_")}
    per_layer = [sum(v for k, v in wgrad.items() if k.startswith("vit_wgrad_%s<" % layer)) for layer in ("qkv", "proj", "fc1", "fc2")]
    patch = sum(v for k, v in wgrad.items() if k.startswith("vit_wgrad_patch16_embed<"))
    assert patch >= 2 and per_layer == [12 * patch] * 4, rows
    assert not any(k.startswith("vit_wgrad_patch_embed<") for k in wgrad), rows  # (the 32 x 32 form never ran)
    assert rows.get("vit_attention_bwd", 0) == 0 and rows.get("vit_attention197_bwd", 0) == 12 * patch, rows


def test_finetuner_with_learn_extractor(device, lib):
    """multi-step-learner --learn_extractor --vit16_native_weight_backward on a tiny task. The linear head starts at zero
    (reference classifier_heads.py), so the gradient that reaches the extractor in the FIRST step is exactly zero; the
    personalisation takes two steps, after which patch_embed.proj.weight and pos_embed have moved and the logits are finite."""
    from orbit_dataset_amd import learner
    args = learner.build_multistep_parser().parse_args(
        ["--feature_extractor", "vit_s_16", "--learn_extractor", "--vit16_native_weight_backward", "--personalize_num_grad_steps",
         "2", "--way", "2", "--shots", "1", "--frames_per_shot", "3", "--num_query_videos", "1", "--frames_per_video", "2",
         "--batch_size", "4"])
    learner.verify_args(args)
    L = learner.MultiStepLearner(args)
    fe = L.model.feature_extractor
    assert fe.native_weight_backward_patch16 is True
    task = L.make_task(0)
    lo, hi = task["target_videos"][0]
    L.model.set_test_mode(True)
    lib.orbit_prof_enable(1)
    try:
        L.model.personalise(task["context_clips"], task["context_labels"].to(L.device), L.learning_args())
        rows = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    # 6 context clips in mini-batches of 4, two steps
    assert sum(v for k, v in rows.items() if k.startswith("vit_wgrad_patch16_embed<")) == 2 * 2, rows
    with torch.no_grad():
        out = L.model.predict(attach_frame_history(task["target_clips"][lo:hi, 0], 1)).detach().cpu()
    assert torch.isfinite(out).all() and out.shape[-1] == 2
    state = L.model.state_dict()
    for key in ("feature_extractor.patch_embed.proj.weight", "feature_extractor.pos_embed"):
        assert not torch.equal(state[key].cpu(), L.base_state[key].cpu()), key + " did not change"
        assert torch.isfinite(state[key]).all()
    L.model._reset()
