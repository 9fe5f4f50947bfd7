"""The opt-in FiLM backward through the frozen patch-16 transformer extractors end to end (orbit_vit_enable_backward,
orbit_vit_train_forward / orbit_vit_backward at 197 tokens, autograd.VitFunction, VisionTransformer.native_backward_patch16,
learner --vit16_native_backward) against the float64 CPU pin (tests/vit16_pin.TimmViT16(name).double() with the FiLM dict
through torch.func.functional_call), as tests/test_gpu_vit_train.py for the patch-32 models.

Gate (tests/test_gpu_vit_ops.py): max |got - ref64| <= max(4 * e32, 8 * 2**-24 * max |ref64|), e32 = the fp32 pin's own gradient
error against the float64 pin on the same inputs, measured here. The new kernel alone: tests/test_gpu_vit16_bwd_ops.py.

Largest err / e32 seen on the MI355X (run with -s): 2.03 (vit_b_16_clip, B = 1, dgamma).
"""
import ctypes

import pytest
import torch
from torch.func import functional_call

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import vit16_pin  # noqa: E402
from oracle import blocks  # noqa: E402
from test_gpu_vit_ops import _prof_rows, gate  # noqa: E402
from orbit_dataset_amd import _lib, synthetic  # noqa: E402
from orbit_dataset_amd.data.utils import attach_frame_history  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor  # noqa: E402
from orbit_dataset_amd.model.film import unfreeze_film  # noqa: E402

_CACHE16 = {}


def _pin(name, dtype=None):
    net = vit16_pin.TimmViT16(name).eval()
    if dtype is not None:
        net.load_state_dict(_pair(name)[1].state_dict())
        net = net.to(dtype).requires_grad_(False)
    return net


def _pair(name):
    """(frozen HIP extractor on cuda:0 with FiLM tagging and native_backward_patch16 = True, CPU pin), same synthetic parameters."""
    if name not in _CACHE16:
        fe, _ = create_feature_extractor(name, with_film=True, learn_extractor=False)
        pin = _pin(name)
        synthetic.init_parameters_(pin)
        fe.load_state_dict(pin.state_dict(), strict=True)
        fe.eval().to("cuda:0")
        fe.native_backward_patch16 = True
        _CACHE16[name] = (fe, pin)
    return _CACHE16[name]


def _case(name, B):
    """Inputs of one (model, batch) and the pin's film gradients of sum(feats * R) in float64 and fp32; computed once."""
    key = ("case", name, B)
    if key not in _CACHE16:
        fe, pin = _pair(name)
        g = torch.Generator().manual_seed(140 + B)
        D = pin.output_size
        frames = torch.randn(B, 3, 224, 224, generator=g)
        R = torch.randn(B, D, generator=g)
        slots = pin.film_slot_names()
        own = dict(pin.named_parameters())
        gam = [(own[s + ".weight"].detach() * (1 + 0.1 * torch.randn(D, generator=g))) for s in slots]
        bet = [0.1 * torch.randn(D, generator=g) for s in slots]
        ref = {}
        for dtype in (torch.float64, torch.float32):
            net = _pin(name, dtype)
            film = {}
            for s, a, b in zip(slots, gam, bet):
                film[s + ".weight"] = a.detach().to(dtype).clone().requires_grad_(True)
                film[s + ".bias"] = b.detach().to(dtype).clone().requires_grad_(True)
            (functional_call(net, film, (frames.to(dtype),)) * R.to(dtype)).sum().backward()
            ref[dtype] = (torch.cat([film[s + ".weight"].grad for s in slots]).double(),
                          torch.cat([film[s + ".bias"].grad for s in slots]).double())
        e32 = tuple((a - b).abs().max().item() for a, b in zip(ref[torch.float32], ref[torch.float64]))
        _CACHE16[key] = dict(frames=frames, R=R, gamma=torch.cat(gam), beta=torch.cat(bet), ref64=ref[torch.float64], e32=e32)
    return _CACHE16[key]


def _enabled_plan(fe):
    lib = _lib.load()
    plan = fe._plan(224, 224)
    fe.sync(plan)
    _lib.check(lib.orbit_vit_enable_backward(plan.handle), "orbit_vit_enable_backward")
    return lib, plan


def _native(fe, frames, gamma, beta, dfeats, backward=True):
    """orbit_vit_train_forward (+ orbit_vit_backward) through the C-ABI on NaN-filled, guarded buffers."""
    lib, plan = _enabled_plan(fe)
    B, D, dev = frames.shape[0], fe.output_size, frames.device
    st = _lib.stream_handle()
    assert lib.orbit_vit_tape_bytes(plan.handle, B) == 109 * ((B * 197 * D * 4 + 255) // 256 * 256)
    tape = torch.empty(lib.orbit_vit_tape_bytes(plan.handle, B), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.orbit_vit_workspace_bytes(plan.handle, B), dtype=torch.uint8, device=dev)
    feats = torch.full((B + 1, D), float("nan"), device=dev)
    feats[B:] = 7777.0
    _lib.check(lib.orbit_vit_train_forward(plan.handle, _lib.dptr(frames), B, _lib.dptr(gamma), _lib.dptr(beta),
                                           _lib.dptr(feats), ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                           ctypes.c_void_p(ws.data_ptr()), ws.numel(), st), "orbit_vit_train_forward")
    if not backward:
        torch.cuda.synchronize()
        assert bool((feats[B:] == 7777.0).all())
        return feats[:B].cpu()
    n = fe.film_size
    dg = torch.full((n + D,), float("nan"), device=dev)
    db = torch.full((n + D,), float("nan"), device=dev)
    dg[n:], db[n:] = 7777.0, 7777.0
    bws = torch.full((lib.orbit_vit_backward_workspace_bytes(plan.handle, B) // 4,), float("nan"), device=dev)
    _lib.check(lib.orbit_vit_backward(plan.handle, B, _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(dfeats),
                                      ctypes.c_void_p(tape.data_ptr()), tape.numel(), _lib.dptr(dg), _lib.dptr(db),
                                      ctypes.c_void_p(bws.data_ptr()), 4 * bws.numel(), st), "orbit_vit_backward")
    torch.cuda.synchronize()
    assert bool((dg[n:] == 7777.0).all()) and bool((db[n:] == 7777.0).all()) and bool((feats[B:] == 7777.0).all())
    return feats[:B].cpu(), dg[:n].cpu(), db[:n].cpu()


def _native_case(name, B):
    key = ("native", name, B)
    if key not in _CACHE16:
        fe, _ = _pair(name)
        c = _case(name, B)
        _CACHE16[key] = _native(fe, c["frames"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), c["R"].cuda())
    return _CACHE16[key]


@pytest.mark.parametrize("with_film", [False, True], ids=["plain", "film"])
@pytest.mark.parametrize("B", [1, 3])
def test_taped_forward_is_the_inference_forward_bit_for_bit(device, B, with_film):
    fe, pin = _pair("vit_s_16")
    g = torch.Generator().manual_seed(B)
    frames = torch.randn(B, 3, 224, 224, generator=g).cuda()
    film = None
    if with_film:
        film = ((1 + 0.1 * torch.randn(fe.film_size, generator=g)).cuda(), (0.1 * torch.randn(fe.film_size, generator=g)).cuda())
    with torch.no_grad():
        want = fe(frames, film=film).cpu()
    got = _native(fe, frames, *(film or (None, None)), None, backward=False)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name,B", [("vit_s_16", 1), ("vit_s_16", 3), ("vit_b_16_clip", 1)])
def test_film_gradients_match_the_float64_pin(device, name, B):
    c = _case(name, B)
    feats, dg, db = _native_case(name, B)
    fe, _ = _pair(name)
    with torch.no_grad():
        assert torch.equal(feats, fe(c["frames"].cuda(), film=(c["gamma"].cuda(), c["beta"].cuda())).cpu())
    gate(dg, c["ref64"][0], c["e32"][0], "vit16 train %s B=%d dgamma" % (name, B))
    gate(db, c["ref64"][1], c["e32"][1], "vit16 train %s B=%d dbeta" % (name, B))


def test_film_generator_path_through_autograd(device):
    """A FilmParameterGenerator-produced FiLM dict: loss = sum(fe(x, film dict of generator(z)) * R) takes a gradient back to the
    generator's input z; against the float64 pin fed by oracle.blocks.FilmParameterGenerator with the same parameters."""
    from orbit_dataset_amd.model.feature_adapters import FilmParameterGenerator
    name, B, Z, HID = "vit_s_16", 3, 16, 16
    fe, pin = _pair(name)
    c = _case(name, B)
    slots, D = pin.film_slot_names(), pin.output_size
    own = dict(pin.named_parameters())
    sizes = {s + leaf: D for s in slots for leaf in (".weight", ".bias")}
    init = {n: own[n].detach().clone() for n in sizes}
    gen = FilmParameterGenerator(sizes, {k: v.clone() for k, v in init.items()}, Z, HID, slot_names=slots)
    g = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for q in gen.parameters():
            q.copy_(0.3 * torch.randn(q.shape, generator=g))
    state = {k: v.clone() for k, v in gen.state_dict().items()}
    z0 = torch.randn(1, Z, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        net = _pin(name, dtype)
        oracle_gen = blocks.FilmParameterGenerator(sizes, {k: v.to(dtype) for k, v in init.items()}, Z, HID).to(dtype)
        oracle_gen.load_state_dict(state)
        z = z0.clone().to(dtype).requires_grad_(True)
        (functional_call(net, oracle_gen(z), (c["frames"].to(dtype),)) * c["R"].to(dtype)).sum().backward()
        ref[dtype] = z.grad.double()
    e32 = (ref[torch.float32] - ref[torch.float64]).abs().max().item()
    gen = gen.to("cuda:0")
    z = z0.clone().cuda().requires_grad_(True)
    film = gen(z)
    gamma = torch.cat([film[s + ".weight"] for s in slots])
    beta = torch.cat([film[s + ".bias"] for s in slots])
    (fe(c["frames"].cuda(), film=(gamma, beta)) * c["R"].cuda()).sum().backward()
    gate(z.grad.cpu(), ref[torch.float64], e32, "vit16 train autograd z.grad (FilmParameterGenerator)")
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in gen.parameters())
    assert all(q.grad is None for q in fe.parameters())


def test_unfreeze_film_path_fills_the_50_layernorm_grads(device):
    """The multi-step finetuner's route: no film vectors, the FiLM-slot LayerNorm Parameters themselves require a gradient."""
    name, B = "vit_s_16", 3
    c = _case(name, B)
    fe, names = create_feature_extractor(name, with_film=True, learn_extractor=False)
    fe.load_state_dict(_pair(name)[1].state_dict(), strict=True)
    fe.eval().to("cuda:0")
    unfreeze_film(names, fe)
    frames, R = c["frames"].cuda(), c["R"].cuda()
    with torch.no_grad():
        fe(frames)  # the plan exists and has run inference before the attribute is set
    fe.native_backward_patch16 = True
    (fe(frames) * R).sum().backward()
    _, dg, db = _native(fe, frames, None, None, R)
    D = fe.output_size
    params = dict(fe.named_parameters())
    seen = set()
    for i, (slot, _) in enumerate(fe.film_slot_modules()):
        for leaf, want in ((".weight", dg), (".bias", db)):
            p = params[slot + leaf]
            assert p.grad is not None and torch.equal(p.grad.cpu(), want[i * D:(i + 1) * D]), slot + leaf
            seen.add(slot + leaf)
    assert len(seen) == 50
    assert all(p.grad is None for n, p in params.items() if n not in seen)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        net = _pin(name, dtype)
        for n, q in net.named_parameters():
            q.requires_grad_(n in seen)
        (net(c["frames"].to(dtype)) * c["R"].to(dtype)).sum().backward()
        ref[dtype] = {n: q.grad.double() for n, q in net.named_parameters() if n in seen}
    ref64, ref32 = ref[torch.float64], ref[torch.float32]
    order = [s for s, _ in fe.film_slot_modules()]
    for leaf, got in ((".weight", dg), (".bias", db)):
        r64 = torch.cat([ref64[s + leaf] for s in order])
        e32 = (torch.cat([ref32[s + leaf] for s in order]) - r64).abs().max().item()
        gate(got, r64, e32, "vit16 train unfreeze_film d" + leaf[1:])


def test_gradients_add_over_frames_and_runs_are_bitwise_equal(device):
    name = "vit_s_16"
    fe, _ = _pair(name)
    c = _case(name, 3)
    args = (c["gamma"].cuda(), c["beta"].cuda())
    _, dg3, db3 = _native_case(name, 3)
    again = _native(fe, c["frames"].cuda(), *args, c["R"].cuda())
    assert all(torch.equal(a, b) for a, b in zip(_native_case(name, 3), again)), "two backward runs differ"
    sg, sb = torch.zeros_like(dg3, dtype=torch.float64), torch.zeros_like(db3, dtype=torch.float64)
    for i in range(3):
        _, a, b = _native(fe, c["frames"][i:i + 1].cuda(), *args, c["R"][i:i + 1].cuda())
        sg, sb = sg + a.double(), sb + b.double()
    # both sides are within the gate of the float64 gradient of the batch, which is the sum of the frames' gradients
    gate(sg.float(), c["ref64"][0], c["e32"][0], "vit16 train additivity dgamma (sum of 3 single frames)")
    gate(sb.float(), c["ref64"][1], c["e32"][1], "vit16 train additivity dbeta (sum of 3 single frames)")
    for got, summed, ref, e32 in ((dg3, sg, c["ref64"][0], c["e32"][0]), (db3, sb, c["ref64"][1], c["e32"][1])):
        tol = max(4 * e32, 8 * 2.0 ** -24 * ref.abs().max().item())
        diff = (got.double() - summed).abs().max().item()
        print("[vit16-train] additivity: |batch - sum of frames| %.3g  e32 %.3g  ratio %.2f" % (diff, e32, diff / e32))
        assert diff <= tol


def test_backward_after_a_parameter_upload_is_refused(device):
    name = "vit_s_16"
    fe, names = create_feature_extractor(name, with_film=True, learn_extractor=False)
    fe.load_state_dict(_pair(name)[1].state_dict(), strict=True)
    fe.eval().to("cuda:0")
    fe.native_backward_patch16 = True
    x = _case(name, 1)["frames"].cuda()
    g = torch.ones(fe.film_size, device="cuda:0", requires_grad=True)
    loss = fe(x, film=(g, torch.zeros_like(g))).sum()
    with torch.no_grad():
        fe.norm.bias.add_(0.5)
        fe(x)  # re-uploads the parameters into the plan
    with pytest.raises(RuntimeError, match="modified .* between the forward"):
        loss.backward()
    loss = fe(x, film=(g, torch.zeros_like(g))).sum()
    loss.backward()  # a fresh tape under the new parameters runs
    assert torch.isfinite(g.grad).all()


def test_refusals(device, lib):
    x = torch.zeros(1, 3, 224, 224, device="cuda:0")
    fe, _ = create_feature_extractor("vit_s_16", with_film=True, learn_extractor=False)
    fe.to("cuda:0")
    g = torch.ones(fe.film_size, device="cuda:0", requires_grad=True)
    assert fe.native_backward_patch16 is False
    fe.native_backward = fe.native_weight_backward = True  # the patch-32 opt-ins open nothing here
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe(x, film=(g, torch.zeros_like(g)))
    assert not fe._plans
    fe2, _ = create_feature_extractor("vit_s_16", with_film=True, learn_extractor=True)
    fe2.to("cuda:0")
    fe2.native_backward_patch16 = True
    with pytest.raises(NotImplementedError, match="first: cls_token"):
        fe2(x)
    with pytest.raises(NotImplementedError, match="first: cls_token"):
        fe2(x, film=(g, torch.zeros_like(g)))
    assert not fe2._plans, "a plan was built (parameters uploaded) before the refusal"
    fe2.requires_grad_(False)
    fe2.patch_embed.proj.weight.requires_grad_(True)  # one non-FiLM parameter is enough
    with pytest.raises(NotImplementedError, match="patch_embed.proj.weight"):
        fe2(x)
    with torch.no_grad():
        assert fe2(x).shape == (1, 384)
    # weight gradients on the enabled, finalized plan: refused by the library before any launch
    fe3, _ = _pair("vit_s_16")
    _, plan = _enabled_plan(fe3)
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


def test_learner_lite_training_smoke(device, lib):
    """learner --mode train --feature_extractor vit_s_16 --adapt_features --with_lite --vit16_native_backward: one 2-way task of a
    handful of frames per optimizer step, two steps."""
    from orbit_dataset_amd import learner
    args = learner.build_parser().parse_args(
        ["--mode", "train", "--feature_extractor", "vit_s_16", "--adapt_features", "--with_lite", "--vit16_native_backward",
         "--way", "2", "--shots", "1", "--frames_per_shot", "3", "--num_query_videos", "1", "--frames_per_video", "2",
         "--num_train_tasks", "2", "--tasks_per_batch", "1", "--num_lite_samples", "2", "--batch_size", "4",
         "--learning_rate", "1e-3"])
    learner.verify_args(args)
    L = learner.Learner(args)
    fe = L.model.feature_extractor
    assert fe.native_backward_patch16 is True and fe.native_backward is False and fe.native_weight_backward is False
    gen_params = [p for p in L.model.film_generator.parameters() if p.requires_grad]
    assert gen_params
    snaps = [[p.detach().clone() for p in gen_params]]
    grads = []

    def hook(opt, a, k):
        grads.append([None if p.grad is None else p.grad.detach().clone() for p in L.model.set_encoder.parameters()])
        snaps.append([p.detach().clone() for p in gen_params])

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
    for before, after in zip(snaps, snaps[1:]):
        assert any(not torch.equal(a, b) for a, b in zip(before, after)), "FiLM-generator parameters did not change"
        assert all(torch.isfinite(a).all() for a in after)
    # per task the query batch's tape, 12 blocks (tests/test_gpu_vit_train.py)
    assert rows.get("vit_attention197_bwd", 0) == 2 * 12, rows
    assert rows.get("vit_attention_bwd", 0) == 0, rows
    assert all(any(g is not None and bool((g != 0).any()) for g in step) for step in grads)
    assert all(p.grad is None for p in fe.parameters())


def test_finetuner_step(device, lib):
    """multi-step-learner --adapt_features --vit16_native_backward --personalize_num_grad_steps 1 on a tiny task: the FineTuner's
    step runs the 197-token backward and the logits are finite. The linear head starts at zero (reference classifier_heads.py),
    so the gradient that reaches the extractor in the FIRST step is exactly zero and Adam leaves the FiLM parameters where they
    are; that a FiLM parameter (a FiLM-slot LayerNorm weight / bias of the extractor) moves is shown with a second step."""
    from orbit_dataset_amd import learner
    args = learner.build_multistep_parser().parse_args(
        ["--feature_extractor", "vit_s_16", "--adapt_features", "--vit16_native_backward", "--personalize_num_grad_steps", "1",
         "--way", "2", "--shots", "1", "--frames_per_shot", "3", "--num_query_videos", "1", "--frames_per_video", "2",
         "--batch_size", "4"])
    learner.verify_args(args)
    L = learner.MultiStepLearner(args)
    fe = L.model.feature_extractor
    assert fe.native_backward_patch16 is True
    task = L.make_task(0)
    lo, hi = task["target_videos"][0]
    L.model.set_test_mode(True)
    slots = [s for s, _ in fe.film_slot_modules()]

    def moved():
        state = L.model.state_dict()
        return [k for k in state if any(k.endswith(s + leaf) for s in slots for leaf in (".weight", ".bias"))
                and not torch.equal(state[k].cpu(), L.base_state[k].cpu())]

    for steps in (1, 2):
        L.model.load_state_dict(L.base_state, strict=False)
        lib.orbit_prof_enable(1)
        try:
            L.model.personalise(task["context_clips"], task["context_labels"].to(L.device),
                                dict(L.learning_args(), num_grad_steps=steps))
            rows = _prof_rows(lib)
        finally:
            lib.orbit_prof_enable(0)
        assert rows.get("vit_attention197_bwd", 0) == steps * 2 * 12, rows  # 6 context clips in mini-batches of 4
        with torch.no_grad():
            out = L.model.predict(attach_frame_history(task["target_clips"][lo:hi, 0], 1)).detach().cpu()
        assert torch.isfinite(out).all() and out.shape[-1] == 2
        if steps == 2:
            assert moved(), "no FiLM parameter changed"
            assert all(torch.isfinite(p).all() for p in fe.parameters())
        L.model._reset()
