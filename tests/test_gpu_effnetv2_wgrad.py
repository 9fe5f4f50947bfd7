"""Native training of efficientnet_v2_s end to end (ORBIT_PLAN_RES_POST_TRAINING, EfficientNetV2S.native_weight_backward,
--effnetv2_native_weight_backward): batch-statistics forward, running-statistics updates and the gradient of every parameter
from orbit_extractor_train_forward / orbit_extractor_backward, against the CPU pin (tests/effnetv2_pin.py) in train() evaluated
in float64 with torch autograd.

Gates. Features: that of tests/test_gpu_effnetv2.py, max(FEAT_TOL, 4 x E32). Every parameter gradient and every running
statistic (tests/test_gpu_vit_ops.gate): max |got - ref64| <= max(4 * e32, 8 * 2**-24 * max |ref64|), e32 = the float32 pin's own
error against the float64 pin on the same inputs, measured here. The pin holds 450 parameters (110 convolutions, 110 BatchNorm
pairs, 30 squeeze-excite blocks of four) and 110 BatchNorms; the counts are taken from it. Each test prints its largest err / e32
(run with -s). The operators one by one: tests/test_gpu_effnetv2_wgrad_ops.py.

Largest err / e32 seen on the MI355X, gradients / running statistics: 2.38 / 2.41 (64 x 64, B = 4), 3.27 / 1.85 (70 x 54, B = 3),
1.82 / 1.90 (224 x 224, B = 1); with the FiLM pair 2.57 (FiLM) / 2.50 / 2.14; eval() 3.02. Smallest batch variance of a BatchNorm
channel in the float64 pin: 2.0e-03 / 2.6e-03 / 9.7e-03.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.func import functional_call

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
import effnetv2_pin  # noqa: E402
from test_gpu_effnetv2 import FEAT_TOL, LOGIT_TOL, NAME, feat_err  # noqa: E402
from test_gpu_vit_ops import gate  # noqa: E402
from oracle.recogniser import OracleRecogniser  # noqa: E402
from oracle.training import LiteTrainer  # noqa: E402
from orbit_dataset_amd import _lib, synthetic  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor  # noqa: E402
from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser  # noqa: E402

# H, W, frames, seed. 64x64: the last maps are 2 x 2, 16 rows per BatchNorm channel; 70x54: both padding parities; 224x224: many-split
# filter gradients, and more dense convolutions / squeeze-excite blocks than one job list of the batched reductions holds
CASES = {"64x64": (64, 64, 4, 1), "70x54": (70, 54, 3, 2), "224x224": (224, 224, 1, 3)}
_CACHE = {}


def _state():
    """the synthetic parameters every network of this file starts from (float32 state_dict of the pin)"""
    if "sd" not in _CACHE:
        pin = effnetv2_pin.EfficientNet()
        synthetic.init_parameters_(pin)
        _CACHE["sd"] = {k: v.clone() for k, v in pin.state_dict().items()}
        assert len(list(pin.parameters())) == 450 and sum(isinstance(m, nn.BatchNorm2d) for m in pin.modules()) == 110
    return _CACHE["sd"]


def _pin(dtype, train=True):
    net = effnetv2_pin.EfficientNet().to(dtype)
    net.load_state_dict(_state())
    return net.train(train)


def _extractor(train=True):
    """the HIP extractor on cuda:0 under the second opt-in, reset to the initial parameters and running statistics"""
    if "fe" not in _CACHE:
        fe, names = create_feature_extractor(NAME, True, True, True)
        fe.native_weight_backward = True
        _CACHE["fe"], _CACHE["film_names"] = fe.cuda(), names
    fe = _CACHE["fe"]
    fe.load_state_dict(_state(), strict=True)
    fe.requires_grad_(True)
    fe.zero_grad(set_to_none=True)
    return fe.train(train)


def _reference(key, train=True, film=False):
    """float64 and float32 pin on one case: features, gradients of sum(feats * R) w.r.t. every parameter (and the 84 FiLM
    tensors with film=True), the state_dict after the forward, e32 of each; computed once."""
    ck = (key, train, film)
    if ck not in _CACHE:
        H, W, B, seed = CASES[key]
        g = torch.Generator().manual_seed(H * 1000 + W + seed)
        frames = torch.randn(B, 3, H, W, generator=g)
        R = torch.randn(B, 1280, generator=g)
        films = None
        if film:
            _extractor()
            films = {}
            for n in _CACHE["film_names"]:
                p = _state()[n]
                films[n] = p * (1 + 0.03 * torch.randn(p.shape, generator=g)) + 0.0075 * torch.randn(p.shape, generator=g)
        out = {}
        min_var = [float("inf")]
        for dtype in (torch.float64, torch.float32):
            net = _pin(dtype, train)
            handles = []
            if dtype == torch.float64 and train:
                def hook(m, inp, _o):
                    min_var[0] = min(min_var[0], inp[0].var((0, 2, 3), unbiased=False).min().item())
                handles = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
            leaves = {n: t.to(dtype).clone().requires_grad_(True) for n, t in films.items()} if film else {}
            feats = functional_call(net, leaves, (frames.to(dtype),)) if film else net(frames.to(dtype))
            (feats * R.to(dtype)).sum().backward()
            for h in handles:
                h.remove()
            grads = {n: p.grad.double() for n, p in net.named_parameters() if p.grad is not None}
            out[dtype] = dict(feats=feats.detach(), grads=grads, fgrads={n: t.grad.double() for n, t in leaves.items()},
                              sd={k: v.detach().double() for k, v in net.state_dict().items()})
        r64, r32 = out[torch.float64], out[torch.float32]
        assert torch.isfinite(r64["feats"]).all() and r64["feats"].abs().max().item() < 50, "pin features left the calibrated regime"
        if train:
            print("\n[effnetv2-wgrad] %s: smallest batch variance over all BatchNorm channels of the float64 pin %.3g" % (key, min_var[0]))
            assert min_var[0] >= 1e-6, "a near-constant channel: change this case's seed"
        e = lambda a, b: (a.double() - b).abs().max().item()
        _CACHE[ck] = dict(frames=frames, R=R, films=films, feats64=r64["feats"], grads64=r64["grads"], fgrads64=r64["fgrads"],
                          sd64=r64["sd"], feat_e32=feat_err(r32["feats"], r64["feats"]),
                          e32={n: e(r32["grads"][n], r64["grads"][n]) for n in r64["grads"]},
                          fe32={n: e(r32["fgrads"][n], r64["fgrads"][n]) for n in r64["fgrads"]},
                          sd_e32={k: e(r32["sd"][k], v) for k, v in r64["sd"].items()})
    return _CACHE[ck]


def _gate_grads(fe, c, what, skip=()):
    params = dict(fe.named_parameters())
    assert set(params) >= set(c["grads64"])
    worst, where = 0.0, ""
    for n, ref in c["grads64"].items():
        if n in skip:
            continue
        assert params[n].grad is not None, n
        r = gate(params[n].grad.cpu(), ref, c["e32"][n], "%s %s" % (what, n))
        if r > worst:
            worst, where = r, n
    print("\n[effnetv2-wgrad] %s: largest err / e32 over %d parameter gradients %.2f (%s)"
          % (what, len(c["grads64"]) - len(skip), worst, where))


def _gate_stats(fe, c, what):
    sd = {k: v.cpu() for k, v in fe.state_dict().items()}
    worst, n = 0.0, 0
    for k, ref in c["sd64"].items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(ref), k  # (the pin's counter: one more than before after a train() forward)
        elif k.endswith(("running_mean", "running_var")):
            worst = max(worst, gate(sd[k], ref, c["sd_e32"][k], "%s %s" % (what, k)))
            n += 1
    assert n == 220
    print("\n[effnetv2-wgrad] %s: largest err / e32 over the running statistics of 110 BatchNorms %.2f" % (what, worst))


def _check_features(c, feats, what):
    bound = max(FEAT_TOL, 4 * c["feat_e32"])
    err = feat_err(feats, c["feats64"])
    print("\n[effnetv2-wgrad] %s: features err %.3g vs the float64 pin, E32 %.3g, bound %.3g" % (what, err, c["feat_e32"], bound))
    assert torch.isfinite(feats).all() and err <= bound, (what, err, bound)


@pytest.mark.parametrize("key", list(CASES))
def test_training_step_against_the_float64_pin(device, key):
    """train(): features under batch statistics, every parameter gradient, every running statistic, the step counters."""
    c = _reference(key)
    fe = _extractor()
    feats = fe(c["frames"].cuda())
    (feats * c["R"].cuda()).sum().backward()
    _check_features(c, feats.detach().cpu(), key)
    assert all(p.grad is not None for p in fe.parameters()), "the module's backward() left a .grad unfilled"
    assert len(c["grads64"]) == 450
    _gate_grads(fe, c, key)
    _gate_stats(fe, c, key)
    assert int(fe.bn1.num_batches_tracked) == int(_state()["bn1.num_batches_tracked"]) + 1


def test_film_pair_and_every_parameter_together(device):
    """The `film=` pair requires a gradient as well (LITE with --adapt_features --learn_extractor): the 84 FiLM gradients and
    the gradients of every parameter the forward still reads (the 84 replaced BatchNorm tensors get none, as in the pin)."""
    c = _reference("64x64", film=True)
    fe = _extractor()
    slots = [n for n, _ in fe.film_slot_modules()]
    gamma = torch.cat([c["films"][s + ".weight"] for s in slots]).cuda().requires_grad_(True)
    beta = torch.cat([c["films"][s + ".bias"] for s in slots]).cuda().requires_grad_(True)
    feats = fe(c["frames"].cuda(), film=(gamma, beta))
    (feats * c["R"].cuda()).sum().backward()
    _check_features(c, feats.detach().cpu(), "64x64 film=")
    assert len(c["fgrads64"]) == 84 and len(c["grads64"]) == 450 - 84
    worst, off = 0.0, 0
    for s, (_, m) in zip(slots, fe.film_slot_modules()):
        C = m.weight.numel()
        for leaf, vec in ((".weight", gamma.grad), (".bias", beta.grad)):
            n = s + leaf
            worst = max(worst, gate(vec[off:off + C].cpu(), c["fgrads64"][n], c["fe32"][n], "64x64 film= d " + n))
        off += C
    print("\n[effnetv2-wgrad] 64x64 film=: largest err / e32 over the 84 FiLM gradients %.2f" % worst)
    _gate_grads(fe, c, "64x64 film=")
    _gate_stats(fe, c, "64x64 film=")


def test_eval_mode_filter_gradients_through_the_frozen_batchnorm(device):
    """eval() under the opt-in: running statistics, the gradient of every parameter through the frozen BatchNorm, statistics and
    step counters untouched."""
    c = _reference("64x64", train=False)
    fe = _extractor(train=False)
    feats = fe(c["frames"].cuda())
    (feats * c["R"].cuda()).sum().backward()
    _check_features(c, feats.detach().cpu(), "64x64 eval()")
    _gate_grads(fe, c, "64x64 eval()")
    sd = fe.state_dict()
    for k, v in _state().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(sd[k].cpu(), v), k
    _gate_stats(fe, c, "64x64 eval()")


def test_two_runs_are_bitwise_equal(device):
    """No atomics anywhere on this path: features, every gradient and every running statistic of two runs of one case agree
    bit for bit (the second replays what the first ran eagerly)."""
    c = _reference("70x54")
    runs = []
    for _ in range(2):
        fe = _extractor()
        feats = fe(c["frames"].cuda())
        (feats * c["R"].cuda()).sum().backward()
        runs.append((feats.detach().cpu(), {n: p.grad.cpu() for n, p in fe.named_parameters()},
                     {k: v.cpu() for k, v in fe.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_one_trainable_filter_in_a_frozen_network(device):
    c = _reference("64x64")
    fe = _extractor()
    fe.requires_grad_(False)
    fe.conv_stem.weight.requires_grad_(True)
    feats = fe(c["frames"].cuda())
    (feats * c["R"].cuda()).sum().backward()
    r = gate(fe.conv_stem.weight.grad.cpu(), c["grads64"]["conv_stem.weight"], c["e32"]["conv_stem.weight"], "only conv_stem.weight")
    print("\n[effnetv2-wgrad] only conv_stem.weight trainable: err / e32 %.2f" % r)
    assert all(p.grad is None for n, p in fe.named_parameters() if n != "conv_stem.weight")


def test_per_block_squeeze_excite_gradients_pass_the_same_gate(device):
    """ORBIT_FILTER_GRADS_SE_PER_BLOCK (HipNetwork.se_param_grads_per_block, the A/B form of tools/effnetv2_bench.py): the 120
    squeeze-excite parameter gradients from the per-block kernel."""
    c = _reference("64x64")
    fe = _extractor()
    fe.se_param_grads_per_block = True
    try:
        (fe(c["frames"].cuda()) * c["R"].cuda()).sum().backward()
    finally:
        del fe.se_param_grads_per_block
    se = [n for n in c["grads64"] if ".se." in n]
    assert len(se) == 120
    _gate_grads(fe, c, "64x64 per-block se", skip=[n for n in c["grads64"] if ".se." not in n])


def test_the_first_opt_in_alone_still_refuses(device, lib):
    fe, _ = create_feature_extractor(NAME, True, True, True)
    fe.load_state_dict(_state(), strict=True)
    fe.cuda()
    fe.native_backward = True
    x = torch.zeros(2, 3, 64, 64, device="cuda:0")
    fe.train()
    with pytest.raises(NotImplementedError):
        fe(x)
    fe.eval()
    with pytest.raises(NotImplementedError):
        fe(x)  # own parameters that require a gradient
    assert not fe._plans
    # and the C-ABI on a flags-3 plan
    plan = fe._plan(64, 64, trainable=True)
    fe.sync(plan)
    B = 2
    feats, dfeats = torch.zeros(B, 1280, device="cuda:0"), torch.zeros(B, 1280, device="cuda:0")
    tape = torch.empty(lib.orbit_extractor_tape_bytes(plan.handle, B), dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(lib.orbit_extractor_backward_workspace_bytes(plan.handle, B), dtype=torch.uint8, device="cuda:0")
    flat = torch.zeros(lib.orbit_extractor_grad_floats(plan.handle), device="cuda:0")
    tp, st = ctypes.c_void_p(tape.data_ptr()), _lib.stream_handle()
    for flags in (0, 1, 3):
        assert lib.orbit_extractor_train_forward_ex(plan.handle, _lib.dptr(x), B, None, None, 1, 0.1, _lib.dptr(feats), tp,
                                                    tape.numel(), flags, st) != 0
    for bn_train, filter_grads in ((0, 1), (1, 0), (1, 1), (0, 2)):
        assert lib.orbit_extractor_backward(plan.handle, _lib.dptr(x), B, None, None, bn_train, _lib.dptr(dfeats), tp, tape.numel(),
                                            _lib.dptr(flat), filter_grads, None, None, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                            st) != 0
    torch.cuda.synchronize()
    assert not feats.any() and not flat.any()
    # the same instance under the second opt-in builds another plan and runs
    fe.native_weight_backward = True
    fe.train()
    out = fe(x)
    assert len(fe._plans) == 2 and torch.isfinite(out).all()


def test_recogniser_lite_step(device):
    """SingleStepFewShotRecogniser(learn_extractor, proto), 3-way at 64 x 64: one LITE step - train-mode cache pass under
    no_grad, the taped subset, the taped query batch - against the same step on the float64 pin in train() inside the oracle's
    LiteTrainer (BatchNorm mode rule: reference few_shot_recognisers.py:176-183)."""
    H = 4
    model = SingleStepFewShotRecogniser(NAME, False, "proto", 1, 8, True, H, 1.0)
    synthetic.init_parameters_(model)
    model.feature_extractor.native_weight_backward = True
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(False)
    assert model.feature_extractor.training
    task = synthetic.make_task(3, way=3, shots=1, frames_per_shot=2, num_query=6, frame_size=64, template="blobs")
    ctx, lab, tgt, tlab = task["context_clips"], task["context_labels"], task["target_clips"], task["target_labels"]
    sd = {k[len("feature_extractor."):]: v.cpu().clone() for k, v in model.state_dict().items() if k.startswith("feature_extractor.")}
    np.random.seed(7)
    model.personalise_with_lite(ctx.cuda(), lab.cuda())
    loss = F.cross_entropy(model.predict_a_batch(tgt.cuda()), tlab.cuda())
    loss.backward()
    params = dict(model.feature_extractor.named_parameters())
    for n, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert bool((params["conv_stem.weight"].grad != 0).any()) and bool((params["blocks.5.14.se.conv_reduce.weight"].grad != 0).any())
    ref = OracleRecogniser("resnet18", False, "proto", 1, 8, num_lite_samples=H)
    ref.fe = effnetv2_pin.EfficientNet()
    ref.fe.load_state_dict(sd)
    ref.fe.double()
    trainer = LiteTrainer(ref, True, 1)
    ref.clear_caches()
    np.random.seed(7)
    trainer.personalise_with_lite(ctx.double(), lab)
    want = F.cross_entropy(trainer.predict_a_batch(tgt.double()), tlab)
    want.backward()
    assert ref.fe.training
    print("\n[effnetv2-wgrad] LITE step loss %.6f, float64 oracle %.6f" % (loss.item(), want.item()))
    assert abs(loss.item() - want.item()) < LOGIT_TOL
    # the running statistics went through the same three train-mode forwards
    got_sd = {k: v.cpu() for k, v in model.feature_extractor.state_dict().items()}
    want_sd = ref.fe.state_dict()
    assert int(got_sd["bn1.num_batches_tracked"]) == int(want_sd["bn1.num_batches_tracked"]) == 3
    for k in ("bn1.running_mean", "bn2.running_var", "blocks.5.14.bn2.running_var"):
        assert (got_sd[k].double() - want_sd[k]).abs().max().item() <= 1e-4 * max(1.0, want_sd[k].abs().max().item()), k


def test_learner_lite_training_smoke(device):
    """learner --mode train --learn_extractor --with_lite --effnetv2_native_weight_backward: two tasks at 64 x 64."""
    from orbit_dataset_amd import learner
    args = learner.build_parser().parse_args(
        ["--mode", "train", "--feature_extractor", NAME, "--learn_extractor", "--with_lite", "--effnetv2_native_weight_backward",
         "--frame_size", "64", "--way", "2", "--shots", "1", "--frames_per_shot", "3", "--num_query_videos", "1",
         "--frames_per_video", "4", "--num_train_tasks", "2", "--tasks_per_batch", "1", "--num_lite_samples", "4",
         "--batch_size", "8", "--learning_rate", "1e-3"])
    L = learner.Learner(args)
    fe = L.model.feature_extractor
    assert fe.native_weight_backward is True and args.frame_norm_method == "imagenet_inception"
    watched = ("conv_stem.weight", "blocks.1.0.conv_exp.weight", "blocks.5.14.se.conv_expand.weight", "bn2.weight")
    before = {k: v.detach().cpu().clone() for k, v in fe.state_dict().items()}
    stats = L.train()
    assert stats["num_tasks"] == 2
    assert stats["loss"][0] is not None and np.isfinite(stats["loss"][0])
    after = {k: v.detach().cpu() for k, v in fe.state_dict().items()}
    for k in watched:
        assert torch.isfinite(after[k]).all() and not torch.equal(before[k], after[k]), k + " did not change"
    assert int(after["bn1.num_batches_tracked"]) > int(before["bn1.num_batches_tracked"])
    assert not torch.equal(before["bn1.running_mean"], after["bn1.running_mean"])
