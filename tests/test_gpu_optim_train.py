"""The training recipe end to end on resnet18 at 32 x 32, 2-way synthetic tasks, 2 optimizer steps per epoch: the native optimizer
against torch's, the schedule as the optimizer sees it in every step, checkpoint + resume against a straight run, and the
FineTuner's personalise() with the native step.

The agreement rule ("the rule of (a)"): two runs of the DEFAULT optimizer on identical tasks give the spread of the training step
itself, as one relative number: spread = max over tensors of max|a - b| / max|a|. A native run must agree with the default run
within 4 x spread x max|tensor|, per tensor. Where the two default runs are bit-identical the rule falls back on the operator
test's bound (tests/test_gpu_optim_ops.py: 2 x torch's own fp32 deviation + 1e-7 x max|p|) scaled by the number of optimizer
steps. There is no float64 training run to measure torch's deviation against, so the yardstick is the one torch itself offers:
its two fp32 Adam steps that the learner can select, the default (`fused=False`, which is torch's single-tensor path: it
multiplies sqrt(v) by the reciprocal of sqrt(1 - beta2^t)) and `--fused_optimizer`. With torch_dev = max over tensors of
max|fused - default| / max|default|, the fallback bound is (2 x torch_dev + steps x 1e-7) x max|tensor|. The native step itself
is bit-identical to torch's FOREACH path (the operator test prints max|native - torch_fp32| = 0), which divides where the
single-tensor path multiplies by a reciprocal; Adam's m / (sqrt(v) + eps) then amplifies such last-bit differences wherever a
gradient element is close to zero, in torch's own variants as here. Which branch held is printed by the tests.
(A first version of this file assumed one ulp per step for torch's own deviation, 4.6e-7 x max|tensor| per step, and no
amplification through the following steps; the native run differed from the single-tensor default by 5.4e-7 x max|tensor| on
one tensor after 4 steps under it.)"""
import copy

import pytest
import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import learner, optim
from orbit_dataset_amd.data.utils import attach_frame_history

pytestmark = pytest.mark.gpu

MODEL = ["--feature_extractor", "resnet18", "--learn_extractor", "--frame_size", "32", "--way", "2", "--shots", "1",
         "--frames_per_shot", "3", "--num_query_videos", "1", "--frames_per_video", "4", "--batch_size", "8"]
TRAIN = MODEL + ["--mode", "train", "--num_train_tasks", "2", "--tasks_per_batch", "1", "--learning_rate", "1e-3"]
# one schedule for every run of (a) and (c), with a fixed --decay_epochs: f(0) = 1e-4 (warm-up), f(1) = 1e-3
SCHEDULE = ["--scheduler", "multistep", "--warmup_epochs", "1", "--warmup_lr", "1e-4", "--decay_epochs", "2"]


def run(argv):
    L = learner.Learner(learner.build_parser().parse_args(argv))
    stats = L.train()
    return stats, {k: v.detach().cpu().clone() for k, v in L.model.state_dict().items()}, L


def floats(state):
    return {k: v for k, v in state.items() if v.is_floating_point()}


def spread_of(a, b):
    return max(((a[k] - b[k]).abs().max() / a[k].abs().max().clamp_min(1e-30)).item() for k in floats(a))


def assert_agree(got, want, spread, torch_dev, steps, what):
    """the module docstring's rule; prints which branch held and the worst figure against its bound"""
    rel = 4 * spread if spread > 0 else 2 * torch_dev + steps * 1e-7
    worst = 0.0
    for k, w in want.items():
        if not w.is_floating_point():
            assert torch.equal(got[k], w), k
            continue
        err, bound = (got[k] - w).abs().max().item(), rel * w.abs().max().item()
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
        assert err <= bound, "%s: %s differs by %.3e > %.3e" % (what, k, err, bound)
    print("%s: %s; worst |difference| / bound = %.3g" % (what, "within 4 x the spread %.3e of two default runs" % spread if spread > 0
          else "default runs bit-identical: operator bound, torch's fused vs default deviation %.3e, %d steps (%.3e relative)"
          % (torch_dev, steps, rel), worst))


@pytest.fixture(scope="module")
def runs(device, lib, tmp_path_factory):
    """computed once: two default runs, the native run (which also writes the checkpoints of the straight run)"""
    straight = tmp_path_factory.mktemp("straight")
    base = TRAIN + SCHEDULE + ["--epochs", "2"]
    first, second, fused = run(base), run(base), run(base + ["--fused_optimizer"])
    native = run(base + ["--native_optimizer", "--checkpoint_dir", str(straight)])
    return {"default": first, "again": second, "native": native, "spread": spread_of(first[1], second[1]),
            "torch_dev": spread_of(first[1], fused[1]), "dir": straight, "steps": 4}


def test_native_against_torch(runs):
    stats, state, L = runs["native"]
    assert type(L.optimizer) is optim.NativeAdam and type(runs["default"][2].optimizer) is torch.optim.Adam
    assert stats["num_tasks"] == 4 and all(torch.isfinite(v).all() for v in floats(state).values())
    # training moved the parameters by far more than the bound below
    before = {k: v.detach().cpu() for k, v in learner.Learner(learner.build_parser().parse_args(TRAIN)).model.state_dict().items()}
    moved = max((state[k] - before[k]).abs().max().item() for k in floats(state))
    assert moved > 1e-4, moved
    assert_agree(state, runs["default"][1], runs["spread"], runs["torch_dev"], runs["steps"],
                 "native vs torch optimizer, 4 steps")
    # the same state keys and shapes as torch.optim.Adam's
    want = runs["default"][2].optimizer.state_dict()
    got = L.optimizer.state_dict()
    # (the learner builds its torch optimizer with fused=False where torch's own default, and NativeAdam's entry, is None)
    strip = lambda groups: [{k: v for k, v in g.items() if k != "fused"} for g in groups]  # noqa: E731
    assert strip(got["param_groups"]) == strip(want["param_groups"]) and got["state"].keys() == want["state"].keys()
    assert got["param_groups"][0].keys() == want["param_groups"][0].keys()
    for k, s in want["state"].items():
        assert s.keys() == got["state"][k].keys()
        assert float(got["state"][k]["step"]) == float(s["step"]) == 4.0 and got["state"][k]["step"].device.type == "cpu"
        assert got["state"][k]["exp_avg"].shape == s["exp_avg"].shape


def test_schedule_reaches_every_step(device, lib):
    args = Namespace_of(TRAIN + ["--scheduler", "multistep", "--warmup_epochs", "1", "--decay_epochs", "2", "--epochs", "3",
                                 "--extractor_lr_scale", "0.1", "--native_optimizer"])
    f = optim.schedule_fn(args)[0]
    # the host test's anchors for these arguments: warm-up from 1e-6, milestone 2 taking effect at epoch 1
    assert [f(t) for t in range(3)] == [1e-6, 1e-3 * 0.5, 1e-3 * 0.5]
    seen = []
    handle = register_optimizer_step_post_hook(
        lambda opt, a, k: seen.append(tuple(g["lr"] for g in opt.param_groups)))
    try:
        L = learner.Learner(args)
        stats = L.train()
    finally:
        handle.remove()
    want = [(f(epoch), f(epoch) * 0.1) for epoch in range(3)]
    assert seen == [want[epoch] for epoch in range(3) for _ in range(2)]
    assert [tuple(x) for x in stats["lr_history"]] == want and (stats["lr"], stats["fe_lr"]) == want[-1]
    assert optim.get_curr_learning_rates(L.optimizer) == [f(3), f(3) * 0.1]  # step(epoch + 1) ran after the last epoch


def Namespace_of(argv):
    return learner.build_parser().parse_args(argv)


def test_resume_equals_the_straight_run(runs, tmp_path):
    straight_stats, straight, L = runs["native"]
    checkpoint = torch.load(str(runs["dir"] / "checkpoint.pt"), map_location="cpu")
    assert set(checkpoint) == {"epoch", "model_state_dict", "optimizer_state_dict", "best_stats"} and checkpoint["epoch"] == 2
    for k, v in straight.items():
        assert torch.equal(checkpoint["model_state_dict"][k], v), k
    # the optimizer state loads into a plain torch.optim.Adam over the same groups
    plain = torch.optim.Adam([{"params": g["params"]} for g in L.optimizer.param_groups], lr=1.0)
    plain.load_state_dict(copy.deepcopy(checkpoint["optimizer_state_dict"]))
    assert [g["lr"] for g in plain.param_groups] == optim.get_curr_learning_rates(L.optimizer)
    state = plain.state[L.optimizer.param_groups[1]["params"][0]]
    assert float(state["step"]) == 4.0 and state["exp_avg"].is_cuda and state["exp_avg_sq"].abs().max() > 0
    # stop after one epoch, then resume to two
    base = TRAIN + SCHEDULE + ["--native_optimizer", "--checkpoint_dir", str(tmp_path)]
    stopped_stats, stopped, _ = run(base + ["--epochs", "1"])
    assert torch.load(str(tmp_path / "checkpoint.pt"), map_location="cpu")["epoch"] == 1
    assert stopped_stats["lr_history"] == straight_stats["lr_history"][:1]
    resumed_stats, resumed, _ = run(base + ["--epochs", "2", "--resume"])
    assert resumed_stats["start_epoch"] == 1 and resumed_stats["num_tasks"] == 2
    assert resumed_stats["lr_history"] == straight_stats["lr_history"][1:]
    assert any(not torch.equal(resumed[k], stopped[k]) for k in floats(resumed))
    assert any("running_mean" in k for k in straight)  # BatchNorm running statistics are part of the comparison
    if runs["spread"] == 0:
        for k, v in straight.items():
            assert torch.equal(resumed[k], v), k
        print("resume: bit-identical to the straight run")
    else:
        assert_agree(resumed, straight, runs["spread"], runs["torch_dev"], runs["steps"], "resumed vs straight run")


def test_finetuner_personalise_with_the_native_step(device, lib):
    def logits_of(extra, fused=False):
        args = learner.build_multistep_parser().parse_args(MODEL + ["--personalize_num_grad_steps", "3", "--personalize_weight_decay",
                                                                    "0.2", "--personalize_betas", "0.9", "0.98"] + extra)
        L = learner.MultiStepLearner(args)
        assert L.learning_args()["native_optimizer"] is bool(extra)
        task = L.make_task(0)
        lo, hi = task["target_videos"][0]
        L.model.set_test_mode(True)
        L.model.personalise(task["context_clips"], task["context_labels"].to(L.device), dict(L.learning_args(), fused_optimizer=fused))
        with torch.no_grad():
            out = L.model.predict(attach_frame_history(task["target_clips"][lo:hi, 0], 1)).detach().cpu()
        L.model._reset()
        return out

    first, second, native = logits_of([]), logits_of([]), logits_of(["--native_optimizer"])
    assert torch.isfinite(native).all() and native.shape == first.shape
    spread = ((first - second).abs().max() / first.abs().max()).item()
    torch_dev = ((first - logits_of([], fused=True)).abs().max() / first.abs().max()).item()
    assert_agree({"logits": native}, {"logits": first}, spread, torch_dev, 3, "finetuner logits, native vs torch optimizer, 3 steps")
