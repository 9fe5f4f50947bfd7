"""Milliseconds per optimizer step: optim.NativeAdam (one launch, csrc/optim.hip) against torch.optim.Adam three ways - `default`,
what the learner builds without a flag (`fused=False`, which selects torch's single-tensor loop: ~10 launches per TENSOR),
`foreach` (`foreach=True`, torch's own default on the GPU: ~10 launches per group) and `fused` (`fused=True`,
--fused_optimizer) - on the parameter lists of the efficientnet_b0 CNAPs model
(--adapt_features --learn_extractor --classifier versa) and of vit_b_32. One JSON line.

    python tools/optim_bench.py [--steps 50] [--warmup 10] [--rounds 3]

Only the shapes of the parameters are taken from the models: the tensors are plain fp32 device tensors, so no native plan is
built. A step is what the learner's loop does around it: every parameter gets a gradient tensor (the pointers alternate between
two sets with --moving_grads, which makes the native step re-upload its table every time), then optimizer.step() and
optimizer.zero_grad(set_to_none=True). Two times per optimizer: `wall_ms`, a host clock around steps that end in a device
synchronise (host time + kernel time of ONE step, what a loop that synchronises per task pays), and `stream_ms`, device events
around the whole window of steps divided by their number (the rate at which a queue of steps drains). The four optimizers are
timed alternately, `rounds` times; the figures are medians over the rounds' medians. GB/s is 28 bytes per element (p, g, m, v
read; p, m, v written) over stream_ms. Nothing here is gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from orbit_dataset_amd.optim import NativeAdam  # noqa: E402


def shapes_of(name):
    """[(shape, group)] in the optimizer's order: everything but the extractor, then the extractor (optim.init_optimizer)"""
    from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser
    if name == "efficientnet_b0_cnaps":
        model = SingleStepFewShotRecogniser("efficientnet_b0", True, "versa", 1, 256, True, 16, 1.0)
    else:
        model = SingleStepFewShotRecogniser(name, False, "proto", 1, 256, True, 16, 1.0)
    extractor = set(map(id, model.feature_extractor.parameters()))
    rest = [(tuple(p.shape), 0) for p in model.parameters() if id(p) not in extractor]
    return rest + [(tuple(p.shape), 1) for p in model.feature_extractor.parameters()]


def make(kind, shapes, device):
    g = torch.Generator(device=device).manual_seed(1)
    params = [torch.randn(s, device=device, generator=g) * 0.05 for s, _ in shapes]
    grads = [[torch.randn(s, device=device, generator=g) * 1e-3 for s, _ in shapes] for _ in range(2)]
    groups = [{"params": [p for p, (_, k) in zip(params, shapes) if k == gi]} for gi in (0, 1)]
    groups = [g_ for g_ in groups if g_["params"]]
    kw = dict(lr=5e-6, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)
    if kind == "native":
        opt = NativeAdam(groups, **kw)
    elif kind == "default":
        opt = torch.optim.Adam(groups, fused=False, **kw)  # optim.init_optimizer without a flag
    else:
        opt = torch.optim.Adam(groups, foreach=(kind == "foreach") or None, fused=(kind == "fused") or None, **kw)
    return opt, params, grads


def one_step(opt, params, grads):
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()
    opt.zero_grad(set_to_none=True)


def measure(opt, params, grads, steps, warmup, moving):
    pick = (lambda i: grads[i % 2]) if moving else (lambda i: grads[0])
    for i in range(warmup):
        one_step(opt, params, pick(i))
    torch.cuda.synchronize()
    wall = []
    for i in range(steps):
        t0 = time.perf_counter()
        one_step(opt, params, pick(i))
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        one_step(opt, params, pick(i))
    b.record()
    b.synchronize()
    return statistics.median(wall), a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", default="efficientnet_b0_cnaps,vit_b_32")
    ap.add_argument("--moving_grads", action="store_true")
    a = ap.parse_args()
    _lib.require_gpu()
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "moving_grads": a.moving_grads, "models": {}}
    for name in a.models.split(","):
        shapes = shapes_of(name)
        n = sum(int(torch.Size(s).numel()) for s, _ in shapes)
        kinds = ("default", "foreach", "fused", "native")
        built = {k: make(k, shapes, device) for k in kinds}
        samples = {k: [] for k in kinds}
        for _ in range(a.rounds):  # alternating: other work shares the host
            for k in kinds:
                samples[k].append(measure(*built[k], a.steps, a.warmup, a.moving_grads))
        row = {"tensors": len(shapes), "elements": n, "mbytes_per_step": 28.0 * n / 1e6}
        for k in kinds:
            wall = statistics.median(s[0] for s in samples[k])
            stream = statistics.median(s[1] for s in samples[k])
            row[k] = {"wall_ms": round(wall, 4), "stream_ms": round(stream, 4), "gb_per_s": round(28.0 * n / stream / 1e6, 1),
                      "wall_ms_rounds": [round(s[0], 4) for s in samples[k]]}
        # the three must have computed the same thing
        ref = built["foreach"][1]
        for k in ("default", "fused", "native"):
            row[k]["max_rel_diff_vs_foreach"] = max(
                ((p - q).abs().max() / q.abs().max().clamp_min(1e-30)).item() for p, q in zip(built[k][1], ref))
        out["models"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
