"""Throughput of the efficientnet_v2_s extractor (csrc/extractor.hip, build_efficientnet_v2_s): one JSON line.

200 frames of 224 x 224 through the extractor in eval() under no_grad, without FiLM and with the fast `film=` path: the median
ms per 200 frames after warm-up and frames per second; the per-family kernel time of one plain forward from the library's
per-launch event records (orbit_prof_*: dense convolutions by kernel variant, depthwise, squeeze-excite gate, pooling); and the
dense convolutions' and the whole forward's TF/s as fractions of the fp32 MFMA peak bench.py prices the flagship workload on.

    python tools/effnetv2_bench.py [--steps 10] [--warmup 3] [--frames 200] [--size 224]

--train times one CNAPs LITE step instead (SingleStepFewShotRecogniser with adapt_features and the prototype head on the frozen
extractor with native_backward: personalise_with_lite over --way x --context_per_class context frames, predict_a_batch over
--query frames, cross-entropy, backward into the FiLM generator and the set encoder), beside the same calls under
torch.no_grad() - the step's forward-only time - and reports orbit_extractor_tape_bytes per frame at that size.

    python tools/effnetv2_bench.py --train [--steps 5] [--warmup 2] [--way 5] [--context_per_class 40] [--query 200] [--size 224]

--train --learn_extractor times one ProtoNets LITE step with every parameter of the extractor trained instead (the recipe of the
reference's efficientnet_v2_s checkpoints: learn_extractor, no FiLM, native_weight_backward; batch-statistics BatchNorm on the
cache pass, the LITE subset and the query batch; backward into all 450 parameters), and the same step with the squeeze-excite
parameter gradients summed per block (HipNetwork.se_param_grads_per_block) beside it: the A/B of the batched kernel.

Nothing here is gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib, synthetic  # noqa: E402
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor  # noqa: E402

PEAK_TF = 157.3  # bench.py PEAK_FP32_MFMA_TFLOPS (v_mfma_f32_32x32x2_f32, dense)
NAME = "efficientnet_v2_s"


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def _family(variant):
    if variant.startswith("conv_igemm"):
        return "conv:" + variant[len("conv_igemm"):]
    for prefix, key in (("conv_splitk_reduce", "conv:splitk_reduce"), ("pw_rgemm", "conv:pw_rgemm"), ("pw_stream", "conv:pw_stream"),
                        ("dwconv", "depthwise"), ("se_gate", "se_gate"), ("avgpool", "avgpool"), ("bn_fold", "bn_fold")):
        if variant.startswith(prefix):
            return key
    return "other"


def _families(run):
    """{family: ms, flops, launches} of one call of `run` from the per-launch event records."""
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.orbit_prof_enable(1)
    run()
    torch.cuda.synchronize()
    t, f, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
    lib.orbit_prof_collect(ctypes.byref(t), ctypes.byref(f), ctypes.byref(n))
    fam = {}
    for i in range(lib.orbit_prof_num_variants()):
        name = ctypes.create_string_buffer(48)
        launches, ms, flops, nbytes = ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        lib.orbit_prof_variant(i, name, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(flops), ctypes.byref(nbytes))
        d = fam.setdefault(_family(name.value.decode()), {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0})
        d["ms"] += ms.value
        d["flops"] += flops.value
        d["bytes"] += nbytes.value
        d["launches"] += launches.value
    lib.orbit_prof_enable(0)
    return fam


def learn_main(a):
    """One ProtoNets LITE step with the whole extractor trained, batched and per-block squeeze-excite gradients (module docstring)."""
    import numpy as np
    import torch.nn.functional as F
    from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser
    lib = _lib.load()
    model = SingleStepFewShotRecogniser(NAME, False, "proto", 1, 256, True, a.lite_samples, 1.0)
    synthetic.init_parameters_(model)
    fe = model.feature_extractor
    fe.native_weight_backward = True
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(False)
    S = a.size
    task = synthetic.make_task_on_device(0, a.way, 1, a.context_per_class, a.query, S, 1, "cuda:0", template="blobs")
    ctx, lab, tgt, tlab = task["context_clips"], task["context_labels"], task["target_clips"], task["target_labels"]

    def step():
        np.random.seed(7)
        model._clear_caches()
        model.personalise_with_lite(ctx, lab)
        loss = F.cross_entropy(model.predict_a_batch(tgt), tlab)
        loss.backward()
        model._reset()
        model.zero_grad(set_to_none=True)
        return loss

    plan = fe._plan(S, S, trainable=True)
    result = {"metric": "effnetv2_lite_learn_step_ms", "frame_size": S, "way": a.way, "context_frames": len(ctx),
              "query_frames": len(tgt), "lite_samples": a.lite_samples, "parameters_trained": sum(1 for _ in fe.parameters()),
              "tape_bytes_per_frame": lib.orbit_extractor_tape_bytes(plan.handle, 8) // 8,
              "backward_workspace_bytes_per_frame": lib.orbit_extractor_backward_workspace_bytes(plan.handle, 8) // 8}
    for tag, per_block in (("step", False), ("step_se_per_block", True), ("step_again", False)):
        fe.se_param_grads_per_block = per_block
        med, lo, hi = _time(step, a.steps, a.warmup)
        result[tag] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
    fe.se_param_grads_per_block = False
    result["loss"] = round(float(step().detach()), 6)
    result["max_memory_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(result))


def train_main(a):
    """One CNAPs LITE step and its forward-only time (module docstring)."""
    import numpy as np
    import torch.nn.functional as F
    from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser
    lib = _lib.load()
    model = SingleStepFewShotRecogniser(NAME, True, "proto", 1, 256, False, a.lite_samples, 1.0)
    synthetic.init_parameters_(model)
    fe = model.feature_extractor
    fe.native_backward = True
    model._set_device("cuda:0")
    model._send_to_device()
    model.set_test_mode(False)
    S = a.size
    task = synthetic.make_task_on_device(0, a.way, 1, a.context_per_class, a.query, S, 1, "cuda:0", template="blobs")
    ctx, lab, tgt, tlab = task["context_clips"], task["context_labels"], task["target_clips"], task["target_labels"]

    def step():  # one task of Learner.train_task_with_lite (one query batch): set-encoder and feature cache passes included
        np.random.seed(7)
        model._clear_caches()
        model.personalise_with_lite(ctx, lab)
        loss = F.cross_entropy(model.predict_a_batch(tgt), tlab) + 0.001 * model.film_generator.regularization_term()
        if loss.requires_grad:
            loss.backward()
        model._reset()
        model.zero_grad(set_to_none=True)
        return loss

    def forward_only():
        with torch.no_grad():
            step()

    plan = fe._plan(S, S, trainable=True)
    result = {"metric": "effnetv2_lite_step_ms", "frame_size": S, "way": a.way, "context_frames": len(ctx), "query_frames": len(tgt),
              "lite_samples": a.lite_samples,
              "tape_bytes_per_frame": lib.orbit_extractor_tape_bytes(plan.handle, 8) // 8,
              "tape_bytes_1_frame": lib.orbit_extractor_tape_bytes(plan.handle, 1)}
    for tag, fn in (("step", step), ("forward_only", forward_only)):
        med, lo, hi = _time(fn, a.steps, a.warmup)
        result[tag] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
    result["loss"] = round(float(step().detach()), 6)
    result["max_memory_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(result))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--frames", type=int, default=200)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--train", action="store_true", help="time one CNAPs LITE step and its forward-only time instead")
    p.add_argument("--learn_extractor", action="store_true",
                   help="with --train: one ProtoNets LITE step with every parameter trained (native_weight_backward), and its "
                        "A/B with per-block squeeze-excite gradients")
    p.add_argument("--way", type=int, default=5)
    p.add_argument("--context_per_class", type=int, default=40)
    p.add_argument("--query", type=int, default=200)
    p.add_argument("--lite_samples", type=int, default=16)
    a = p.parse_args(argv)
    _lib.require_gpu()
    torch.cuda.set_device(0)
    if a.train:
        return learn_main(a) if a.learn_extractor else train_main(a)
    fe, _ = create_feature_extractor(NAME, with_film=True, learn_extractor=False)
    synthetic.init_parameters_(fe)
    fe.to("cuda:0").eval()
    B, S = a.frames, a.size
    x = torch.randn(B, 3, S, S, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1))
    out = torch.empty(B, fe.output_size, device="cuda:0")
    slots = fe.film_slot_modules()
    gamma = torch.cat([m.weight.detach().reshape(-1) for _, m in slots]) * 1.01
    beta = torch.cat([m.bias.detach().reshape(-1) for _, m in slots]) + 0.01

    def plain():
        with torch.no_grad():
            fe(x, out=out)

    def film():
        with torch.no_grad():
            fe(x, film=(gamma, beta), out=out)

    macs = fe.macs_per_frame(S, S)
    tflop = 2.0 * macs * B / 1e12
    result = {"metric": "effnetv2_ms_per_%d_frames" % B, "frames": B, "frame_size": S, "peak_tflops": PEAK_TF,
              "gmacs_per_frame": round(macs / 1e9, 4), "floor_ms": round(tflop / PEAK_TF * 1e3, 3)}
    for tag, fn in (("plain", plain), ("film", film)):
        med, lo, hi = _time(fn, a.steps, a.warmup)
        result[tag] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                       "frames_per_s": round(B / med * 1e3, 1), "tflops": round(tflop / med * 1e3, 2),
                       "fraction_of_peak": round(tflop / med * 1e3 / PEAK_TF, 3)}
    fam = _families(plain)
    result["families"] = {k: {"ms": round(v["ms"], 3), "launches": v["launches"],
                              "tflops": round(v["flops"] / v["ms"] / 1e9, 2) if v["ms"] else 0.0,
                              "gb_per_s": round(v["bytes"] / v["ms"] / 1e6, 1) if v["ms"] else 0.0}
                          for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])}
    conv_ms = sum(v["ms"] for k, v in fam.items() if k.startswith("conv:"))
    conv_fl = sum(v["flops"] for k, v in fam.items() if k.startswith("conv:"))
    result["launches"] = sum(v["launches"] for v in fam.values())
    result["kernel_ms_total"] = round(sum(v["ms"] for v in fam.values()), 3)
    result["conv_ms"] = round(conv_ms, 3)
    result["conv_tflops"] = round(conv_fl / conv_ms / 1e9, 2) if conv_ms else 0.0
    result["conv_fraction_of_peak"] = round(conv_fl / conv_ms / 1e9 / PEAK_TF, 3) if conv_ms else 0.0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
