"""Throughput of the transformer extractors (csrc/vit.hip) on config-3-shaped tasks: one JSON line.

For each of vit_s_32 / vit_b_32 / vit_b_32_clip (or, with --models, the patch-16 vit_s_16 / vit_b_16 / vit_b_16_clip): a 5-way task with 200 support and 200 query frames at 224 x 224, run
personalise() + predict() in test mode with ProtoNets (`proto`) and with CNAPs (`versa` + FiLM adaptation); the median ms per
task after warm-up, query frames/s, per-family kernel time of one proto task from the library's per-launch event records
(token GEMM, attention, LayerNorm, patch embedding), the token GEMMs' TF/s as a fraction of the 155 TF fp32 MFMA peak, and
torch.nn.functional.linear (fp32, the vendor BLAS) on the same four shapes at M = 10 000 token rows as a reference point.

    python tools/vit_bench.py [--steps 10] [--warmup 3] [--models vit_s_32,vit_b_32,vit_b_32_clip]
    python tools/vit_bench.py --models vit_s_16,vit_b_16,vit_b_16_clip

--train reports the training side instead, for any of the six models: ms of taped forward + orbit_vit_backward_params (every
parameter's gradient, through the module with its weight-gradient opt-in: native_weight_backward, or
native_weight_backward_patch16 for the patch-16 models) at the step shapes B = 16 and B = 200 - median, minimum and maximum over
--steps repetitions after --warmup - the profiler's weight-gradient rows of one such step per layer (launches, ms and TF/s of
the split-reduction launches at the step's own row count, the patch-embedding filter gradient among them), the weight-gradient
GEMM family's TF/s per layer shape at M = 10 000 token rows (orbit_op_vit_linear_wgrad, split-reduction launch + reduce), and
fp32 `dy.t() @ x` through torch (the vendor BLAS) on the same shapes. Nothing here is gated.

    python tools/vit_bench.py --train --models vit_s_16,vit_b_16,vit_b_16_clip

--train_film reports the FiLM-gradient step of the frozen network, for any of the six models: ms of taped forward +
orbit_vit_backward (through the module with its FiLM opt-in: native_backward, or native_backward_patch16 for the patch-16
models) at a LITE-sized batch of 16 frames, and the profiler's per-kernel rows of one such step - launches, ms and share of
the step's kernel time - with the attention backward's time relative to the attention forward's on the same batch.

    python tools/vit_bench.py --train_film --models vit_s_16,vit_b_16,vit_b_16_clip

--precision bf16 runs the same inference report on the opt-in bf16 plan (VisionTransformer.bf16_inference: qkv / proj / fc1 / fc2
on v_mfma_f32_32x32x16_bf16, everything else fp32); the token GEMMs' TF/s are then a fraction of the 2 500 TF dense bf16 peak.
--compare_precision runs one resident task on both plans of one model and prints the largest feature difference, the largest
logit difference and the argmax agreement. --gemm_shapes times the bf16 and the fp32 token GEMM on the eight ViT-S / ViT-B layer
shapes at M = 39 400 rows (200 frames of 197 tokens) from the per-launch event records.

    python tools/vit_bench.py --precision bf16 --models vit_s_32,vit_b_32,vit_b_32_clip,vit_s_16,vit_b_16,vit_b_16_clip
    python tools/vit_bench.py --compare_precision --models vit_s_32,vit_b_16
    python tools/vit_bench.py --gemm_shapes

--frame_size S runs the inference report on S x S frames (square, a multiple of the patch size, 32..512): it sets
VisionTransformer.resample_pos_embed when S is not 224, so the plans come from orbit_vit_create_sized and the position table is
resampled to the S / patch grid; with --precision bf16 as well.

    python tools/vit_bench.py --frame_size 96 --models vit_b_32_clip
    python tools/vit_bench.py --frame_size 384 --models vit_b_16_clip --precision bf16
"""
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
from orbit_dataset_amd.model.few_shot_recognisers import SingleStepFewShotRecogniser  # noqa: E402

PEAK_TF = 155.0  # fp32 MFMA, measured (v_mfma_f32_32x32x2_f32)
PEAK_TF_BF16 = 2500.0  # dense bf16 MFMA (v_mfma_f32_32x32x16_bf16), the specification's figure


def _samples(fn, steps, warmup):
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
    return ms


def _time(fn, steps, warmup):
    return statistics.median(_samples(fn, steps, warmup))


def _model(name, adapt, classifier, bf16=False, frame_size=224):
    m = SingleStepFewShotRecogniser(name, adapt, classifier, 1, 200, False, 16, 1.0)
    synthetic.init_parameters_(m)
    m.feature_extractor.bf16_inference = bool(bf16)
    m.feature_extractor.resample_pos_embed = frame_size != 224  # (other sizes: the opt-in resampled position table)
    m._set_device("cuda:0")
    m._send_to_device()
    m.set_test_mode(True)
    return m


def _task_fn(model, task):
    def run():
        with torch.no_grad():
            model.personalise(task["context_clips"], task["context_labels"])
            model.predict(task["target_clips"])
            model._reset()
    return run


def _families(run):
    """per-family kernel ms and flops of one call of `run` from orbit_prof_* records"""
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
        v = name.value.decode()
        if not v.startswith("vit_"):
            key = "other"
        elif v.startswith(("vit_qkv", "vit_proj", "vit_fc1", "vit_fc2")):
            key = "gemm"
        elif v.startswith(("vit_patch_embed", "vit_cls_token")):
            key = "patch"
        else:
            key = v[4:]
        d = fam.setdefault(key, {"ms": 0.0, "flops": 0.0, "launches": 0})
        d["ms"] += ms.value
        d["flops"] += flops.value
        d["launches"] += launches.value
    lib.orbit_prof_enable(0)
    return fam


def _torch_linear(D, steps, warmup, M=10000):
    torch.backends.cuda.matmul.allow_tf32 = False
    out = {}
    for tag, K, N in (("qkv", D, 3 * D), ("proj", D, D), ("fc1", D, 4 * D), ("fc2", 4 * D, D)):
        x = torch.randn(M, K, device="cuda:0")
        w = torch.randn(N, K, device="cuda:0") / K ** 0.5
        b = torch.randn(N, device="cuda:0")
        ms = _time(lambda: torch.nn.functional.linear(x, w, b), steps, warmup)
        out[tag] = {"ms": round(ms, 4), "tflops": round(2.0 * M * N * K / ms / 1e9, 2)}
    return out


def _spread(fn, steps, warmup):
    """as _time, with the spread: {median, min, max} ms over `steps` repetitions"""
    ms = _samples(fn, steps, warmup)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def _wgrad_rows(run):
    """the profiler's weight-gradient rows of one call of `run`, per layer: launches, ms and TF/s (the split launches' own
    flops; the reduce launches are listed apart)"""
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.orbit_prof_enable(1)
    run()
    torch.cuda.synchronize()
    lib.orbit_prof_collect(None, None, None)
    out = {}
    for i in range(lib.orbit_prof_num_variants()):
        name = ctypes.create_string_buffer(48)
        launches, ms, flops = ctypes.c_long(), ctypes.c_double(), ctypes.c_double()
        lib.orbit_prof_variant(i, name, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(flops), None)
        v = name.value.decode()
        if launches.value and v.startswith("vit_wgrad_"):
            out[v[len("vit_wgrad_"):]] = {"launches": launches.value, "ms": round(ms.value, 4),
                                          "tflops": round(flops.value / ms.value / 1e9, 2) if ms.value else 0.0}
    lib.orbit_prof_enable(0)
    return out


def _train_step(name, B, steps, warmup):
    from orbit_dataset_amd.model.feature_extractors import create_feature_extractor
    fe, _ = create_feature_extractor(name, with_film=False, learn_extractor=True)
    synthetic.init_parameters_(fe)
    fe.to("cuda:0")
    fe.native_weight_backward = fe.native_weight_backward_patch16 = True  # (each is ignored by the other patch size)
    x = torch.randn(B, 3, 224, 224, device="cuda:0")
    r = torch.randn(B, fe.output_size, device="cuda:0")

    def step():
        for p in fe.parameters():
            p.grad = None
        (fe(x) * r).sum().backward()
    return _spread(step, steps, warmup), _wgrad_rows(step)


def _wgrad_shapes(D, steps, warmup, M=10000):
    """per layer shape: the native wgrad (launch + reduce) and torch's dy.t() @ x, both fp32, ms and TF/s"""
    lib = _lib.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    out = {}
    for tag, N, K, gelu in (("qkv", 3 * D, D, 0), ("proj", D, D, 0), ("fc1", 4 * D, D, 0), ("fc2", D, 4 * D, 1)):
        dy = torch.randn(M, N, device="cuda:0")
        x = torch.randn(M, K, device="cuda:0")
        dw, db = torch.empty(N, K, device="cuda:0"), torch.empty(N, device="cuda:0")
        need = lib.orbit_op_vit_linear_wgrad_workspace_floats(M, N, K)
        ws = torch.empty(max(need, 64), device="cuda:0")

        def native():
            _lib.check(lib.orbit_op_vit_linear_wgrad(_lib.dptr(dy), _lib.dptr(x), _lib.dptr(dw), _lib.dptr(db), M, N, K, gelu,
                                                     _lib.dptr(ws), need, _lib.stream_handle()), "orbit_op_vit_linear_wgrad")
        ms = _time(native, steps, warmup)
        ms_t = _time(lambda: torch.matmul(dy.t(), x), steps, warmup)
        tf = lambda t: round(2.0 * M * N * K / t / 1e9, 2)
        out[tag] = {"N": N, "K": K, "gelu_on_x": gelu, "wgrad_ms": round(ms, 4), "wgrad_tflops": tf(ms),
                    "torch_ms": round(ms_t, 4), "torch_tflops": tf(ms_t)}
    return out


def main_train(a):
    result = {"metric": "vit_train_ms", "what": "taped forward + orbit_vit_backward_params, every parameter trainable",
              "peak_tflops": PEAK_TF, "models": {}}
    for name in a.models.split(","):
        r = {"fwd_bwd_ms": {}, "fwd_bwd_ms_spread": {}, "wgrad_rows_of_a_step": {}}
        for B in (16, 200):
            ms, rows = _train_step(name, B, a.steps, a.warmup)
            r["fwd_bwd_ms"]["B%d" % B] = ms["median"]
            r["fwd_bwd_ms_spread"]["B%d" % B] = ms
            r["wgrad_rows_of_a_step"]["B%d" % B] = rows
            torch.cuda.empty_cache()
        r["wgrad_m10000"] = _wgrad_shapes(384 if name.startswith("vit_s_") else 768, a.steps, a.warmup)
        result["models"][name] = r
        torch.cuda.empty_cache()
    print(json.dumps(result))


FILM_BATCH = 16  # frames with a gradient per LITE step (learner --num_lite_samples 16)


def _kernel_rows(run):
    """{profiler row: (launches, ms)} of one call of `run`"""
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.orbit_prof_enable(1)
    run()
    torch.cuda.synchronize()
    lib.orbit_prof_collect(None, None, None)
    rows = {}
    for i in range(lib.orbit_prof_num_variants()):
        name = ctypes.create_string_buffer(48)
        launches, ms = ctypes.c_long(), ctypes.c_double()
        lib.orbit_prof_variant(i, name, ctypes.byref(launches), ctypes.byref(ms), None, None)
        if launches.value:
            rows[name.value.decode()] = (launches.value, ms.value)
    lib.orbit_prof_enable(0)
    return rows


def main_train_film(a):
    from orbit_dataset_amd.model.feature_extractors import create_feature_extractor
    B = FILM_BATCH
    result = {"metric": "vit_train_film_ms", "what": "taped forward + orbit_vit_backward, frozen network, FiLM vectors trainable",
              "batch_frames": B, "models": {}}
    for name in a.models.split(","):
        fe, _ = create_feature_extractor(name, with_film=True, learn_extractor=False)
        synthetic.init_parameters_(fe)
        fe.eval().to("cuda:0")
        fe.native_backward = fe.native_backward_patch16 = True  # (each is ignored by the other patch size)
        x = torch.randn(B, 3, 224, 224, device="cuda:0")
        r = torch.randn(B, fe.output_size, device="cuda:0")
        gamma = torch.ones(fe.film_size, device="cuda:0", requires_grad=True)
        beta = torch.zeros(fe.film_size, device="cuda:0", requires_grad=True)

        def step():
            gamma.grad = beta.grad = None
            (fe(x, film=(gamma, beta)) * r).sum().backward()
        ms = _time(step, a.steps, a.warmup)
        rows = _kernel_rows(step)
        total = sum(t for _, t in rows.values())
        out = {"fwd_bwd_ms": round(ms, 3), "kernel_ms_total": round(total, 3),
               "kernels": {k: {"launches": n, "ms": round(t, 4), "share": round(t / total, 4)}
                           for k, (n, t) in sorted(rows.items(), key=lambda kv: -kv[1][1])}}
        fwd = [k for k in rows if k in ("vit_attention", "vit_attention197")]
        bwd = [k for k in rows if k in ("vit_attention_bwd", "vit_attention197_bwd")]
        if fwd and bwd:
            per = lambda k: rows[k][1] / rows[k][0]
            out["attention_bwd_share_of_step"] = round(rows[bwd[0]][1] / total, 4)
            out["attention_bwd_over_fwd"] = round(per(bwd[0]) / per(fwd[0]), 2)
        result["models"][name] = out
        del fe
        torch.cuda.empty_cache()
    print(json.dumps(result))


def main_compare_precision(a):
    """one resident task through the fp32 plan and the bf16 plan of the same module (same parameters): features of all 400 frames,
    logits of the 200 query frames"""
    result = {"metric": "vit_bf16_vs_fp32", "task": "5-way, 200 support + 200 query frames, 224x224, proto head", "models": {}}
    for name in a.models.split(","):
        task = synthetic.make_task_on_device(0, 5, 5, 8, 200, 224, 1, "cuda:0")
        model = _model(name, False, "proto")
        fe = model.feature_extractor
        frames = torch.cat((task["context_clips"].flatten(end_dim=1), task["target_clips"].flatten(end_dim=1)))
        out = {}
        for precision in ("fp32", "bf16"):
            fe.bf16_inference = precision == "bf16"
            with torch.no_grad():
                feats = torch.cat([fe(frames[i:i + 200]) for i in range(0, frames.shape[0], 200)])
                model.personalise(task["context_clips"], task["context_labels"])
                logits = model.predict(task["target_clips"]).clone()
                model._reset()
            out[precision] = (feats, logits)
        (f32, l32), (f16, l16) = out["fp32"], out["bf16"]
        result["models"][name] = {
            "max_abs_feature": round(f32.abs().max().item(), 4), "max_abs_feature_diff": round((f16 - f32).abs().max().item(), 5),
            "max_abs_logit": round(l32.abs().max().item(), 3), "max_abs_logit_diff": round((l16 - l32).abs().max().item(), 4),
            "argmax_agreement": round((l16.argmax(1) == l32.argmax(1)).float().mean().item(), 4), "query_frames": l32.shape[0]}
        del model, fe
        torch.cuda.empty_cache()
    print(json.dumps(result))


GEMM_M = 39400  # 200 frames of 197 tokens


def main_gemm_shapes(a):
    """orbit_op_vit_linear and orbit_op_vit_linear_bf16 (tile rule of the forward) on the eight layer shapes: mean ms per launch of
    --steps launches after --warmup, from the per-launch event records"""
    lib = _lib.load()
    M = GEMM_M
    result = {"metric": "vit_gemm_bf16_vs_fp32", "M": M, "peak_tflops": {"fp32": PEAK_TF, "bf16": PEAK_TF_BF16}, "shapes": {}}
    for D in (384, 768):
        for tag, K, N, epi in (("qkv", D, 3 * D, 0), ("proj", D, D, 2), ("fc1", D, 4 * D, 1), ("fc2", 4 * D, D, 2)):
            x = torch.randn(M, K, device="cuda:0")
            w = torch.randn(N, K, device="cuda:0") / K ** 0.5
            b = torch.randn(N, device="cuda:0")
            res = torch.randn(M, N, device="cuda:0") if epi == 2 else None
            y = torch.empty(M, N, device="cuda:0")
            wb = torch.empty(N, K, dtype=torch.int16, device="cuda:0")
            _lib.check(lib.orbit_op_vit_pack_bf16(_lib.dptr(w), ctypes.c_void_p(wb.data_ptr()), w.numel(), _lib.stream_handle()),
                       "orbit_op_vit_pack_bf16")

            def fp32():
                _lib.check(lib.orbit_op_vit_linear(_lib.dptr(x), _lib.dptr(w), _lib.dptr(b), _lib.dptr(res), _lib.dptr(y), M, N, K,
                                                   epi, 0, _lib.stream_handle()), "orbit_op_vit_linear")

            def bf16():
                _lib.check(lib.orbit_op_vit_linear_bf16(_lib.dptr(x), ctypes.c_void_p(wb.data_ptr()), _lib.dptr(b), _lib.dptr(res),
                                                        _lib.dptr(y), M, N, K, epi, 0, _lib.stream_handle()),
                           "orbit_op_vit_linear_bf16")
            r = {"K": K, "N": N}
            for what, fn in (("fp32", fp32), ("bf16", bf16)):
                for _ in range(a.warmup):
                    fn()

                def many():
                    for _ in range(a.steps):
                        fn()
                rows = {k: v for k, v in _kernel_rows(many).items() if k.startswith("vit_op_linear")}
                (row, (launches, ms)), = rows.items()
                r[what] = {"row": row, "ms": round(ms / launches, 4), "tflops": round(2.0 * M * N * K / (ms / launches) / 1e9, 1)}
            r["speedup"] = round(r["fp32"]["ms"] / r["bf16"]["ms"], 2)
            result["shapes"]["%s_D%d" % (tag, D)] = r
    print(json.dumps(result))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--models", default="vit_s_32,vit_b_32,vit_b_32_clip",
                   help="comma-separated, any of the six transformer extractors")
    p.add_argument("--train", action="store_true", help="the training step and the weight-gradient GEMMs instead")
    p.add_argument("--train_film", action="store_true",
                   help="the FiLM-gradient step of the frozen network at a batch of %d frames instead (all six models)" % FILM_BATCH)
    p.add_argument("--precision", choices=("fp32", "bf16"), default="fp32",
                   help="the inference report on the fp32 plan (default) or on the opt-in bf16 plan")
    p.add_argument("--frame_size", type=int, default=224,
                   help="the inference report at another frame size (a multiple of the patch size in 32..512): sets "
                        "VisionTransformer.resample_pos_embed when it is not 224")
    p.add_argument("--compare_precision", action="store_true",
                   help="one resident task on both plans of each model: feature / logit differences and argmax agreement instead")
    p.add_argument("--gemm_shapes", action="store_true",
                   help="the bf16 and the fp32 token GEMM on the eight layer shapes at M = %d instead" % GEMM_M)
    a = p.parse_args(argv)
    _lib.require_gpu()
    torch.cuda.set_device(0)
    if a.compare_precision:
        return main_compare_precision(a)
    if a.gemm_shapes:
        return main_gemm_shapes(a)
    if a.train_film:
        return main_train_film(a)
    if a.train:
        return main_train(a)
    bf16 = a.precision == "bf16"
    peak = PEAK_TF_BF16 if bf16 else PEAK_TF  # of the token GEMMs; the floor below stays the fp32 one (what the default path can reach)
    S = a.frame_size
    result = {"metric": "vit_task_ms", "task": "5-way, 200 support + 200 query frames, %dx%d" % (S, S), "precision": a.precision,
              "frame_size": S, "peak_tflops": peak, "models": {}}
    for name in a.models.split(","):
        task = synthetic.make_task_on_device(0, 5, 5, 8, 200, S, 1, "cuda:0")
        r = {}
        proto = _model(name, False, "proto", bf16, S)
        run = _task_fn(proto, task)
        r["proto_ms"] = round(_time(run, a.steps, a.warmup), 3)
        r["query_frames_per_s"] = round(200.0 / (r["proto_ms"] / 2) * 1e3, 1)  # (support and query passes are the same size)
        fam = _families(run)
        r["kernel_ms"] = {k: round(v["ms"], 3) for k, v in sorted(fam.items())}
        g = fam.get("gemm", {"ms": 0.0, "flops": 0.0})
        tf = g["flops"] / g["ms"] / 1e9 if g["ms"] else 0.0
        r["gemm_tflops"] = round(tf, 2)
        r["gemm_fraction_of_peak"] = round(tf / peak, 3)
        macs = proto.feature_extractor.macs_per_frame(S, S)
        r["task_tflop"] = round(2 * macs * 400 / 1e12, 3)
        r["task_floor_ms"] = round(2 * macs * 400 / (PEAK_TF * 1e12) * 1e3, 2)
        del proto
        cnaps = _model(name, True, "versa", bf16, S)
        r["cnaps_ms"] = round(_time(_task_fn(cnaps, task), a.steps, a.warmup), 3)
        del cnaps
        r["torch_linear_m10000"] = _torch_linear(384 if name.startswith("vit_s_") else 768, a.steps, a.warmup)
        result["models"][name] = r
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
