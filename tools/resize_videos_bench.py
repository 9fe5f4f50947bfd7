"""tools/resize_videos.py end to end against the reference pipeline (PIL open -> convert -> resize LANCZOS -> save(quality=95)
on host threads, scripts/resize_videos.py) on a synthetic tree of 1080 x 1080 frames: frames/s of both, and - from a second,
profiled run - how the device time splits over the decoder's, the resize's and the encoder's kernels. Every output file is
compared with the reference pipeline's bytes.
Usage (GPU box): python tools/resize_videos_bench.py [--frames 400] [--source 1080] [--size 224] [--runs 2] [--json OUT]"""
import argparse
import ctypes
import glob
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from PIL import Image

import orbit_dataset_amd  # noqa
from orbit_dataset_amd import _lib
from orbit_dataset_amd.data import pipeline
from orbit_dataset_amd.data.encode import resize_tree


def reference_one(job):
    src, dst, size = job
    im = Image.open(src)
    if im.mode != "RGB":
        im = im.convert("RGB")
    if dst is None:
        buf = io.BytesIO()
        im.resize((size, size), resample=Image.LANCZOS).save(buf, format="JPEG", quality=95)
        return buf.getvalue()
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    im.resize((size, size), resample=Image.LANCZOS).save(dst, quality=95)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=400)
    p.add_argument("--source", type=int, default=1080)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--runs", type=int, default=2)
    p.add_argument("--batch", type=int, default=100)
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    _lib.require_gpu()
    lib = _lib.load()
    per_video = max(1, a.frames // 8)
    result = {"device": torch.cuda.get_device_name(0), "pil": Image.__version__, "source": a.source, "size": a.size}
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, "raw")
        n = pipeline.write_synthetic_orbit_directory(raw, users=1, objects_per_user=2, clean_videos=3, clutter_videos=1,
                                                     frames_per_video=per_video, frame_size=a.source)
        files = sorted(glob.glob(os.path.join(raw, "*", "*", "*", "*", "*.jpg")))
        result.update({"frames": n, "source_bytes": sum(os.path.getsize(f) for f in files)})
        for threads in (12, 16):
            secs = []
            for r in range(a.runs):
                out = os.path.join(tmp, "ref%d_%d" % (threads, r))
                t0 = time.perf_counter()
                with ThreadPoolExecutor(max_workers=threads) as pool:
                    list(pool.map(reference_one, [(f, os.path.join(out, os.path.relpath(f, raw)), a.size) for f in files]))
                secs.append(time.perf_counter() - t0)
            result["reference_%d_threads_s" % threads] = secs
            print("reference pipeline, %2d threads: %s s -> %.1f frames/s (best)" % (threads, ["%.2f" % s for s in secs], n / min(secs)), flush=True)
        secs = []
        for r in range(a.runs + 1):  # the first run pays for the resize tables and the allocator
            out = os.path.join(tmp, "dev%d" % r)
            secs.append(resize_tree(raw, out, size=a.size, nthreads=12, batch=a.batch)["seconds"])
        result["device_s"] = secs
        print("tools/resize_videos.py, 12 threads: %s s -> %.1f frames/s (best; first run is the warm-up)"
              % (["%.2f" % s for s in secs], n / min(secs[1:])), flush=True)
        lib.orbit_prof_enable(1)
        stats = resize_tree(raw, os.path.join(tmp, "prof"), size=a.size, nthreads=12, batch=a.batch)
        torch.cuda.synchronize()
        lib.orbit_prof_enable(0)
        ms, launches = ctypes.c_double(), ctypes.c_long()
        lib.orbit_prof_collect(ctypes.byref(ms), None, ctypes.byref(launches))
        kernels = {}
        for i in range(lib.orbit_prof_num_variants()):
            name, count, kms = ctypes.create_string_buffer(48), ctypes.c_long(), ctypes.c_double()
            lib.orbit_prof_variant(i, name, ctypes.byref(count), ctypes.byref(kms), None, None)
            kernels[name.value.decode()] = {"ms": kms.value, "launches": count.value}
        result.update({"profiled_run_s": stats["seconds"], "kernel_ms_total": ms.value, "kernels": kernels, "host_decoded": stats["host_decoded"]})
        print("profiled run: %.2f s wall, %.1f ms on the device:" % (stats["seconds"], ms.value))
        for k, v in sorted(kernels.items(), key=lambda kv: -kv[1]["ms"]):
            print("    %-26s %9.2f ms  %5.1f %%  (%d launches)" % (k, v["ms"], 100 * v["ms"] / ms.value, v["launches"]), flush=True)
        with ThreadPoolExecutor(max_workers=16) as pool:
            want = list(pool.map(reference_one, [(f, None, a.size) for f in files]))
        exact = all(open(os.path.join(tmp, "prof", os.path.relpath(f, raw)), "rb").read() == w for f, w in zip(files, want))
        result["all_files_equal_reference"] = exact
        print("output files %s the reference pipeline's" % ("==" if exact else "!="))
        assert exact
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
