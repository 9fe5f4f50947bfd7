"""orbit_frames_resize_from_uint8 (csrc/ingest.hip: Pillow's 8-bit resize + to_tensor + normalize in one launch) on the two
resizes a user of the ORBIT tree runs - the raw 1080 x 1080 frames to 224, and a 224 tree to 84 - for all three filters, 200
frames per launch: us per launch and GB/s over the profiler's bytes (8-bit frames in, fp32 frames out), the byte floor at the
6.3 TB/s DESIGN.md prices HBM at, and beside them the time PIL's Image.resize takes for the same frames on 16 threads - the
offline pass of the reference (scripts/resize_videos.py:46) this replaces. The first frame of every case is compared with PIL.
--decode measures the JPEG decoder instead (orbit_frames_from_jpeg, csrc/jpeg.hip) on 224 x 224 and 1080 x 1080 frames written
by write_synthetic_orbit_directory: us per launch of each of its three kernels, the bytes uploaded compressed against decoded,
and PIL's decode of the same files on 16 threads; every frame is compared with PIL. --restart_rows N re-saves the frames with a
restart marker every N MCU rows first: those the entropy kernel decodes with one lane per restart interval. --content noise
replaces the frames by uniform noise; --sub_sweep S .. measures the entropy stage alone at these subsequence sizes.
--encode measures the JPEG encoder (orbit_frames_to_jpeg, csrc/jpeg_enc.hip) on 224 x 224 frames - the size tools/resize_videos.py
writes - of smooth and of noise content at quality 95: us per call of each of its kernels beside the kernel's byte floor (its
algorithmic bytes at 6.3 TB/s), the compressed bytes out, and PIL's save(quality=95) of the same frames on 16 threads; every
file is compared with PIL's.
Usage (GPU box): python tools/ingest_bench.py [--decode [--restart_rows N] [--content noise] [--sub_sweep S ..] | --encode] [--frames 200] [--reps 10] [--threads 16]"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

import orbit_dataset_amd  # noqa
from orbit_dataset_amd import _lib
from orbit_dataset_amd.data.utils import NORMALIZE_STATS, frames_from_uint8

HBM_BYTES_PER_S = 6.3e12
PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def measure(lib, run, reps):
    """(us per launch, profiler bytes per launch, kernel name) from the library's per-launch event records"""
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    lib.orbit_prof_enable(1)
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    lib.orbit_prof_enable(0)
    ms, n = ctypes.c_double(), ctypes.c_long()
    lib.orbit_prof_collect(ctypes.byref(ms), None, ctypes.byref(n))
    assert n.value == reps and lib.orbit_prof_num_variants() == 1, (n.value, lib.orbit_prof_num_variants())
    name, nbytes = ctypes.create_string_buffer(48), ctypes.c_double()
    lib.orbit_prof_variant(0, name, None, None, None, ctypes.byref(nbytes))
    return 1e3 * ms.value / reps, nbytes.value / reps, name.value.decode()


def _rewrite_frames(a, paths, size):
    """--content noise: the frames replaced by uniform noise, the least compressible content; --restart_rows N: re-saved with a
    restart marker every N MCU rows. Both at the quality the frames were written at."""
    if a.content != "noise" and a.restart_rows <= 0:
        return
    rng = np.random.default_rng(0)
    kw = {"restart_marker_rows": a.restart_rows} if a.restart_rows > 0 else {}
    for path in paths:
        img = Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)) if a.content == "noise" else Image.open(path)
        img.save(path, quality=90, **kw)


def measure_sub_sweep(a, lib, dev, pool):
    """the entropy stage alone, per frame size: orbit_op_jpeg_entropy form 0 (serial) and form 1, then orbit_op_jpeg_entropy_sub
    at every sub_bytes of --sub_sweep (0 = the production rule) - us per call between two events, the forms taken, the rounds
    per frame - each compared with form 0's coefficients"""
    import glob
    import tempfile
    from orbit_dataset_amd.data import pipeline
    rows = []
    for size in a.sizes:
        with tempfile.TemporaryDirectory() as root:
            pipeline.write_synthetic_orbit_directory(root, users=1, objects_per_user=1, clean_videos=1, clutter_videos=0,
                                                     frames_per_video=a.frames, frame_size=size)
            paths = sorted(glob.glob(os.path.join(root, "*", "*", "*", "*", "*.jpg")))
            _rewrite_frames(a, paths, size)
            jf = pipeline.read_jpeg_frames(paths, pool)
        n, dsize = len(jf.files), ctypes.sizeof(_lib.JpegDesc)
        descs = np.ascontiguousarray(jf.descs).reshape(n, dsize).copy()
        descs.view(np.uint64)[:, 0] = np.cumsum([0] + [len(f) for f in jf.files[:-1]])
        arena = torch.from_numpy(np.frombuffer(b"".join(jf.files), dtype=np.uint8).copy()).to(dev)
        d_descs = torch.from_numpy(descs.reshape(-1)).to(dev)
        cap = 3 * (2 * ((size + 15) // 16)) ** 2
        coef = torch.zeros((n, cap, 64), dtype=torch.int16, device=dev)
        status, taken, rounds = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        args = (_lib.dptr(arena), arena.numel(), _lib.dptr(d_descs), n, size, size)
        tail = (_lib.dptr(coef, torch.int16), coef.numel() * 2, _lib.dptr(status), _lib.dptr(taken))

        def timed(call):
            for _ in range(2):
                call()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
            ev[0].record()
            for i in range(a.reps):
                call()
                ev[i + 1].record()
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any(), "a frame was not decoded"
            us = sorted(1e3 * ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps))
            return us[0], us[len(us) // 2]

        ecs = [len(f) for f in jf.files]
        best, med = timed(lambda: _lib.check(lib.orbit_op_jpeg_entropy(*args, 0, *tail, _lib.stream_handle()), "orbit_op_jpeg_entropy"))
        want = coef.clone()
        rows.append({"size": size, "content": a.content, "restart_rows": a.restart_rows, "what": "form 0", "us_min": best, "us_median": med,
                     "mean_file_bytes": float(np.mean(ecs))})
        best, med = timed(lambda: _lib.check(lib.orbit_op_jpeg_entropy(*args, 1, *tail, _lib.stream_handle()), "orbit_op_jpeg_entropy"))
        rows.append({"size": size, "content": a.content, "restart_rows": a.restart_rows, "what": "form 1", "us_min": best, "us_median": med})
        for sub_bytes in a.sub_sweep:
            best, med = timed(lambda: _lib.check(lib.orbit_op_jpeg_entropy_sub(*args, sub_bytes, *tail, _lib.dptr(rounds), _lib.stream_handle()),
                                                 "orbit_op_jpeg_entropy_sub"))
            t, r = taken.cpu().numpy(), rounds.cpu().numpy()
            rows.append({"size": size, "content": a.content, "restart_rows": a.restart_rows, "what": "sub_bytes %d" % sub_bytes, "us_min": best,
                         "us_median": med, "taken": {int(k): int((t == k).sum()) for k in np.unique(t)},
                         "rounds_mean": float(r[t == 3].mean()) if (t == 3).any() else 0.0, "rounds_max": int(r.max()),
                         "equals_form_0": bool(torch.equal(coef, want))})
        for row in rows[-(2 + len(a.sub_sweep)):]:
            print("%4d %-6s restart_rows %d  %-14s %9.1f us min %9.1f us median  %s" % (
                size, a.content, a.restart_rows, row["what"], row["us_min"], row["us_median"],
                {k: v for k, v in row.items() if k in ("taken", "rounds_mean", "rounds_max", "equals_form_0", "mean_file_bytes")}), flush=True)
            assert row.get("equals_form_0", True), "coefficients differ from the serial walk's"
        del coef, want, arena
    return rows


def measure_decode(a, lib, dev, pool):
    """orbit_frames_from_jpeg against PIL's decode, per frame size"""
    import glob
    import tempfile
    from orbit_dataset_amd.data import pipeline
    rows = []
    for size in a.sizes:
        with tempfile.TemporaryDirectory() as root:
            pipeline.write_synthetic_orbit_directory(root, users=1, objects_per_user=1, clean_videos=1, clutter_videos=0,
                                                     frames_per_video=a.frames, frame_size=size)
            paths = sorted(glob.glob(os.path.join(root, "*", "*", "*", "*", "*.jpg")))
            _rewrite_frames(a, paths, size)
            t0 = time.perf_counter()
            jf = pipeline.read_jpeg_frames(paths, pool)
            read_ms = 1e3 * (time.perf_counter() - t0)
            pil_s = []
            for _ in range(3):
                t0 = time.perf_counter()
                want = pipeline.decode_frames(paths, pool=pool)
                pil_s.append(time.perf_counter() - t0)
        assert not jf.pixels, "synthetic frames must all be in the device path's scope"
        u8 = torch.empty(jf.shape, dtype=torch.uint8, device=dev)
        pinned, held = {}, {}

        def run():
            status, done = pipeline._jpeg_launch(jf, u8, pinned, held, dev)
            done.synchronize()
            return status

        for _ in range(2):
            status = run()
        assert not status.numpy().any(), "a frame was not decoded on the device"
        exact = bool(np.array_equal(u8.cpu().numpy(), want))
        lib.orbit_prof_enable(1)
        for _ in range(a.reps):
            run()
        torch.cuda.synchronize()
        lib.orbit_prof_enable(0)
        ms, n = ctypes.c_double(), ctypes.c_long()
        lib.orbit_prof_collect(ctypes.byref(ms), None, ctypes.byref(n))
        kernels = {}
        for i in range(lib.orbit_prof_num_variants()):
            name, launches, kms = ctypes.create_string_buffer(48), ctypes.c_long(), ctypes.c_double()
            lib.orbit_prof_variant(i, name, ctypes.byref(launches), ctypes.byref(kms), None, None)
            kernels[name.value.decode()] = {"us_per_call": 1e3 * kms.value / a.reps, "launches_per_call": launches.value / a.reps}
        compressed, decoded = sum(len(f) for f in jf.files), int(np.prod(jf.shape))
        row = {"size": size, "frames": a.frames, "restart_rows": a.restart_rows, "content": a.content, "kernels": kernels, "us_per_call": 1e3 * ms.value / a.reps,
               "compressed_bytes": compressed, "decoded_bytes": decoded, "pil_ms": 1e3 * min(pil_s), "pil_threads": a.threads,
               "read_and_parse_ms": read_ms, "all_frames_equal_pil": exact}
        rows.append(row)
        print("%4d x %-4d %d frames, restart_rows %d: %s = %9.1f us per call | upload %.2f MB compressed, %.2f MB decoded (%.1fx) | PIL x%d threads "
              "%8.1f ms (%5.1fx) | read + parse %6.1f ms | frames %s PIL"
              % (size, size, a.frames, a.restart_rows, " + ".join("%s %.1f" % (k, v["us_per_call"]) for k, v in sorted(kernels.items())),
                 row["us_per_call"], compressed / 1e6, decoded / 1e6, decoded / compressed, a.threads, row["pil_ms"],
                 1e3 * row["pil_ms"] / row["us_per_call"], read_ms, "==" if exact else "!="), flush=True)
        assert exact, "a decoded frame differs from PIL"
        del u8
    return rows


def measure_encode(a, lib, dev, pool):
    """orbit_frames_to_jpeg against PIL's save, per content"""
    import io
    from orbit_dataset_amd.data import encode as enc
    size, n, rows = a.encode_size, a.frames, []
    y, x = np.mgrid[0:size, 0:size]
    rng = np.random.default_rng(0)
    for kind in ("smooth", "noise"):
        if kind == "noise":
            host = rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)
        else:
            host = np.stack([np.stack([(x * 7 + y * 3 + 5 * k) % 256, (y * 5 + 40 + k) % 256, (x * y + k) % 256], -1).astype(np.uint8)
                             for k in range(n)])
        u8 = torch.from_numpy(host).to(dev)

        def pil_one(i):
            buf = io.BytesIO()
            Image.fromarray(host[i]).save(buf, format="JPEG", quality=95)
            return buf.getvalue()

        pil_s = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = list(pool.map(pil_one, range(n)))
            pil_s.append(time.perf_counter() - t0)
        p = enc.encode_params(95, 0)
        stride = (lib.orbit_jpeg_encode_bound(size, size, 0, 0) + 15) // 16 * 16
        ws_bytes = lib.orbit_jpeg_encode_workspace_bytes(n, size, size)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        packed = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        sizes = torch.empty(n, dtype=torch.int32, device=dev)
        starts = torch.empty(n + 1, dtype=torch.int32, device=dev)

        def run():
            _lib.check(lib.orbit_frames_to_jpeg(_lib.dptr(u8), n, size, size, ctypes.byref(p), None, None, _lib.dptr(out), stride,
                                                _lib.dptr(sizes), _lib.dptr(ws), ws_bytes, _lib.stream_handle()), "orbit_frames_to_jpeg")
            _lib.check(lib.orbit_jpeg_compact(_lib.dptr(out), stride, _lib.dptr(sizes), n, _lib.dptr(packed), n * stride,
                                              _lib.dptr(starts), _lib.stream_handle()), "orbit_jpeg_compact")

        for _ in range(2):
            run()
        torch.cuda.synchronize()
        at = starts.cpu().numpy().astype(np.int64)
        data = packed[:int(at[n])].cpu().numpy().tobytes()
        exact = all(data[at[i]:at[i + 1]] == want[i] for i in range(n))
        lib.orbit_prof_enable(1)
        for _ in range(a.reps):
            run()
        torch.cuda.synchronize()
        lib.orbit_prof_enable(0)
        ms, launches = ctypes.c_double(), ctypes.c_long()
        lib.orbit_prof_collect(ctypes.byref(ms), None, ctypes.byref(launches))
        compressed = int(at[n])
        mcus = ((size + 15) // 16) ** 2
        blocks, px = 6 * mcus * n, n * size * size
        scan_bytes = compressed - n * 623  # (header and EOI apart; stuffed bytes counted, a small overestimate)
        algorithmic = {"jpeg_enc_color": 3 * px + 384 * mcus * n, "jpeg_enc_dct": 384 * mcus * n + 128 * blocks, "jpeg_enc_size": 132 * blocks,
                       "jpeg_enc_scan": 8 * blocks + scan_bytes, "jpeg_enc_pack": 136 * blocks + scan_bytes,
                       "jpeg_enc_ff": scan_bytes + scan_bytes // 8, "jpeg_enc_assemble": 2 * compressed + scan_bytes // 8,
                       "jpeg_compact": 2 * compressed}
        kernels = {}
        for i in range(lib.orbit_prof_num_variants()):
            name, count, kms = ctypes.create_string_buffer(48), ctypes.c_long(), ctypes.c_double()
            lib.orbit_prof_variant(i, name, ctypes.byref(count), ctypes.byref(kms), None, None)
            k = name.value.decode()
            kernels[k] = {"us_per_call": 1e3 * kms.value / a.reps, "launches_per_call": count.value / a.reps,
                          "byte_floor_us": 1e6 * algorithmic[k] / HBM_BYTES_PER_S}
        row = {"size": size, "frames": n, "content": kind, "kernels": kernels, "us_per_call": 1e3 * ms.value / a.reps,
               "compressed_bytes": compressed, "raw_bytes": 3 * px, "pil_ms": 1e3 * min(pil_s), "pil_ms_runs": [1e3 * v for v in pil_s],
               "pil_threads": a.threads, "all_files_equal_pil": exact}
        rows.append(row)
        print("%d x %d %-6s %d frames: %9.1f us per call (sum of kernels) | %.2f MB out of %.2f MB | PIL x%d threads %8.1f ms (%5.1fx) | files %s PIL"
              % (size, size, kind, n, row["us_per_call"], compressed / 1e6, 3 * px / 1e6, a.threads, row["pil_ms"],
                 1e3 * row["pil_ms"] / row["us_per_call"], "==" if exact else "!="), flush=True)
        for k, v in sorted(kernels.items()):
            print("    %-20s %8.1f us   byte floor %6.2f us" % (k, v["us_per_call"], v["byte_floor_us"]), flush=True)
        assert exact, "an encoded file differs from PIL's"
    return rows


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--encode", action="store_true", help="measure the JPEG encoder instead of the resize")
    p.add_argument("--encode_size", type=int, default=224, help="with --encode: the frame size")
    p.add_argument("--decode", action="store_true", help="measure the JPEG decoder instead of the resize")
    p.add_argument("--sizes", type=int, nargs="+", default=[224, 1080], help="with --decode: the frame sizes")
    p.add_argument("--restart_rows", type=int, default=0,
                   help="with --decode: re-save the frames with a restart marker every N MCU rows (Pillow's restart_marker_rows), "
                        "which the entropy kernel decodes with one lane per restart interval; 0 = no markers")
    p.add_argument("--content", choices=("smooth", "noise"), default="smooth",
                   help="with --decode: the frames write_synthetic_orbit_directory draws, or uniform noise (the least compressible content)")
    p.add_argument("--sub_sweep", type=int, nargs="+", default=None,
                   help="with --decode: measure the entropy stage alone instead - serial, interval form, and the subsequence form at "
                        "each of these sub_bytes (0 = the production rule)")
    p.add_argument("--frames", type=int, default=200)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--json", default=None, help="also write the rows to this file")
    a = p.parse_args(argv)
    _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    mean, std = (torch.tensor(v)[:, None, None] for v in NORMALIZE_STATS["imagenet"])
    pool = ThreadPoolExecutor(max_workers=a.threads)
    if a.encode:
        print("%d frames per call, device %s, PIL %s on %d threads" % (a.frames, torch.cuda.get_device_name(0), Image.__version__, a.threads))
        rows = measure_encode(a, lib, dev, pool)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        return rows
    if a.decode:
        print("%d frames per call, device %s, PIL %s on %d threads" % (a.frames, torch.cuda.get_device_name(0), Image.__version__, a.threads))
        rows = measure_sub_sweep(a, lib, dev, pool) if a.sub_sweep is not None else measure_decode(a, lib, dev, pool)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        return rows
    rows = []
    print("%d frames per launch, device %s, PIL %s on %d threads" % (a.frames, torch.cuda.get_device_name(0), Image.__version__, a.threads))
    for size_in, size_out in ((1080, 224), (224, 84)):
        u8 = torch.randint(0, 256, (a.frames, size_in, size_in, 3), dtype=torch.uint8, device=dev)
        host = u8.cpu().numpy()
        for resample in ("lanczos", "bicubic", "bilinear"):
            out = {}

            def run():
                out["y"] = frames_from_uint8(u8, dev, "imagenet", channels_last=True, size=size_out, resample=resample)

            us, nbytes, name = measure(lib, run, a.reps)
            floor_us = 1e6 * nbytes / HBM_BYTES_PER_S

            def pil_one(i):
                return np.array(Image.fromarray(host[i]).resize((size_out, size_out), PIL_FILTERS[resample]))

            pil_s = []
            for _ in range(3):
                t0 = time.perf_counter()
                resized = list(pool.map(pil_one, range(a.frames)))
                pil_s.append(time.perf_counter() - t0)
            want = (torch.from_numpy(resized[0]).permute(2, 0, 1).float().div(255) - mean) / std
            exact = bool(torch.equal(out["y"][0].cpu(), want))
            rows.append({"in": size_in, "out": size_out, "filter": resample, "kernel": name, "frames": a.frames, "us_per_launch": us,
                         "bytes_per_launch": nbytes, "gb_per_s": nbytes / us / 1e3, "byte_floor_us": floor_us,
                         "floor_over_time": floor_us / us, "pil_ms": 1e3 * min(pil_s), "pil_threads": a.threads, "first_frame_equals_pil": exact})
            print("%4d -> %3d %-8s %9.1f us/launch  %7.1f GB/s  (byte floor %6.1f us at 6.3 TB/s, %4.1f %% of the time)   PIL x%d threads %8.1f ms "
                  "(%5.0fx)   first frame %s PIL" % (size_in, size_out, resample, us, nbytes / us / 1e3, floor_us, 100 * floor_us / us,
                                                     a.threads, 1e3 * min(pil_s), 1e6 * min(pil_s) / us, "==" if exact else "!="), flush=True)
            assert exact, "the resized frame differs from PIL"
        del u8, host
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
