"""JPEG files for the decoder tests (test_jpeg_host.py, test_gpu_jpeg.py, test_gpu_jpeg_pipeline.py): the size list, the
encodings Pillow writes them with, the damaged variants, and the stand-alone host program built with the sanitizers."""
import os
import shutil
import subprocess

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# narrow-chroma replication (chroma plane <= 2 wide), sides that are no multiple of the MCU on either axis, exact multiples
SIZES = [(1, 1), (8, 8), (2, 3), (3, 6), (9, 2), (17, 23), (33, 16), (24, 40), (37, 53)]
# name -> (mode, keyword arguments of Image.save)
ENCODINGS = {
    "default": ("RGB", {}),
    "444": ("RGB", {"subsampling": 0}),
    "422": ("RGB", {"subsampling": 1}),
    "420": ("RGB", {"subsampling": 2}),
    "q30": ("RGB", {"quality": 30}),
    "q95": ("RGB", {"quality": 95}),
    "optimize": ("RGB", {"optimize": True}),
    "restart": ("RGB", {"restart_marker_blocks": 2}),
    "gray": ("L", {}),
}
SAMPLING = {"default": (2, 2), "444": (1, 1), "422": (2, 1), "420": (2, 2), "q30": (2, 2), "q95": (2, 2), "optimize": (2, 2),
            "restart": (2, 2), "gray": (1, 1)}


def content(kind, H, W, seed=0):
    if kind == "noise":
        return np.random.default_rng(1000 * H + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * 7 + y * 3) % 256, (y * 5 + 40) % 256, (x * y) % 256], -1).astype(np.uint8)


def encode(pixels, enc):
    """uint8 [H, W, 3] -> the bytes of the JPEG file Pillow writes for encoding `enc`"""
    import io
    mode, kw = ENCODINGS[enc]
    buf = io.BytesIO()
    Image.fromarray(pixels).convert(mode).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pillow_rgb(data):
    import io
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def ecs_start(data):
    """offset of the entropy-coded segment: the byte behind the first SOS header"""
    i = 2
    while True:
        assert data[i] == 0xFF
        length = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xDA:
            return i + 2 + length
        i += 2 + length


def damaged_variants(data):
    """name -> bytes: the entropy segment cut at 25 / 50 / 90 %, one byte inverted at ten evenly spaced offsets of it, and the
    first restart marker removed (the file must have one)"""
    s = ecs_start(data)
    n = len(data) - s
    out = {"cut%d" % f: data[:s + n * f // 100] for f in (25, 50, 90)}
    for i in range(10):
        o = s + n * (2 * i + 1) // 20
        out["flip%d" % i] = data[:o] + bytes([data[o] ^ 0xFF]) + data[o + 1:]
    j = data.index(b"\xff\xd0", s)
    out["no_restart"] = data[:j] + data[j + 2:]
    return out


def damaged_sources():
    """three small files with restart markers: 4:2:0, 4:4:4 at quality 95, grayscale"""
    return {"420": encode(content("noise", 24, 40, 1), "restart"),
            "444": _encode_kw(content("noise", 37, 53, 2), "RGB", restart_marker_blocks=2, subsampling=0, quality=95),
            "gray": _encode_kw(content("noise", 17, 23, 3), "L", restart_marker_blocks=2)}


def _encode_kw(pixels, mode, **kw):
    import io
    buf = io.BytesIO()
    Image.fromarray(pixels).convert(mode).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def build_host_check(out_dir):
    """tools/jpeg_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer -> path of the program"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(out_dir, "jpeg_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "orbit-dataset_amd", "csrc"),
                    os.path.join(ROOT, "tools", "jpeg_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_host_check(exe, data, work_dir):
    """-> (exit code, parse code, status, pixels or None, stderr)"""
    src, dst = os.path.join(work_dir, "in.jpg"), os.path.join(work_dir, "out.rgb")
    with open(src, "wb") as f:
        f.write(data)
    if os.path.exists(dst):
        os.remove(dst)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    if r.returncode != 0:
        return r.returncode, None, None, None, r.stderr
    w = r.stdout.split()
    parse, status, W, H = int(w[1]), int(w[3]), int(w[5]), int(w[7])
    pixels = np.fromfile(dst, dtype=np.uint8).reshape(H, W, 3) if os.path.exists(dst) else None
    return 0, parse, status, pixels, r.stderr
