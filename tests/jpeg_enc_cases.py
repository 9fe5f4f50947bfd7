"""Frames for the encoder tests (test_jpeg_enc_host.py, test_gpu_jpeg_encode.py): the grid of sizes, qualities, contents and
restart rows on which the integer restatement of libjpeg's baseline encoder is known to equal Pillow's bytes, thinned to a
list that still holds every size with every content, every quality, and 18 x 22 / 37 x 53 with restart rows; Pillow's bytes
for a case (computed once per process); the stand-alone host program built with the sanitizers."""
import functools
import io
import os
import shutil
import subprocess

import numpy as np
from PIL import Image

import jpeg_cases

ROOT = jpeg_cases.ROOT
SIZES = jpeg_cases.SIZES + [(16, 16), (18, 22), (32, 32), (224, 224)]
QUALITIES = (100, 95, 75, 30, 1)
CONTENTS = ("noise", "smooth", "constant", "checker", "redblue")
RESTART_ROWS = (0, 1, 2)


def content(kind, H, W, seed=0):
    """uint8 [H, W, 3]: noise, jpeg_cases' smooth pattern, one colour, the 0 / 255 checkerboard (the most stuffed bytes per
    block), the red / blue 2 x 2 checker (chroma at its extremes)"""
    if kind in ("noise", "smooth"):
        return jpeg_cases.content(kind, H, W, seed)
    if kind == "constant":
        return np.full((H, W, 3), (200, 30, 90), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "checker":
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    a = (((x >> 1) + (y >> 1)) & 1).astype(np.uint8)
    return np.stack([a * 255, 0 * a, (1 - a) * 255], axis=-1).astype(np.uint8)


def grid():
    """[(H, W, quality, content, restart_rows)]: every size x content once, quality and restart rows rotating through them,
    then 18 x 22 (the size that tells the padding orders apart) and 37 x 53 with restart rows 1 and 2 on every content"""
    cases = []
    for i, (H, W) in enumerate(SIZES):
        for j, kind in enumerate(CONTENTS):
            cases.append((H, W, QUALITIES[(i + j) % 5], kind, RESTART_ROWS[(i + 2 * j) % 3]))
    for H, W in ((18, 22), (37, 53)):
        for rows in (1, 2):
            for j, kind in enumerate(CONTENTS):
                c = (H, W, QUALITIES[(j + rows) % 5], kind, rows)
                if c not in cases:
                    cases.append(c)
    return cases


@functools.lru_cache(maxsize=None)
def pillow_bytes(H, W, quality, kind, rows, comment=None, seed=0):
    kw = {}
    if rows:
        kw["restart_marker_rows"] = rows
    if comment:
        kw["comment"] = comment
    buf = io.BytesIO()
    Image.fromarray(content(kind, H, W, seed)).save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


def build_host_check(out_dir):
    """tools/jpeg_enc_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer -> path of the program"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(out_dir, "jpeg_enc_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "orbit-dataset_amd", "csrc"),
                    os.path.join(ROOT, "tools", "jpeg_enc_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_host_check(exe, pixels, quality, rows, work_dir, comment=None):
    """-> (exit code, file bytes or None, stderr)"""
    src, dst = os.path.join(work_dir, "in.rgb"), os.path.join(work_dir, "out.jpg")
    pixels.tofile(src)
    if os.path.exists(dst):
        os.remove(dst)
    H, W = pixels.shape[:2]
    cmd = [exe, src, str(H), str(W), str(quality), str(rows)] + ([comment] if comment else []) + [dst]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return r.returncode, None, r.stderr
    with open(dst, "rb") as f:
        return 0, f.read(), r.stderr
