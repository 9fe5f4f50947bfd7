"""JPEG files WITHOUT restart markers for the tests of the subsequence-parallel entropy decode (test_jpeg_sub_host.py,
test_gpu_jpeg_sub.py): the case list, the subsequence sizes every case runs at, the rule that says which form a frame takes
(restated from csrc/jpeg_core.h), and the stand-alone host program tools/jpeg_sub_host_check.cpp built with the sanitizers."""
import functools
import os
import shutil
import subprocess

import numpy as np

from jpeg_cases import ROOT, _encode_kw, content, ecs_start, pillow_rgb  # noqa: F401
from jpeg_par_cases import cap_blocks, device_decode, device_entropy, upload  # noqa: F401
from jpeg_par_cases import cases as par_cases

SUB_MAX = 1024  # JPEG_SUB_MAX of csrc/jpeg_core.h
SUB_BYTES, SUB_PER_ROUND, SUB_MIN_BYTES, SUB_MIN_MCUS = 128, 256, 512, 64  # the production rule's constants, same file
SERIAL, PARALLEL, SUB, SUB_REWALKED = 0, 1, 3, 4  # `taken`
SIZES = (4, 16, 128, 1 << 20)  # S; the last is larger than every segment here: N = 1, the frame is walked serially


def _flat(H, W):
    return np.full((H, W, 3), 117, dtype=np.uint8)


def _stuffed_edge_file(S=16):
    """a file in which the 00 of a stuffed FF 00 is the first byte of a subsequence of S bytes (found by trying seeds)"""
    for seed in range(400):
        data = _encode_kw(content("noise", 24, 40, 977 * seed), "RGB", subsampling=2, quality=95)
        s = ecs_start(data)
        if any(data[i] == 0 and data[i - 1] == 0xFF for i in range(s + S, len(data) - 2, S)):
            return data
    return None


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (file, H, W); all without restart markers but `restart`"""
    out = {
        "one_mcu_8": (_encode_kw(content("noise", 8, 8), "RGB", subsampling=2), 8, 8),
        "one_mcu_16": (_encode_kw(content("noise", 16, 16), "RGB", subsampling=2), 16, 16),
        "gray": (_encode_kw(content("noise", 17, 23), "L"), 17, 23),
        "444": (_encode_kw(content("noise", 24, 40), "RGB", subsampling=0), 24, 40),
        "422": (_encode_kw(content("noise", 33, 16), "RGB", subsampling=1), 33, 16),
        "420_noise": (_encode_kw(content("noise", 37, 53), "RGB", subsampling=2), 37, 53),
        "smooth": (_encode_kw(content("smooth", 48, 56), "RGB", subsampling=2), 48, 56),
        "flat": (_encode_kw(_flat(64, 64), "RGB", subsampling=2), 64, 64),
        "wide": (_encode_kw(content("noise", 1080, 16), "RGB", subsampling=2), 1080, 16),
        "stuffed_edge": (_stuffed_edge_file(), 24, 40),
        "restart": par_cases()["a"][:3],
    }
    return out


def ecs_bytes(data):
    return len(data) - ecs_start(data)


def mcus(data):
    """MCUs of the frame, from its SOF0 header: sides over 8 times the first component's sampling factors, rounded up"""
    i = data.index(b"\xff\xc0")
    H, W, ncomp = (data[i + 5] << 8) | data[i + 6], (data[i + 7] << 8) | data[i + 8], data[i + 9]
    h, v = (data[i + 11] >> 4, data[i + 11] & 15) if ncomp == 3 else (1, 1)
    return -(-W // (8 * h)) * -(-H // (8 * v))


def rule(data, sub_bytes, has_restart=False):
    """-> (the `taken` a well-formed file must report, N): jpeg_sub_size of csrc/jpeg_core.h"""
    if has_restart:
        return PARALLEL, 0
    n_bytes = ecs_bytes(data)
    S = sub_bytes
    if sub_bytes == 0:
        if n_bytes < SUB_MIN_BYTES or mcus(data) < SUB_MIN_MCUS:
            return SERIAL, 0
        S = SUB_BYTES
        while -(-n_bytes // S) > SUB_PER_ROUND:
            S *= 2
    n = -(-n_bytes // S)
    return (SUB, n) if 2 <= n <= SUB_MAX else (SERIAL, 0)


def damaged(data):
    """name -> bytes: the `cut50` and `flip3` of jpeg_cases.damaged_variants - the entropy segment cut at 50 %, the byte at 7 / 20
    of it inverted - restated, because that function also removes a restart marker and these files have none"""
    s = ecs_start(data)
    n = len(data) - s
    o = s + n * 7 // 20
    return {"cut50": data[:s + n * 50 // 100], "flip3": data[:o] + bytes([data[o] ^ 0xFF]) + data[o + 1:]}


def other_file(H, W, seed=5):
    """another 4:2:0 file of the same size without restart markers"""
    return _encode_kw(content("noise", H, W, seed), "RGB", subsampling=2)


def build_sub_host_check(out_dir):
    """tools/jpeg_sub_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer -> path of the program"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(out_dir, "jpeg_sub_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "orbit-dataset_amd", "csrc"),
                    os.path.join(ROOT, "tools", "jpeg_sub_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_sub_host_check(exe, data, work_dir, sub_bytes):
    """-> (exit code, {parse, serial, sub, taken, equal, n, rounds, decodes, idct, width, height} or None, pixels or None, stderr)"""
    src, dst = os.path.join(work_dir, "in.jpg"), os.path.join(work_dir, "out.rgb")
    with open(src, "wb") as f:
        f.write(data)
    if os.path.exists(dst):
        os.remove(dst)
    r = subprocess.run([exe, src, dst, str(sub_bytes)], capture_output=True, text=True)
    if r.returncode != 0:
        return r.returncode, None, None, r.stderr
    w = r.stdout.split()
    res = {w[i]: int(w[i + 1]) for i in range(0, 22, 2)}
    pixels = np.fromfile(dst, dtype=np.uint8).reshape(res["height"], res["width"], 3) if os.path.exists(dst) else None
    return 0, res, pixels, r.stderr


# ---- the device side (used by the GPU tests only) ------------------------------------------------------------------------------
def device_entropy_sub(lib, device, files, H, W, sub_bytes):
    """orbit_op_jpeg_entropy_sub -> (int16 [n, cap_blocks, 64] on the device, status list, taken list, rounds list)"""
    import torch
    from orbit_dataset_amd import _lib
    n = len(files)
    arena, descs, codes = upload(lib, device, files)
    assert codes == [0] * n
    coef = torch.zeros((n, cap_blocks(H, W), 64), dtype=torch.int16, device=device)
    status, taken, rounds = (torch.full((n,), -99, dtype=torch.int32, device=device) for _ in range(3))
    _lib.check(lib.orbit_op_jpeg_entropy_sub(_lib.dptr(arena), arena.numel(), _lib.dptr(descs), n, H, W, sub_bytes,
                                             _lib.dptr(coef, torch.int16), coef.numel() * 2, _lib.dptr(status), _lib.dptr(taken),
                                             _lib.dptr(rounds), _lib.stream_handle()), "orbit_op_jpeg_entropy_sub")
    torch.cuda.synchronize()
    return coef, status.cpu().tolist(), taken.cpu().tolist(), rounds.cpu().tolist()
