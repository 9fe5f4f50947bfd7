"""Restart-marked JPEG files for the tests of the interval-parallel entropy decode (test_jpeg_par_host.py,
test_gpu_jpeg_par.py): the case list with the form each file must take, the variants with misplaced markers, and the
stand-alone host program tools/jpeg_par_host_check.cpp built with the sanitizers."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

from jpeg_cases import ROOT, _encode_kw, content, damaged_sources, damaged_variants, ecs_start, pillow_rgb  # noqa: F401

TILE = 1024  # ORBIT_JPEG_STAGE_BYTES
MAX_INTERVALS = 1024  # JPEG_PAR_MAX_INTERVALS of csrc/jpeg_core.h
SERIAL, PARALLEL, REWALKED = 0, 1, 2  # `taken`


def restart_markers(data):
    """absolute offsets of the FF of every RSTn marker of the entropy-coded segment (there an FF is followed by 00 unless it
    starts a marker)"""
    s, out = ecs_start(data), []
    for i in range(s, len(data) - 1):
        if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7:
            out.append(i)
    return out


def _tile_edge_file():
    """case i: 1080 x 16 with a restart marker per MCU row, the FF of one marker being the last byte of a 1 KB tile of the
    segment (found by trying seeds)"""
    for seed in range(4000):
        data = _encode_kw(content("noise", 1080, 16, 7919 * seed), "RGB", restart_marker_rows=1)
        s = ecs_start(data)
        if any((m - s) % TILE == TILE - 1 for m in restart_markers(data)):
            return data
    return None


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (file, H, W, intervals by the geometry, the form the frame must take)"""
    b = _encode_kw(content("noise", 37, 53), "RGB", restart_marker_blocks=5, subsampling=2)
    first = restart_markers(b)[0]
    out = {
        "a": (_encode_kw(content("noise", 24, 40), "RGB", restart_marker_blocks=2, subsampling=2), 24, 40, 3, PARALLEL),
        "b": (b, 37, 53, 3, PARALLEL),
        "c": (_encode_kw(content("noise", 136, 24), "RGB", restart_marker_blocks=1, subsampling=2), 136, 24, 18, PARALLEL),
        "c444": (_encode_kw(content("noise", 136, 24), "RGB", restart_marker_blocks=1, subsampling=0), 136, 24, 51, PARALLEL),
        "d": (_encode_kw(content("noise", 1080, 16), "RGB", restart_marker_rows=1, subsampling=2), 1080, 16, 68, PARALLEL),
        "e": (_encode_kw(content("noise", 17, 23), "L", restart_marker_blocks=2), 17, 23, 5, PARALLEL),
        "f": (_encode_kw(content("noise", 33, 16), "RGB", restart_marker_rows=1, subsampling=1), 33, 16, 5, PARALLEL),
        "g": (b[:first] + b"\xff" + b[first:], 37, 53, 3, PARALLEL),  # a fill byte in front of the first marker
        "h": (_encode_kw(content("noise", 264, 264), "RGB", restart_marker_blocks=1, subsampling=0), 264, 264, 1089, SERIAL),
        "i": (_tile_edge_file(), 1080, 16, 68, PARALLEL),
        "j": (_encode_kw(content("noise", 8, 8), "RGB", restart_marker_rows=1), 8, 8, 1, SERIAL),
    }
    return out


def marker_free(H, W, seed=5):
    """a 4:2:0 file of the same size without restart markers"""
    return _encode_kw(content("noise", H, W, seed), "RGB", subsampling=2)


def misplaced_marker_variants(data):
    """name -> bytes, from a file with at least three restart markers: two of them swapped, one doubled, an EOI planted in
    front of the middle one"""
    m = restart_markers(data)
    assert len(m) >= 3 and data[m[0] + 1] != data[m[1] + 1]
    swapped = bytearray(data)
    swapped[m[0] + 1], swapped[m[1] + 1] = data[m[1] + 1], data[m[0] + 1]
    mid = m[len(m) // 2]
    return {"swapped": bytes(swapped), "doubled": data[:m[1]] + data[m[1]:m[1] + 2] + data[m[1]:],
            "eoi": data[:mid] + b"\xff\xd9" + data[mid:]}


def build_par_host_check(out_dir):
    """tools/jpeg_par_host_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer -> path of the program"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(out_dir, "jpeg_par_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "orbit-dataset_amd", "csrc"),
                    os.path.join(ROOT, "tools", "jpeg_par_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_par_host_check(exe, data, work_dir):
    """-> (exit code, {parse, serial, parallel, taken, equal, nseg, idct, width, height} or None, pixels or None, stderr)"""
    src, dst = os.path.join(work_dir, "in.jpg"), os.path.join(work_dir, "out.rgb")
    with open(src, "wb") as f:
        f.write(data)
    if os.path.exists(dst):
        os.remove(dst)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    if r.returncode != 0:
        return r.returncode, None, None, r.stderr
    w = r.stdout.split()
    res = {w[i]: int(w[i + 1]) for i in range(0, 18, 2)}
    pixels = np.fromfile(dst, dtype=np.uint8).reshape(res["height"], res["width"], 3) if os.path.exists(dst) else None
    return 0, res, pixels, r.stderr


# ---- the device side (used by the GPU tests only) ------------------------------------------------------------------------------
def upload(lib, device, files):
    """-> (arena tensor, descriptor tensor, parse codes): the files packed without padding, so no load may rely on alignment"""
    import torch
    from orbit_dataset_amd import _lib
    size = ctypes.sizeof(_lib.JpegDesc)
    descs = np.zeros((len(files), size), dtype=np.uint8)
    codes, at, offsets = [], 0, []
    for i, f in enumerate(files):
        codes.append(lib.orbit_jpeg_parse(f, len(f), descs[i].ctypes.data, size))
        offsets.append(at)
        at += len(f)
    descs.view(np.uint64)[:, 0] = offsets
    arena = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).to(device)
    return arena, torch.from_numpy(descs.reshape(-1)).to(device), codes


def cap_blocks(H, W):
    return 3 * (2 * ((W + 15) // 16)) * (2 * ((H + 15) // 16))


def device_entropy(lib, device, files, H, W, form):
    """orbit_op_jpeg_entropy -> (int16 [n, cap_blocks, 64] on the device, status list, taken list)"""
    import torch
    from orbit_dataset_amd import _lib
    n = len(files)
    arena, descs, codes = upload(lib, device, files)
    assert codes == [0] * n
    coef = torch.zeros((n, cap_blocks(H, W), 64), dtype=torch.int16, device=device)
    status = torch.full((n,), -99, dtype=torch.int32, device=device)
    taken = torch.full((n,), -99, dtype=torch.int32, device=device)
    _lib.check(lib.orbit_op_jpeg_entropy(_lib.dptr(arena), arena.numel(), _lib.dptr(descs), n, H, W, form, _lib.dptr(coef, torch.int16),
                                         coef.numel() * 2, _lib.dptr(status), _lib.dptr(taken), _lib.stream_handle()),
               "orbit_op_jpeg_entropy")
    torch.cuda.synchronize()
    return coef, status.cpu().tolist(), taken.cpu().tolist()


def device_decode(lib, device, files, H, W, workspace_bytes=None):
    """orbit_frames_from_jpeg -> (uint8 [n, H, W, 3] on the host, status list)"""
    import torch
    from orbit_dataset_amd import _lib
    n = len(files)
    arena, descs, codes = upload(lib, device, files)
    assert codes == [0] * n
    out = torch.full((n, H, W, 3), 77, dtype=torch.uint8, device=device)
    status = torch.full((n,), -99, dtype=torch.int32, device=device)
    ws_bytes = lib.orbit_jpeg_workspace_bytes(n, H, W) if workspace_bytes is None else workspace_bytes
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    _lib.check(lib.orbit_frames_from_jpeg(_lib.dptr(arena), arena.numel(), _lib.dptr(descs), n, H, W, _lib.dptr(out), _lib.dptr(status),
                                          _lib.dptr(ws), ws_bytes, _lib.stream_handle()), "orbit_frames_from_jpeg")
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().tolist()
