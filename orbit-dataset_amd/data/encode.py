"""The output side of the offline resize pass (reference scripts/resize_videos.py:38-47: Image.open -> convert('RGB') ->
resize((s, s), LANCZOS) -> save(quality=95) on host threads) on the device:

  resize_frames_u8_device   uint8 frames -> uint8 frames at another size, equal to PIL's Image.resize of each (csrc/ingest.hip,
                            orbit_frames_resize_u8: the resize of the input pipeline with an 8-bit store).
  encode_frames_device      uint8 frames [B, H, W, 3] -> the bytes of the JPEG files PIL's Image.save(quality=q) writes for them
                            (csrc/jpeg_enc.hip, orbit_frames_to_jpeg), compacted on the device so that one copy of about the
                            compressed size brings a batch back.
  resize_tree               the whole pass over a directory tree (tools/resize_videos.py is its command line).
"""
import ctypes
import io
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .utils import output_size, resample_filter

ENCODE_WORKSPACE_CAP = 1 << 30  # bytes of encoder workspace per call; more frames go through it in chunks (orbit_frames_to_jpeg)


def resize_frames_u8_device(frames, size, resample="lanczos", channels_last=True):
    """uint8 device frames [B, H, W, 3] (or [B, 3, H, W] with channels_last=False) -> uint8 [B, Ho, Wo, 3], bit-identical to
    np.asarray(Image.fromarray(frame).resize((Wo, Ho), resample)). size: an int or (Ho, Wo)."""
    from .. import _lib
    _lib.require_gpu()
    lib = _lib.load()
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError("expected uint8 frames [B, H, W, 3], got %s %s" % (frames.dtype, tuple(frames.shape)))
    B, H, W = (frames.shape[0], frames.shape[1], frames.shape[2]) if channels_last else (frames.shape[0], frames.shape[2], frames.shape[3])
    Ho, Wo = output_size(size, H, W)
    with torch.cuda.device(frames.device):
        out = torch.empty((B, Ho, Wo, 3), dtype=torch.uint8, device=frames.device)
        if B:
            _lib.check(lib.orbit_frames_resize_u8(_lib.dptr(frames, torch.uint8), 1 if channels_last else 0, B, H, W, Ho, Wo,
                                                  resample_filter(resample), _lib.dptr(out), _lib.stream_handle()),
                       "orbit_frames_resize_u8")
    return out


def encode_params(quality=95, restart_rows=0):
    from .. import _lib
    p = _lib.JpegEnc()
    _lib.check(_lib.load().orbit_jpeg_encode_params(int(quality), int(restart_rows), ctypes.byref(p), ctypes.sizeof(p)),
               "orbit_jpeg_encode_params")
    return p


def encode_frames_device(u8_hwc, quality=95, restart_rows=0, comments=None, workspace_cap=ENCODE_WORKSPACE_CAP):
    """uint8 device frames [B, H, W, 3] -> list of B bytes objects: the baseline 4:2:0 JPEG files PIL writes for them with
    Image.save(quality=quality[, restart_marker_rows=restart_rows]), byte for byte. comments: per frame None / b"" or the bytes
    of a COM segment (what PIL carries over from Image.info["comment"])."""
    from .. import _lib
    _lib.require_gpu()
    lib = _lib.load()
    if u8_hwc.dtype != torch.uint8 or u8_hwc.dim() != 4 or u8_hwc.shape[3] != 3:
        raise ValueError("expected uint8 frames [B, H, W, 3], got %s %s" % (u8_hwc.dtype, tuple(u8_hwc.shape)))
    B, H, W = int(u8_hwc.shape[0]), int(u8_hwc.shape[1]), int(u8_hwc.shape[2])
    if B == 0:
        return []
    params = encode_params(quality, restart_rows)
    device = u8_hwc.device
    with torch.cuda.device(device):
        offsets = d_comments = None
        longest = 0
        if comments is not None and any(comments):
            if len(comments) != B:
                raise ValueError("%d comments for %d frames" % (len(comments), B))
            blobs = [bytes(c) if c else b"" for c in comments]
            offsets = np.zeros(B + 1, dtype=np.uint32)
            offsets[1:] = np.cumsum([len(c) for c in blobs])
            longest = max(len(c) for c in blobs)
            d_comments = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).to(device)
        stride = lib.orbit_jpeg_encode_bound(H, W, int(restart_rows), longest)
        if stride == 0:
            raise ValueError("encode_frames_device: %dx%d frames (restart_rows %d, a comment of %d bytes) are outside the encoder's limits"
                             % (H, W, restart_rows, longest))
        stride = (stride + 15) // 16 * 16
        one = lib.orbit_jpeg_encode_workspace_bytes(1, H, W)
        ws_bytes = min(one * B, max(workspace_cap // one, 1) * one)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        out = torch.empty(B * stride, dtype=torch.uint8, device=device)
        packed = torch.empty(B * stride, dtype=torch.uint8, device=device)
        sizes = torch.empty(B, dtype=torch.int32, device=device)
        starts = torch.empty(B + 1, dtype=torch.int32, device=device)
        _lib.check(lib.orbit_frames_to_jpeg(_lib.dptr(u8_hwc, torch.uint8), B, H, W, ctypes.byref(params), _lib.dptr(d_comments),
                                            None if offsets is None else offsets.ctypes.data, _lib.dptr(out), stride, _lib.dptr(sizes),
                                            _lib.dptr(ws), ws_bytes, _lib.stream_handle()), "orbit_frames_to_jpeg")
        _lib.check(lib.orbit_jpeg_compact(_lib.dptr(out), stride, _lib.dptr(sizes), B, _lib.dptr(packed), B * stride, _lib.dptr(starts),
                                          _lib.stream_handle()), "orbit_jpeg_compact")
        at = starts.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        data = packed[:int(at[B])].cpu().numpy().tobytes()
    return [data[at[b]:at[b + 1]] for b in range(B)]


# ---- the pass over a tree ----------------------------------------------------------------------------------------------------------
def _read_source(path):
    """-> (file bytes, parse code, orbit_jpeg_desc_t as uint8 array, (H, W), PIL-decoded pixels or None, comment or None)"""
    from PIL import Image
    from .. import _lib
    from .pipeline import _pil_rgb
    lib = _lib.load()
    with open(path, "rb") as f:
        data = f.read()
    desc = np.zeros(ctypes.sizeof(_lib.JpegDesc), dtype=np.uint8)
    code = lib.orbit_jpeg_parse(data, len(data), desc.ctypes.data, desc.size)
    with Image.open(io.BytesIO(data)) as im:
        comment = im.info.get("comment")  # what resize() and convert() keep and save() writes as the COM segment
    if isinstance(comment, str):
        comment = comment.encode()
    pixels = None
    if code != 0:  # progressive, CMYK, not a JPEG ..: PIL decodes it, it joins its batch as pixels
        pixels = _pil_rgb(data)
        size = pixels.shape[:2]
    else:
        d = desc.view(np.int32)
        size = (int(d[6]), int(d[5]))
    return data, code, desc, size, pixels, comment


def resize_tree(data_path, save_path, size=224, nthreads=12, quality=95, resample="lanczos", restart_rows=0, batch=200, device="cuda"):
    """Every .jpg under data_path -> the same relative path under save_path, resized to size x size and re-encoded: the
    reference's scripts/resize_videos.py, file for file and byte for byte with the installed Pillow at the default flags.
    Threads read and parse the files and write the results; decode (orbit_frames_from_jpeg), resize and encode run on the
    device, a batch of frames of one source size at a time. Files the device decoder leaves to the host (or reports damaged)
    are decoded by PIL. Returns {"frames", "seconds", "frames_per_s", "host_decoded"}."""
    from .. import _lib
    from .pipeline import JpegFrames, _jpeg_launch, _pil_rgb
    _lib.require_gpu()
    device = torch.device(device)
    t0 = time.perf_counter()
    paths = []
    for root, _, files in sorted(os.walk(data_path)):
        paths += [os.path.join(root, f) for f in sorted(files) if f.lower().endswith((".jpg", ".jpeg"))]
    host_decoded = 0
    pinned, held = {}, {}

    def write(job):
        path, data = job
        dst = os.path.join(save_path, os.path.relpath(path, data_path))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "wb") as f:
            f.write(data)

    def run_batch(pool, group, hw):
        nonlocal host_decoded
        H, W = hw
        jf = JpegFrames([g[1][0] for g in group], np.stack([g[1][2] for g in group]), [g[1][1] for g in group],
                        {i: g[1][4] for i, g in enumerate(group) if g[1][4] is not None}, (len(group),), hw)
        with torch.cuda.device(device):
            u8 = torch.empty((len(group), H, W, 3), dtype=torch.uint8, device=device)
            status, done = _jpeg_launch(jf, u8, pinned, held, device)
            done.synchronize()
            bad = [i for i in range(len(group)) if status[i] > 0]
            for i in bad:
                u8[i].copy_(torch.from_numpy(_pil_rgb(jf.files[i])))
            host_decoded += len(jf.pixels) + len(bad)
            small = resize_frames_u8_device(u8, size, resample)
            files = encode_frames_device(small, quality, restart_rows, [g[1][5] for g in group])
        return list(pool.map(write, [(g[0], data) for g, data in zip(group, files)]))

    with ThreadPoolExecutor(max_workers=max(1, int(nthreads))) as pool:
        groups = {}
        for k0 in range(0, len(paths), 4 * batch):  # read ahead a few batches at a time: the files of a tree need not fit in memory
            part = paths[k0:k0 + 4 * batch]
            for path, src in zip(part, pool.map(_read_source, part)):
                g = groups.setdefault(src[3], [])
                g.append((path, src))
                if len(g) == batch:
                    run_batch(pool, g, src[3])
                    groups[src[3]] = []
        for hw, g in groups.items():
            if g:
                run_batch(pool, g, hw)
    seconds = time.perf_counter() - t0
    return {"frames": len(paths), "seconds": seconds, "frames_per_s": len(paths) / seconds if seconds > 0 else 0.0,
            "host_decoded": host_decoded}
