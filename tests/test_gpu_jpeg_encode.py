"""orbit_frames_to_jpeg (csrc/jpeg_enc.hip): frames encoded on the device equal the bytes of Pillow's
Image.save(quality=q[, restart_marker_rows=r]) byte for byte. The tolerance is zero and derived: libjpeg's baseline
compression path is integer arithmetic throughout (colour conversion, 2 x 2 averaging, islow forward DCT, quantiser, Huffman
coding), restated in csrc/jpeg_enc_core.h, and test_jpeg_enc_host.py establishes on the CPU that the restatement holds on this
grid. orbit_frames_resize_u8 likewise equals Image.resize. Every call goes through the C-ABI with guard bytes around the
output slices and the workspace."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from orbit_dataset_amd.data import encode as enc  # noqa: E402

from jpeg_enc_cases import SIZES, content, grid, pillow_bytes  # noqa: E402

GUARD = 256


def device_encode(lib, device, frames, quality, rows, comments=None, ws_frames=None, stream=None):
    """the C-ABI directly, guard bytes (0xA5) in front of, between and behind the output slices and around the workspace
    -> list of files"""
    frames = np.ascontiguousarray(frames)
    B, H, W = frames.shape[:3]
    p = enc.encode_params(quality, rows)
    offsets = d_comments = None
    longest = 0
    if comments is not None:
        offsets = np.zeros(B + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum([len(c) for c in comments])
        longest = max(len(c) for c in comments)
        d_comments = torch.from_numpy(np.frombuffer(b"".join(comments) + b"\0", dtype=np.uint8).copy()).to(device)
    bound = lib.orbit_jpeg_encode_bound(H, W, rows, longest)
    assert bound > 0
    stride = bound + GUARD  # every slice is followed by GUARD bytes that stay 0xA5
    one = lib.orbit_jpeg_encode_workspace_bytes(1, H, W)
    assert one > 0 and one % 16 == 0
    ws_bytes = one * (B if ws_frames is None else ws_frames)
    out = torch.full((GUARD + B * stride,), 0xA5, dtype=torch.uint8, device=device)
    ws = torch.full((GUARD + ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    sizes = torch.full((B + 2,), -1515870811, dtype=torch.int32, device=device)  # 0xA5A5A5A5
    d_frames = torch.from_numpy(frames).to(device)
    torch.cuda.synchronize()
    handle = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _lib.stream_handle()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _lib.check(lib.orbit_frames_to_jpeg(_lib.dptr(d_frames), B, H, W, ctypes.byref(p), _lib.dptr(d_comments),
                                        None if offsets is None else offsets.ctypes.data,
                                        ctypes.c_void_p(out.data_ptr() + GUARD), stride, ctypes.c_void_p(sizes.data_ptr() + 4),
                                        ctypes.c_void_p(ws.data_ptr() + GUARD), ws_bytes, handle), "orbit_frames_to_jpeg")
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    host, n = out.cpu().numpy(), sizes.cpu().numpy()
    assert n[0] == n[B + 1] == -1515870811, "a length was written outside out_bytes[0 .. B)"
    wsh = ws.cpu().numpy()
    assert (wsh[:GUARD] == 0xA5).all() and (wsh[GUARD + ws_bytes:] == 0xA5).all(), "the guard bytes around the workspace changed"
    assert (host[:GUARD] == 0xA5).all(), "the guard bytes in front of the output changed"
    files = []
    for b in range(B):
        s = GUARD + b * stride
        assert 0 < n[1 + b] <= bound, (b, n[1 + b], bound)
        assert (host[s + n[1 + b]:s + stride] == 0xA5).all(), "frame %d wrote behind its file" % b
        files.append(host[s:s + n[1 + b]].tobytes())
    return files


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_grid_equals_pillow(lib, device, size):
    cases = [c for c in grid() if c[:2] == size]
    assert len(cases) >= 5
    for H, W, quality, kind, rows in cases:
        got = device_encode(lib, device, content(kind, H, W)[None], quality, rows)
        assert got[0] == pillow_bytes(H, W, quality, kind, rows), (H, W, quality, kind, rows)


@pytest.mark.parametrize("rows", (0, 1))
def test_batch_of_five_with_different_content(lib, device, rows):
    for H, W in ((37, 53), (18, 22), (64, 64)):
        kinds = ("noise", "smooth", "constant", "checker", "redblue")
        frames = np.stack([content(k, H, W) for k in kinds])
        got = device_encode(lib, device, frames, 95, rows)
        for k, f in zip(kinds, got):
            assert f == pillow_bytes(H, W, 95, k, rows), (H, W, k, rows)


def test_chunked_workspace_gives_the_same_files(lib, device):
    """5 frames through a workspace that holds 2: three chunks"""
    H, W = 37, 53
    frames = np.stack([content("noise", H, W, seed) for seed in range(5)])
    got = device_encode(lib, device, frames, 75, 1, ws_frames=2)
    for seed, f in enumerate(got):
        assert f == pillow_bytes(H, W, 75, "noise", 1, seed=seed), seed


def test_comments_of_different_lengths(lib, device):
    H, W = 33, 16
    comments = [b"Lavc58.134.100", b"", b"x", bytes(range(1, 256)) * 3, b""]
    frames = np.stack([content("smooth", H, W, 0)] * 5)
    for rows in (0, 1):
        got = device_encode(lib, device, frames, 95, rows, comments=comments, ws_frames=2)
        for c, f in zip(comments, got):
            assert f == pillow_bytes(H, W, 95, "smooth", rows, c or None), (rows, len(c))
            assert (b"\xff\xfe" in f[:24]) == bool(c)


def test_side_stream(lib, device):
    H, W = 24, 40
    side = torch.cuda.Stream(device)
    frames = np.stack([content("noise", H, W, seed) for seed in range(3)])
    got = device_encode(lib, device, frames, 95, 0, stream=side)
    for seed, f in enumerate(got):
        assert f == pillow_bytes(H, W, 95, "noise", 0, seed=seed)


def test_frame_zero_does_not_depend_on_its_batch(lib, device):
    H, W = 37, 53
    frames = np.stack([content("noise", H, W, seed) for seed in range(3)])
    for rows in (0, 1):
        assert device_encode(lib, device, frames, 95, rows)[0] == device_encode(lib, device, frames[:1], 95, rows)[0]


def test_round_trip_through_the_device_decoder(lib, device):
    """orbit_frames_from_jpeg of the device-encoded files == Pillow's decode of Pillow's files"""
    from test_gpu_jpeg import device_decode
    for H, W, rows in ((37, 53, 0), (18, 22, 1), (64, 64, 1)):
        kinds = ("noise", "smooth", "redblue")
        files = device_encode(lib, device, np.stack([content(k, H, W) for k in kinds]), 95, rows)
        got, status, codes = device_decode(lib, device, files, H, W)
        assert codes == [0] * 3 and status == [0] * 3
        for i, k in enumerate(kinds):
            want = np.asarray(Image.open(io.BytesIO(pillow_bytes(H, W, 95, k, rows))).convert("RGB"))
            assert np.array_equal(got[i], want), (H, W, k)


def test_python_entry_point_and_compaction(device):
    """encode_frames_device: the files come back through orbit_jpeg_compact in one copy"""
    H, W = 37, 53
    frames = torch.from_numpy(np.stack([content("noise", H, W, seed) for seed in range(4)])).to(device)
    comments = [None, b"Lavc58.134.100", b"", b"abc"]
    got = enc.encode_frames_device(frames, quality=75, restart_rows=1, comments=comments)
    assert [type(f) for f in got] == [bytes] * 4
    for seed, (c, f) in enumerate(zip(comments, got)):
        assert f == pillow_bytes(H, W, 75, "noise", 1, c or None, seed=seed)
    # a workspace cap below one frame still encodes, one frame at a time
    assert enc.encode_frames_device(frames, quality=75, restart_rows=1, comments=comments, workspace_cap=1) == got
    assert enc.encode_frames_device(frames[:0]) == []


RESIZES = (((37, 53), (16, 16)), ((64, 48), (24, 24)), ((24, 24), (40, 56)))
PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


@pytest.mark.parametrize("resample", sorted(PIL_FILTERS))
def test_resize_u8_equals_pillow(device, resample):
    for (H, W), (Ho, Wo) in RESIZES:
        frames = np.stack([content("noise", H, W, seed) for seed in range(3)])
        want = np.stack([np.asarray(Image.fromarray(f).resize((Wo, Ho), PIL_FILTERS[resample])) for f in frames])
        got = enc.resize_frames_u8_device(torch.from_numpy(frames).to(device), (Ho, Wo), resample)
        assert got.shape == (3, Ho, Wo, 3) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want), (H, W, Ho, Wo, resample)
        planar = torch.from_numpy(frames).to(device).permute(0, 3, 1, 2).contiguous()
        assert torch.equal(enc.resize_frames_u8_device(planar, (Ho, Wo), resample, channels_last=False), got)
