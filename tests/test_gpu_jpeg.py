"""orbit_frames_from_jpeg (csrc/jpeg.hip): baseline JPEG files decoded on the device equal
np.asarray(Image.open(f).convert("RGB")) bit for bit. The tolerance is zero and derived: libjpeg's default decode path is
integer arithmetic throughout (Huffman decode, islow inverse DCT, triangle upsampling, table colour conversion), restated
in csrc/jpeg_core.h. Except in the fallback and damaged tests every frame must come from the device: parse code 0 and
status 0 are asserted, so no test can pass by routing its input to PIL."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from orbit_dataset_amd.data import pipeline  # noqa: E402

from jpeg_cases import ENCODINGS, SIZES, content, damaged_sources, damaged_variants, ecs_start, encode, pillow_rgb  # noqa: E402

DESC = ctypes.sizeof(_lib.JpegDesc)


def device_decode(lib, device, files, H, W, workspace_bytes=None):
    """the C-ABI directly: -> (uint8 [n, H, W, 3] on the host, status list, parse codes)"""
    n = len(files)
    descs = np.zeros((n, DESC), dtype=np.uint8)
    codes, at, offsets = [], 0, []
    for i, f in enumerate(files):
        codes.append(lib.orbit_jpeg_parse(f, len(f), descs[i].ctypes.data, DESC))
        offsets.append(at)
        at += len(f)  # packed, unaligned: the kernel's loads may not rely on alignment
    descs.view(np.uint64)[:, 0] = offsets
    arena = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()).to(device)
    d_descs = torch.from_numpy(descs.reshape(-1)).to(device)
    out = torch.full((n, H, W, 3), 77, dtype=torch.uint8, device=device)
    status = torch.full((n,), -99, dtype=torch.int32, device=device)
    need = lib.orbit_jpeg_workspace_bytes(n, H, W)
    assert need == n * lib.orbit_jpeg_workspace_bytes(1, H, W) > 0
    ws_bytes = need if workspace_bytes is None else workspace_bytes
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    _lib.check(lib.orbit_frames_from_jpeg(_lib.dptr(arena), arena.numel(), _lib.dptr(d_descs), n, H, W, _lib.dptr(out),
                                          _lib.dptr(status), _lib.dptr(ws), ws_bytes, _lib.stream_handle()), "orbit_frames_from_jpeg")
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().tolist(), codes


def assert_exact(lib, device, files, H, W, **kw):
    got, status, codes = device_decode(lib, device, files, H, W, **kw)
    assert codes == [0] * len(files) and status == [0] * len(files), (codes, status)
    for i, f in enumerate(files):
        assert np.array_equal(got[i], pillow_rgb(f)), "frame %d of %dx%d differs from Pillow" % (i, H, W)
    return got


@pytest.mark.parametrize("enc", sorted(ENCODINGS))
def test_size_list_equals_pillow(lib, device, enc):
    for H, W in SIZES:
        assert_exact(lib, device, [encode(content(kind, H, W), enc) for kind in ("noise", "smooth")], H, W)


def test_mixed_batch(lib, device):
    """4:2:0, 4:4:4, grayscale, per-file Huffman tables and two qualities in one launch"""
    H, W = 24, 40
    files = [encode(content("noise", H, W, k), enc) for k, enc in enumerate(("420", "444", "gray", "optimize", "q30", "q95", "422"))]
    files += [encode(content("smooth", H, W), enc) for enc in ("optimize", "gray", "q30")]
    assert_exact(lib, device, files, H, W)


def test_long_stream_with_a_stuffed_byte_across_a_staging_boundary(lib, device):
    """a noise image at quality 95 whose entropy segment spans at least three staging tiles and holds an FF 00 pair with the FF
    as the last byte of one tile and the 00 as the first of the next (found by trying seeds, on the CPU)"""
    tile = _lib.JPEG_STAGE_BYTES
    H, W = 48, 56
    for seed in range(4000):
        data = encode(content("noise", H, W, 7919 * seed), "q95")
        s = ecs_start(data)
        n = len(data) - s
        hits = [b for b in range(tile, n - 1, tile) if data[s + b - 1] == 0xFF and data[s + b] == 0x00]
        if hits:
            break
    else:
        pytest.fail("no seed puts FF 00 across a tile boundary")
    assert n >= 3 * tile and hits and data[s + hits[0] - 1:s + hits[0] + 1] == b"\xff\x00"
    assert_exact(lib, device, [data, encode(content("smooth", H, W), "q95")], H, W)


def test_one_frame_of_the_synthetic_tree(device, tmp_path):
    pipeline.write_synthetic_orbit_directory(str(tmp_path), users=1, objects_per_user=1, clean_videos=1, clutter_videos=0,
                                             frames_per_video=1, frame_size=224)
    paths = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith(".jpg")]
    assert len(paths) == 1
    stats = {}
    got = pipeline.decode_frames_device(paths, device, stats=stats)
    assert stats["fallback_frames"] == 0 and stats["status"] == [0] and got.shape == (1, 224, 224, 3) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), pipeline.decode_frames(paths))


def test_chunked_workspace_gives_the_same_pixels(lib, device):
    H, W = 33, 16
    files = [encode(content("noise", H, W, k), ("420", "444", "gray", "422", "restart")[k % 5]) for k in range(11)]
    whole = assert_exact(lib, device, files, H, W)
    one = lib.orbit_jpeg_workspace_bytes(1, H, W)
    for frames_per_chunk in (1, 4):  # 11 chunks; 2 chunks of 4 and one of 3
        chunked = assert_exact(lib, device, files, H, W, workspace_bytes=frames_per_chunk * one + 64)
        assert np.array_equal(chunked, whole)


def test_out_of_scope_files_are_decoded_by_pil(device, tmp_path):
    import io
    from PIL import Image
    H, W = 24, 40
    files = [encode(content("noise", H, W, k), "420") for k in range(4)]
    buf = io.BytesIO()
    Image.fromarray(content("smooth", H, W)).save(buf, format="JPEG", progressive=True)
    files.insert(2, buf.getvalue())
    paths = []
    for i, f in enumerate(files):
        paths.append(str(tmp_path / ("%d.jpg" % i)))
        open(paths[-1], "wb").write(f)
    stats = {}
    got = pipeline.decode_frames_device(paths, device, stats=stats).cpu().numpy()
    assert stats["fallback_frames"] == 1 and stats["out_of_scope"] == 1 and stats["damaged"] == 0
    assert stats["status"] == [0, 0, -1, 0, 0]  # -ORBIT_JPEG_PROGRESSIVE: skipped on the device
    for i, f in enumerate(files):
        assert np.array_equal(got[i], pillow_rgb(f))


# one cut and one inverted byte that tests/test_jpeg_host.py runs through the same walker under the sanitizers
DAMAGED = (("420", "cut50"), ("444", "flip3"))


def test_damaged_files_get_a_status_and_leave_the_others_exact(lib, device):
    sources = damaged_sources()
    for name, variant in DAMAGED:
        good = sources[name]
        H, W = pillow_rgb(good).shape[:2]
        bad = damaged_variants(good)[variant]
        enc = {"420": "420", "444": "444"}[name]
        others = [encode(content("noise", H, W, k), enc) for k in range(3)]
        files = [others[0], bad, others[1], good, others[2]]
        got, status, codes = device_decode(lib, device, files, H, W)
        assert codes == [0] * 5
        assert status[1] > 0 and [status[i] for i in (0, 2, 3, 4)] == [0] * 4, status
        for i in (0, 2, 3, 4):
            assert np.array_equal(got[i], pillow_rgb(files[i]))
