"""orbit_frames_resize_from_uint8 (csrc/ingest.hip) on hardware: 8-bit frames resized and normalised in one launch must EQUAL
Pillow's Image.resize of the same frames followed by the reference transform (to_tensor + normalize, data/datasets.py:422-431)
on the CPU - torch.equal, no tolerance: the resize is Pillow's integer arithmetic on Pillow's tables, the transform the same
two fp32 operations in the same order."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from orbit_dataset_amd.data.utils import NORMALIZE_STATS, frames_from_uint8  # noqa: E402

PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
# (H_in, W_in) -> (H_out, W_out)
SHAPES = [((224, 224), (84, 84)),    # ratio 2.67; 84 is no multiple of the 16 x 32 tile: tails on both axes, several blocks,
          #                              and 54 input rows per tile: two staging rounds of 32, the second short
          ((37, 53), (84, 84)),      # upscale, non-square
          ((225, 223), (84, 84)),    # odd sizes
          ((96, 64), (32, 48)),      # another ratio per axis
          ((64, 96), (64, 48)),      # vertical pass skipped
          ((96, 64), (48, 64)),      # horizontal pass skipped
          ((5, 7), (3, 2))]          # the window is wider than the image: both edge clamps


def frames(seed, B, H, W):
    """frame 0 .. : uniform noise, then a random 0 / 255 image (drives lanczos / bicubic overshoot into both clamps, in the
    intermediate rows and in the result), alternating"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    out[1::2] = rng.integers(0, 2, size=out[1::2].shape, dtype=np.uint8) * 255
    return out


def reference(u8_bhwc, out_hw, resample, method):
    mean, std = (torch.tensor(v)[None, :, None, None] for v in NORMALIZE_STATS[method])
    resized = np.stack([np.asarray(Image.fromarray(f).resize((out_hw[1], out_hw[0]), PIL_FILTERS[resample])) for f in u8_bhwc])
    return (torch.from_numpy(resized).permute(0, 3, 1, 2).float().div(255) - mean) / std


def run(u8_bhwc, out_hw, resample, method, channels_last, device):
    src = torch.from_numpy(u8_bhwc)
    if not channels_last:
        src = src.permute(0, 3, 1, 2).contiguous()
    return frames_from_uint8(src, device, method, channels_last=channels_last, size=out_hw, resample=resample).cpu()


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("resample", ["bilinear", "bicubic", "lanczos"])
@pytest.mark.parametrize("hw_in,hw_out", SHAPES)
def test_resize_equals_pillow(device, hw_in, hw_out, resample, channels_last):
    u8 = frames(hw_in[0] * 1000 + hw_in[1], 3, *hw_in)
    got = run(u8, hw_out, resample, "imagenet", channels_last, device)
    want = reference(u8, hw_out, resample, "imagenet")
    assert got.shape == want.shape == (3, 3, *hw_out)
    bad = (got != want)
    assert torch.equal(got, want), "%d of %d values differ" % (int(bad.sum()), bad.numel())


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("resample", ["bilinear", "bicubic", "lanczos"])
def test_one_1080_frame_to_224(device, resample, channels_last):
    """the real window: 31 taps per axis with lanczos, a 16-row tile reads about 106 input rows"""
    u8 = np.concatenate([frames(1080, 1, 1080, 1080)[:, :540], frames(1081, 2, 1080, 1080)[1:, 540:]], axis=1)  # noise above 0 / 255
    got = run(u8, (224, 224), resample, "imagenet", channels_last, device)
    assert torch.equal(got, reference(u8, (224, 224), resample, "imagenet"))


@pytest.mark.parametrize("method", ["imagenet", "openai_clip"])
def test_normalisation_statistics_and_leading_dimensions(device, method):
    u8 = frames(7, 6, 37, 53)
    clips = torch.from_numpy(u8).reshape(3, 2, 37, 53, 3)  # [clips, T, H, W, 3]
    got = frames_from_uint8(clips.pin_memory(), device, method, channels_last=True, size=(48, 40), resample="lanczos")
    assert got.shape == (3, 2, 3, 48, 40)
    assert torch.equal(got.cpu().reshape(6, 3, 48, 40), reference(u8, (48, 40), "lanczos", method))
    # an int is a square size
    assert torch.equal(frames_from_uint8(clips, device, method, size=32, resample="bicubic").cpu().reshape(6, 3, 32, 32),
                       reference(u8, (32, 32), "bicubic", method))


def test_stored_size_takes_the_existing_call(device, lib):
    """size=None, or size equal to the stored size: the launch and the values of the call without a resize"""
    u8 = torch.from_numpy(frames(11, 3, 37, 41))
    plain = frames_from_uint8(u8, device)
    lib.orbit_prof_enable(1)
    try:
        same = [frames_from_uint8(u8, device, size=None), frames_from_uint8(u8, device, size=(37, 41), resample="bilinear")]
        lib.orbit_prof_collect(None, None, None)
        assert lib.orbit_prof_num_variants() == 0  # the resize launch would have left a record
        resized = frames_from_uint8(u8, device, size=(20, 41), resample="bilinear")
        torch.cuda.synchronize()
        n = ctypes.c_long(0)
        lib.orbit_prof_collect(None, None, ctypes.byref(n))
        buf, b = ctypes.create_string_buffer(48), ctypes.c_double(0)
        lib.orbit_prof_variant(0, buf, None, None, None, ctypes.byref(b))
    finally:
        lib.orbit_prof_enable(0)
    assert all(torch.equal(t, plain) for t in same)
    assert n.value == 1 and buf.value.decode() == "frames_resize<bilinear>"
    assert b.value == 3 * (3 * 37 * 41 + 4 * 3 * 20 * 41) and resized.shape == (3, 3, 20, 41)  # bytes in + bytes out


def test_large_ratios_both_ways(device):
    """1080 -> 32 on both axes (a 205-tap lanczos window: the tile drops to 4 output rows to hold its input rows beside the
    staged 1080-pixel ones) and 32 -> 1080"""
    u8 = frames(5, 1, 1080, 1080)
    assert torch.equal(run(u8, (32, 32), "lanczos", "imagenet", True, device), reference(u8, (32, 32), "lanczos", "imagenet"))
    assert torch.equal(run(u8, (32, 32), "bicubic", "imagenet", False, device), reference(u8, (32, 32), "bicubic", "imagenet"))
    u8 = frames(6, 1, 32, 32)
    assert torch.equal(run(u8, (1080, 1080), "lanczos", "imagenet", False, device), reference(u8, (1080, 1080), "lanczos", "imagenet"))


def test_oversize_request_is_refused_and_nothing_is_launched(device, lib):
    """a 4000 -> 4 row lanczos window spans the whole 4000-row image; a tile's 64 KB of LDS holds 682 resampled rows"""
    u8 = torch.zeros(1, 4000, 8, 3, dtype=torch.uint8, device=device)
    lib.orbit_prof_enable(1)
    try:
        with pytest.raises(ValueError, match="window"):
            frames_from_uint8(u8, device, size=(4, 8))
        with pytest.raises(ValueError, match="limit"):
            frames_from_uint8(u8, device, size=(8, 20000))
        # 1500 -> 14 rows: a 643-row window fits alone (62 KB), but not beside one 2000-pixel input row of the tile (6 KB)
        with pytest.raises(ValueError, match="exceed"):
            frames_from_uint8(torch.zeros(1, 1500, 2000, 3, dtype=torch.uint8, device=device), device, size=(14, 16))
        n = ctypes.c_long(-1)
        lib.orbit_prof_collect(None, None, ctypes.byref(n))
    finally:
        lib.orbit_prof_enable(0)
    assert n.value == 0
    with pytest.raises(ValueError, match="nearest"):
        frames_from_uint8(u8, device, size=(4, 8), resample="nearest")
    torch.cuda.synchronize()
