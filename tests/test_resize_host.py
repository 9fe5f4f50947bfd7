"""Host side of the on-device frame resize (csrc/ingest.hip): orbit_resize_coeffs, the table the launcher of
orbit_frames_resize_from_uint8 uploads, against Pillow. The table is applied to random rows in numpy with the kernel's
integer formula - out = clamp(((1 << 21) + sum px * kk) >> 22, 0, 255) in int32 - and must give Pillow's one-axis
Image.resize of the same rows exactly. No kernel launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
from PIL import Image

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib
from orbit_dataset_amd.data.utils import RESAMPLE_FILTERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
SIZES = [(224, 84), (1080, 224), (84, 224), (53, 84), (7, 2), (64, 64)]


def coeffs(lib, n_in, n_out, filt):
    """(ksize, kk [out][ksize] int32, xmin [out], count [out]) by the two-call protocol: sizes with NULL, then the table"""
    ksize = ctypes.c_int(0)
    assert lib.orbit_resize_coeffs(n_in, n_out, filt, ctypes.byref(ksize), None, None, None) == 0, _lib.last_error()
    kk = np.full((n_out, ksize.value), 12345, dtype=np.int32)
    xmin, count = np.full(n_out, -1, dtype=np.int32), np.full(n_out, -1, dtype=np.int32)
    second = ctypes.c_int(0)
    assert lib.orbit_resize_coeffs(n_in, n_out, filt, ctypes.byref(second), kk.ctypes.data, xmin.ctypes.data,
                                   count.ctypes.data) == 0, _lib.last_error()
    assert second.value == ksize.value
    return ksize.value, kk, xmin, count


def apply_table(rows, kk, xmin, count):
    """rows u8 [R][in] -> u8 [R][out] with the kernel's integer formula (int32 accumulate, arithmetic shift, clamp)"""
    out = np.empty((rows.shape[0], len(xmin)), dtype=np.uint8)
    for i in range(len(xmin)):
        window = rows[:, xmin[i]:xmin[i] + count[i]].astype(np.int32)
        acc = np.int32(1 << 21) + (window * kk[i, :count[i]][None, :]).sum(axis=1, dtype=np.int32)
        out[:, i] = np.clip(acc >> 22, 0, 255)
    return out


@pytest.mark.parametrize("name", sorted(RESAMPLE_FILTERS))
@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_table_applied_in_integers_equals_pillow(lib, name, n_in, n_out):
    ksize, kk, xmin, count = coeffs(lib, n_in, n_out, RESAMPLE_FILTERS[name])
    assert ksize == 2 * math.ceil(SUPPORT[name] * max(n_in / n_out, 1.0)) + 1
    assert (xmin >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (xmin + count <= n_in).all()
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + count) >= 0).all()  # the launcher's tile spans rely on both
    for i in range(n_out):
        assert not kk[i, count[i]:].any()  # zero behind the window
    rng = np.random.default_rng(n_in * 1000 + n_out)
    rows = np.concatenate([rng.integers(0, 256, size=(6, n_in), dtype=np.uint8),
                           rng.integers(0, 2, size=(6, n_in), dtype=np.uint8) * 255])  # noise, and 0 / 255 extremes: overshoot
    want_h = np.asarray(Image.fromarray(rows).resize((n_out, rows.shape[0]), PIL_FILTERS[name]))
    assert np.array_equal(apply_table(rows, kk, xmin, count), want_h)
    # the same table serves the vertical pass
    cols = np.ascontiguousarray(rows.T)
    want_v = np.asarray(Image.fromarray(cols).resize((cols.shape[1], n_out), PIL_FILTERS[name]))
    assert np.array_equal(apply_table(rows, kk, xmin, count).T, want_v)


def test_bad_arguments_return_an_error_with_a_message(lib):
    k = ctypes.c_int(0)
    for n_in, n_out, filt, word in ((0, 8, 2, "sizes"), (8, 0, 2, "sizes"), (-3, 8, 0, "sizes"), (8, 8, 3, "filter"),
                                    (8, 8, -1, "filter"), (1 << 20, 8, 2, "limit")):
        assert lib.orbit_resize_coeffs(n_in, n_out, filt, ctypes.byref(k), None, None, None) == -1
        assert word in _lib.last_error(), _lib.last_error()
    assert lib.orbit_resize_coeffs(8, 8, 2, None, None, None, None) == -1 and "ksize" in _lib.last_error()
    kk = np.zeros((4, 16), dtype=np.int32)
    assert lib.orbit_resize_coeffs(8, 4, 2, ctypes.byref(k), kk.ctypes.data, None, None) == -1 and "xmin" in _lib.last_error()


def test_entry_points_are_declared_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "orbit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in (("orbit_frames_resize_from_uint8", 12), ("orbit_resize_coeffs", 7)):
        assert hasattr(lib, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, code)
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
    for name, value in RESAMPLE_FILTERS.items():
        assert re.search(r"#define\s+ORBIT_RESIZE_%s\s+%d\b" % (name.upper(), value), header)


def test_null_and_bad_arguments_of_the_launcher_are_refused_before_the_gpu(lib):
    """argument checks come first: no device is touched (this runs on a host without one)"""
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    P = ctypes.c_void_p
    assert lib.orbit_frames_resize_from_uint8(None, 1, 1, 8, 8, 4, 4, 2, f3, f3, P(8), None) == -1
    assert lib.orbit_frames_resize_from_uint8(P(8), 1, 1, 8, 8, 4, 0, 2, f3, f3, P(8), None) == -1
    assert lib.orbit_frames_resize_from_uint8(P(8), 1, 1, 8, 8, 4, 4, 7, f3, f3, P(8), None) == -1
    assert "filter" in _lib.last_error()
    # a 4000 -> 4 row lanczos window is 6001 rows wide: more than a tile holds
    assert lib.orbit_frames_resize_from_uint8(P(8), 1, 1, 4000, 8, 4, 8, 2, f3, f3, P(8), None) == -1
    assert "window" in _lib.last_error()


def test_resample_flag_and_python_arguments():
    import inspect
    from orbit_dataset_amd import learner
    from orbit_dataset_amd.data import pipeline, utils
    p = learner.build_parser()
    assert p.parse_args([]).resample == "lanczos"
    for name in ("lanczos", "bicubic", "bilinear"):
        assert p.parse_args(["--resample", name]).resample == name
    with pytest.raises(SystemExit):
        p.parse_args(["--resample", "nearest"])
    sig = inspect.signature(utils.frames_from_uint8).parameters
    assert sig["size"].default is None and sig["resample"].default == "lanczos"
    sig = inspect.signature(pipeline.TaskPrefetcher.__init__).parameters
    assert sig["frame_size"].default is None and sig["resample"].default == "lanczos"
    assert utils.output_size(None, 5, 7) == (5, 7) and utils.output_size(9, 5, 7) == (9, 9) and utils.output_size((3, 4), 5, 7) == (3, 4)
    with pytest.raises(ValueError, match="nearest"):
        utils.resample_filter("nearest")
