"""The interval-parallel entropy decode on the CPU, no GPU: tools/jpeg_par_host_check.cpp runs the functions of
csrc/jpeg_core.h that the entropy kernel of csrc/jpeg.hip calls for a restart-marked frame - marker scan in lane slices,
interval table, jpeg_walk_interval per interval in descending order, serial walk again on any status - next to the serial
walk, built with AddressSanitizer + UndefinedBehaviorSanitizer and run as its own process. On valid files the form taken is
the one the case list names, the coefficients equal the serial walk's and the pixels equal Pillow's exactly (libjpeg's decode
is integer arithmetic: there is no tolerance to choose); on damaged files status and coefficients are the serial walk's.
The argument checks of orbit_op_jpeg_entropy come first in the call and are tested without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

from jpeg_par_cases import (MAX_INTERVALS, PARALLEL, ROOT, TILE, build_par_host_check, cases, damaged_sources, damaged_variants,
                            ecs_start, misplaced_marker_variants, pillow_rgb, restart_markers, run_par_host_check)


@pytest.fixture(scope="module")
def par_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_par_host_check"))
    return build_par_host_check(out), out


def test_case_list_is_what_it_says():
    """the geometry of every case, on the host: interval counts, the wrap of the marker numbers, the tile edge of case i"""
    cs = cases()
    assert cs["i"][0] is not None, "no seed puts a restart marker's FF on the last byte of a tile"
    for name, (data, H, W, nseg, _) in cs.items():
        assert pillow_rgb(data).shape == (H, W, 3), name
        assert len(restart_markers(data)) == nseg - 1, name
    assert cs["d"][3] > 64 and cs["h"][3] > MAX_INTERVALS and cs["c444"][3] <= 64
    assert [cs["c"][0][m + 1] for m in restart_markers(cs["c"][0])][7:10] == [0xD7, 0xD0, 0xD1]
    data = cs["i"][0]
    assert any((m - ecs_start(data)) % TILE == TILE - 1 for m in restart_markers(data))
    g, first = cs["g"][0], restart_markers(cs["b"][0])[0]
    assert g[first - 1] != 0xFF and g[first:first + 3] == b"\xff\xff\xd0"


@pytest.mark.parametrize("name", sorted(cases()))
def test_valid_files_take_their_form_and_equal_pillow(par_check, name):
    exe, work = par_check
    data, H, W, nseg, taken = cases()[name]
    assert data is not None
    rc, res, pixels, err = run_par_host_check(exe, data, work)
    assert rc == 0 and err == "", err
    assert res["parse"] == 0 and (res["width"], res["height"]) == (W, H)
    assert res["nseg"] == (nseg if taken == PARALLEL else 0)
    assert res["taken"] == taken, res
    assert res["serial"] == 0 and res["parallel"] == 0 and res["idct"] == 0, res
    assert res["equal"] == 1
    assert np.array_equal(pixels, pillow_rgb(data))


def _check_damaged(exe, work, variants):
    seen = set()
    for variant, data in variants.items():
        rc, res, pixels, err = run_par_host_check(exe, data, work)
        assert rc == 0 and err == "", (variant, err)
        assert res["parse"] == 0, variant
        assert res["parallel"] == res["serial"], (variant, res)
        if res["serial"] == 0:
            assert res["equal"] == 1, (variant, res)
        else:
            assert pixels is None
        assert not (res["taken"] == 1 and res["parallel"] != 0), (variant, res)
        seen.add(res["taken"])
    return seen


@pytest.mark.parametrize("name", ["420", "444", "gray", "d"])
def test_damaged_files_have_the_serial_walks_status(par_check, name):
    """the cuts, the ten inverted bytes and the removed marker of jpeg_cases.damaged_variants"""
    exe, work = par_check
    good = cases()["d"][0] if name == "d" else damaged_sources()[name]
    rc, res, _, err = run_par_host_check(exe, good, work)
    assert rc == 0 and err == "" and (res["serial"], res["parallel"], res["taken"], res["equal"]) == (0, 0, 1, 1)
    variants = damaged_variants(good)
    seen = _check_damaged(exe, work, variants)
    # a removed marker is found by the scan (serial from the start); an inverted byte inside an interval is found by its walker
    rc, res, _, _ = run_par_host_check(exe, variants["no_restart"], work)
    assert res["taken"] == 0 and res["serial"] > 0
    assert 2 in seen


@pytest.mark.parametrize("name", ["c", "d"])
def test_misplaced_markers_are_left_to_the_serial_walk(par_check, name):
    exe, work = par_check
    variants = misplaced_marker_variants(cases()[name][0])
    assert sorted(variants) == ["doubled", "eoi", "swapped"]
    _check_damaged(exe, work, variants)
    for variant, data in variants.items():
        rc, res, pixels, err = run_par_host_check(exe, data, work)
        assert res["taken"] in (0, 2) and res["parallel"] == res["serial"] > 0 and pixels is None, (variant, res)


def test_entry_point_is_declared_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "orbit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(lib, "orbit_op_jpeg_entropy") and "orbit_op_jpeg_entropy" in _lib.EXPORTS
    assert re.search(r"\bint\s+orbit_op_jpeg_entropy\s*\(", code)
    assert len(_lib._SIGNATURES["orbit_op_jpeg_entropy"][1]) == 12
    core = open(os.path.join(ROOT, "orbit-dataset_amd", "csrc", "jpeg_core.h")).read()
    assert re.search(r"#define\s+JPEG_PAR_MAX_INTERVALS\s+%d\b" % _lib.JPEG_PAR_MAX_INTERVALS, core)
    assert _lib.JPEG_PAR_MAX_INTERVALS == MAX_INTERVALS


def test_bad_arguments_of_the_entropy_operator_are_refused_before_the_gpu(lib):
    """argument checks come first: no device is touched (this runs on a host without one)"""
    P = ctypes.c_void_p
    H, W = 24, 40
    per_frame = 3 * 6 * 4 * 64 * 2  # 3 planes of (2 * ceil(40 / 16)) x (2 * ceil(24 / 16)) blocks of 64 int16
    ok = dict(arena=P(64), arena_bytes=64, descs=P(64), B=2, H=H, W=W, form=1, coef=P(64), coef_bytes=2 * per_frame, status=P(64),
              taken=P(64), stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.orbit_op_jpeg_entropy(a["arena"], a["arena_bytes"], a["descs"], a["B"], a["H"], a["W"], a["form"], a["coef"],
                                         a["coef_bytes"], a["status"], a["taken"], a["stream"])

    for key in ("arena", "descs", "coef", "status", "taken"):
        assert call(**{key: None}) == -1 and "null" in _lib.last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == -1 and "sizes" in _lib.last_error()
    assert call(H=1 << 20) == -1 and "limit" in _lib.last_error()
    for form in (-1, 2):
        assert call(form=form) == -1 and "form" in _lib.last_error()
    assert call(arena_bytes=0) == -1 and "arena" in _lib.last_error()
    assert call(coef=P(72)) == -1 and "aligned" in _lib.last_error()
    assert call(coef_bytes=2 * per_frame - 1) == -1 and "coef_out" in _lib.last_error()
    assert call(B=3) == -1 and "coef_out" in _lib.last_error()
    assert call(H=33, W=40) == -1 and "coef_out" in _lib.last_error()  # a taller frame needs more blocks
