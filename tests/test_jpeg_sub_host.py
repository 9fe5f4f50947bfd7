"""The subsequence-parallel entropy decode on the CPU, no GPU: tools/jpeg_sub_host_check.cpp runs the functions of
csrc/jpeg_core.h that jpeg_entropy_sub_kernel of csrc/jpeg.hip calls for a frame without restart markers - guessed entries,
Jacobi rounds of jpeg_sub_walk with the lanes emulated in order, exclusive scan, checks, write pass in descending order, the
serial walk again when a check fails - next to the serial walk, built with AddressSanitizer + UndefinedBehaviorSanitizer and
run as its own process. Every case runs at S = 4, 16 and 128 and at an S larger than its segment. On valid files the form
taken is the rule's, 1 <= rounds <= N, the coefficients equal the serial walk's and the pixels equal Pillow's exactly
(libjpeg's decode is integer arithmetic: there is no tolerance to choose); on damaged files status and coefficients are the
serial walk's. The argument checks of orbit_op_jpeg_entropy_sub come first in the call and are tested without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

from jpeg_sub_cases import (PARALLEL, ROOT, SERIAL, SIZES, SUB, SUB_MAX, SUB_REWALKED, build_sub_host_check, cases, damaged,
                            ecs_bytes, ecs_start, mcus, pillow_rgb, rule, run_sub_host_check)


@pytest.fixture(scope="module")
def sub_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_sub_host_check"))
    return build_sub_host_check(out), out


def test_case_list_is_what_it_says():
    cs = cases()
    for name, (data, H, W) in cs.items():
        assert data is not None, name
        assert pillow_rgb(data).shape == (H, W, 3), name
        has_restart = any(data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7 for i in range(ecs_start(data), len(data) - 1))
        assert has_restart == (name == "restart"), name
        assert ecs_bytes(data) < SIZES[-1]
    data = cs["stuffed_edge"][0]
    s = ecs_start(data)
    assert any(data[i] == 0 and data[i - 1] == 0xFF for i in range(s + 16, len(data) - 2, 16))
    assert rule(cs["wide"][0], 16)[1] > 256  # more subsequences than threads of the block
    assert rule(cs["wide"][0], 4) == (SERIAL, 0) and ecs_bytes(cs["wide"][0]) > 4 * SUB_MAX  # more than the table holds
    # the production rule takes both ways: 68 MCUs against 12, and 64 MCUs of too few bytes
    assert mcus(cs["wide"][0]) == 68 and mcus(cs["420_noise"][0]) == 12 and mcus(cs["flat"][0]) == 16 and mcus(cs["gray"][0]) == 9
    assert rule(cs["wide"][0], 0)[0] == SUB and rule(cs["420_noise"][0], 0)[0] == SERIAL and rule(cs["flat"][0], 0)[0] == SERIAL


@pytest.mark.parametrize("sub_bytes", SIZES + (0,))
@pytest.mark.parametrize("name", sorted(cases()))
def test_valid_files_take_their_form_and_equal_pillow(sub_check, name, sub_bytes):
    exe, work = sub_check
    data, H, W = cases()[name]
    rc, res, pixels, err = run_sub_host_check(exe, data, work, sub_bytes)
    assert rc == 0 and err == "", err
    assert res["parse"] == 0 and (res["width"], res["height"]) == (W, H)
    taken, n = rule(data, sub_bytes, name == "restart")
    assert res["taken"] == taken and res["n"] == n, res
    assert res["serial"] == 0 and res["sub"] == 0 and res["idct"] == 0, res
    assert res["equal"] == 1
    if taken == SUB:
        assert 1 <= res["rounds"] <= n and res["decodes"] >= n, res
    else:
        assert res["rounds"] == 0
    if sub_bytes == SIZES[-1]:
        assert taken in (SERIAL, PARALLEL)
    assert np.array_equal(pixels, pillow_rgb(data))


def test_the_round_bound_is_reached(sub_check):
    """a single MCU never lets a walker from a guessed state fall into step: every entry waits for the one before it"""
    exe, work = sub_check
    rc, res, _, _ = run_sub_host_check(exe, cases()["one_mcu_8"][0], work, 4)
    assert rc == 0 and res["taken"] == SUB and res["rounds"] == res["n"] > 2, res


@pytest.mark.parametrize("sub_bytes", (4, 16, 128, 0))
@pytest.mark.parametrize("name", ["420_noise", "444", "wide"])
def test_damaged_files_have_the_serial_walks_status(sub_check, name, sub_bytes):
    exe, work = sub_check
    for variant, data in damaged(cases()[name][0]).items():
        rc, res, pixels, err = run_sub_host_check(exe, data, work, sub_bytes)
        assert rc == 0 and err == "", (variant, err)
        assert res["parse"] == 0, variant
        assert res["sub"] == res["serial"], (variant, res)
        if res["serial"] == 0:  # (an inverted byte may leave a well-formed stream)
            assert res["equal"] == 1, (variant, res)
        else:
            assert res["taken"] in (SERIAL, SUB_REWALKED) and pixels is None, (variant, res)
        if variant == "cut50":
            assert res["serial"] > 0


def test_entry_point_is_declared_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "orbit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(lib, "orbit_op_jpeg_entropy_sub") and "orbit_op_jpeg_entropy_sub" in _lib.EXPORTS
    assert re.search(r"\bint\s+orbit_op_jpeg_entropy_sub\s*\(", code)
    assert len(_lib._SIGNATURES["orbit_op_jpeg_entropy_sub"][1]) == 13
    assert len(_lib._SIGNATURES["orbit_op_jpeg_entropy"][1]) == 12
    core = open(os.path.join(ROOT, "orbit-dataset_amd", "csrc", "jpeg_core.h")).read()
    assert re.search(r"#define\s+JPEG_SUB_MAX\s+%d\b" % _lib.JPEG_SUB_MAX, core)
    assert _lib.JPEG_SUB_MAX == SUB_MAX


def test_bad_arguments_of_the_operator_are_refused_before_the_gpu(lib):
    """argument checks come first: no device is touched (this runs on a host without one)"""
    P = ctypes.c_void_p
    H, W = 24, 40
    per_frame = 3 * 6 * 4 * 64 * 2  # 3 planes of (2 * ceil(40 / 16)) x (2 * ceil(24 / 16)) blocks of 64 int16
    ok = dict(arena=P(64), arena_bytes=64, descs=P(64), B=2, H=H, W=W, sub_bytes=0, coef=P(64), coef_bytes=2 * per_frame, status=P(64),
              taken=P(64), rounds=P(64), stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.orbit_op_jpeg_entropy_sub(a["arena"], a["arena_bytes"], a["descs"], a["B"], a["H"], a["W"], a["sub_bytes"], a["coef"],
                                             a["coef_bytes"], a["status"], a["taken"], a["rounds"], a["stream"])

    for key in ("arena", "descs", "coef", "status", "taken", "rounds"):
        assert call(**{key: None}) == -1 and "null" in _lib.last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == -1 and "sizes" in _lib.last_error()
    assert call(H=1 << 20) == -1 and "limit" in _lib.last_error()
    for sub_bytes in (1, 2, 3, -1, -128):
        assert call(sub_bytes=sub_bytes) == -1 and "sub_bytes" in _lib.last_error()
    assert call(arena_bytes=0) == -1 and "arena" in _lib.last_error()
    assert call(coef=P(72)) == -1 and "aligned" in _lib.last_error()
    assert call(coef_bytes=2 * per_frame - 1) == -1 and "coef_out" in _lib.last_error()
    assert call(B=3) == -1 and "coef_out" in _lib.last_error()
    assert call(H=33, W=40) == -1 and "coef_out" in _lib.last_error()  # a taller frame needs more blocks
