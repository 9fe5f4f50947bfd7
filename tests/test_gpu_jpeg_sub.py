"""jpeg_entropy_sub_kernel of csrc/jpeg.hip on files without restart markers: one walker per subsequence of the entropy-coded
segment. orbit_op_jpeg_entropy_sub must take the form the rule names (`taken`), in the rounds the host model of
tools/jpeg_sub_host_check.cpp takes (they depend on the file and S alone), and write the coefficient planes
orbit_op_jpeg_entropy's form 0 - the serial walk - writes, torch.equal; orbit_frames_from_jpeg must give Pillow's pixels,
np.array_equal. Every comparison is exact: libjpeg's decode path is integer arithmetic, restated in csrc/jpeg_core.h, so
there is no tolerance to choose. Damaged files have the serial walk's status and coefficients and never `taken` 3.
tests/test_jpeg_sub_host.py runs the same functions on the same files under the sanitizers on the CPU."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd.data import pipeline  # noqa: E402

from jpeg_sub_cases import (SERIAL, SIZES, SUB, _encode_kw, _flat, build_sub_host_check, cases, content, damaged, device_decode,  # noqa: E402
                            device_entropy, device_entropy_sub, other_file, pillow_rgb, rule, run_sub_host_check)

CASES = sorted(cases())


@pytest.fixture(scope="module")
def host_rounds(tmp_path_factory):
    """(file, sub_bytes) -> rounds of the host model; the program is built once, without a GPU"""
    out = str(tmp_path_factory.mktemp("jpeg_sub_host_check"))
    exe, memo = build_sub_host_check(out), {}

    def rounds(data, sub_bytes):
        if (data, sub_bytes) not in memo:
            rc, res, _, err = run_sub_host_check(exe, data, out, sub_bytes)
            assert rc == 0 and err == "", err
            memo[(data, sub_bytes)] = res["rounds"]
        return memo[(data, sub_bytes)]

    return rounds


@pytest.fixture(scope="module")
def serial_walk(lib, device):
    """files -> form 0 of orbit_op_jpeg_entropy over them, computed once per batch"""
    memo = {}

    def walk(files, H, W):
        key = tuple(files)
        if key not in memo:
            memo[key] = device_entropy(lib, device, files, H, W, 0)
        return memo[key]

    return walk


@pytest.mark.parametrize("sub_bytes", SIZES + (0,))
@pytest.mark.parametrize("name", CASES)
def test_operator_takes_the_form_and_equals_the_serial_walk(lib, device, host_rounds, serial_walk, name, sub_bytes):
    data, H, W = cases()[name]
    other = other_file(H, W)
    files = [data, other, data]
    serial, st0, taken0 = serial_walk(files, H, W)
    sub, st, taken, rounds = device_entropy_sub(lib, device, files, H, W, sub_bytes)
    assert st0 == [0, 0, 0] and taken0 == [SERIAL] * 3
    want = [rule(f, sub_bytes, name == "restart" and f is data)[0] for f in files]
    assert st == [0, 0, 0] and taken == want, (taken, want)
    assert rounds == [host_rounds(f, sub_bytes) for f in files]
    assert all((r >= 1) == (t == SUB) for r, t in zip(rounds, taken))
    assert torch.equal(sub, serial)
    assert int(serial[0].ne(0).sum()) > 0 and torch.equal(sub[0], sub[2])


@pytest.mark.parametrize("name", CASES)
def test_frames_equal_pillow(lib, device, name):
    data, H, W = cases()[name]
    files = [data, other_file(H, W), data]
    want = [pillow_rgb(f) for f in files]
    one = lib.orbit_jpeg_workspace_bytes(1, H, W)
    for ws in (None, one + 64):  # the whole batch in one launch; three chunks of one frame
        got, status = device_decode(lib, device, files, H, W, workspace_bytes=ws)
        assert status == [0, 0, 0]
        for i in range(3):
            assert np.array_equal(got[i], want[i]), "frame %d of case %s differs from Pillow" % (i, name)


def _damaged():
    out = []
    for name in ("420_noise", "444", "wide"):
        good = cases()[name][0]
        out += [(name + "-" + k, good, v) for k, v in sorted(damaged(good).items())]
    return out


@pytest.mark.parametrize("sub_bytes", (16, 0))
@pytest.mark.parametrize("label,good,bad", _damaged(), ids=[x[0] for x in _damaged()])
def test_damaged_files_have_the_serial_status_and_leave_their_neighbours_exact(lib, device, serial_walk, label, good, bad, sub_bytes):
    H, W = pillow_rgb(good).shape[:2]
    files = [good, bad, other_file(H, W), bad, good]
    serial, st0, _ = serial_walk(files, H, W)
    sub, st, taken, _ = device_entropy_sub(lib, device, files, H, W, sub_bytes)
    assert st == st0, (st0, st)
    assert [st0[i] for i in (0, 2, 4)] == [0, 0, 0] and [taken[i] for i in (0, 2, 4)] == [rule(files[i], sub_bytes)[0] for i in (0, 2, 4)]
    assert taken[0] == SUB or sub_bytes == 0  # (the production rule leaves frames of fewer than 64 MCUs serial; `wide` has 68)
    assert all(t != SUB for t, s in zip(taken, st) if s != 0), (taken, st)
    if label.endswith("cut50"):  # (an inverted byte may leave a well-formed stream; a cut one cannot be decoded)
        assert st0[1] > 0 and st0[3] > 0
    assert torch.equal(sub, serial)  # a damaged frame's coefficients too: they are the serial walk's up to where it stopped
    got, status = device_decode(lib, device, files, H, W)
    # (a stream that still decodes after an inverted byte may fail the range check of the inverse DCT, ORBIT_JPEG_ST_RANGE)
    assert all(s == e if e != 0 else s in (0, 16) for s, e in zip(status, st0)), (status, st0)
    assert [status[i] for i in (0, 2, 4)] == [0, 0, 0]
    for i in (0, 2, 4):
        assert np.array_equal(got[i], pillow_rgb(files[i]))


def test_pipeline_decodes_a_marker_free_tree_on_the_device(lib, device, tmp_path):
    H, W = 128, 120  # 64 MCUs at 4:2:0, the rule's floor: the noise and smooth frames take the form, the flat one has too few bytes
    paths, files = [], []
    for v in range(2):
        os.makedirs(str(tmp_path / ("video%d" % v)))
        for k, pixels in enumerate((content("noise", H, W, 10 * v), content("smooth", H, W), _flat(H, W))):
            files.append(_encode_kw(pixels, "RGB"))
            paths.append(str(tmp_path / ("video%d" % v) / ("%05d.jpg" % k)))
            with open(paths[-1], "wb") as f:
                f.write(files[-1])
    stats = {}
    got = pipeline.decode_frames_device(paths, device, stats=stats)
    assert stats["fallback_frames"] == 0 and stats["status"] == [0] * 6 and got.shape == (6, H, W, 3) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), pipeline.decode_frames(paths))
    _, status, taken, rounds = device_entropy_sub(lib, device, files, H, W, 0)
    want = [rule(f, 0)[0] for f in files]  # the production rule from the file sizes
    assert status == [0] * 6 and taken == want
    assert SUB in want and SERIAL in want
    assert all((r >= 1) == (t == SUB) for r, t in zip(rounds, taken))
