"""The entropy kernel of csrc/jpeg.hip on restart-marked files: one lane per restart interval. orbit_op_jpeg_entropy with
form 1 must take the form the case list names (`taken`) and write the coefficient planes form 0 - the serial walk - writes,
torch.equal; orbit_frames_from_jpeg must give Pillow's pixels, np.array_equal. Every comparison is exact: libjpeg's decode
path is integer arithmetic, restated in csrc/jpeg_core.h, so there is no tolerance to choose. Damaged files have the
serial walk's status whichever form was tried, and never `taken` 1. tests/test_jpeg_par_host.py runs the same functions
on the same files under the sanitizers on the CPU."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd.data import pipeline  # noqa: E402

from jpeg_par_cases import (PARALLEL, SERIAL, _encode_kw, cases, content, damaged_sources, damaged_variants, device_decode,  # noqa: E402
                            device_entropy, marker_free, misplaced_marker_variants, pillow_rgb)

CASES = sorted(cases())


@pytest.mark.parametrize("name", CASES)
def test_entropy_operator_takes_the_form_and_equals_the_serial_walk(lib, device, name):
    data, H, W, _, form_taken = cases()[name]
    assert data is not None
    files = [data, marker_free(H, W), data]
    serial, st0, taken0 = device_entropy(lib, device, files, H, W, 0)
    par, st1, taken1 = device_entropy(lib, device, files, H, W, 1)
    assert st0 == [0, 0, 0] and taken0 == [SERIAL] * 3
    assert st1 == [0, 0, 0] and taken1 == [form_taken, SERIAL, form_taken]
    assert torch.equal(par, serial)
    assert int(serial[0].ne(0).sum()) > 0 and torch.equal(serial[0], serial[2])


@pytest.mark.parametrize("name", CASES)
def test_frames_equal_pillow(lib, device, name):
    data, H, W, _, _ = cases()[name]
    files = [data, marker_free(H, W), data]
    want = [pillow_rgb(f) for f in files]
    one = lib.orbit_jpeg_workspace_bytes(1, H, W)
    for ws in (None, one + 64):  # the whole batch in one launch; three chunks of one frame
        got, status = device_decode(lib, device, files, H, W, workspace_bytes=ws)
        assert status == [0, 0, 0]
        for i in range(3):
            assert np.array_equal(got[i], want[i]), "frame %d of case %s differs from Pillow" % (i, name)


def _damaged():
    out = []
    for name, good in damaged_sources().items():
        v = damaged_variants(good)
        out += [(name + "-" + k, good, v[k]) for k in ("cut50", "flip3")]
    c = cases()["c"][0]
    out += [("c-" + k, c, v) for k, v in sorted(misplaced_marker_variants(c).items())]
    d = cases()["d"][0]
    out.append(("d-no_restart", d, damaged_variants(d)["no_restart"]))
    return out


@pytest.mark.parametrize("label,good,bad", _damaged(), ids=[x[0] for x in _damaged()])
def test_damaged_files_have_the_serial_status_and_leave_their_neighbours_exact(lib, device, label, good, bad):
    H, W = pillow_rgb(good).shape[:2]
    files = [good, bad, marker_free(H, W), bad, good]
    serial, st0, _ = device_entropy(lib, device, files, H, W, 0)
    par, st1, taken = device_entropy(lib, device, files, H, W, 1)
    assert st1 == st0, (st0, st1)
    assert [st0[i] for i in (0, 2, 4)] == [0, 0, 0] and [taken[i] for i in (0, 2, 4)] == [PARALLEL, SERIAL, PARALLEL]
    assert all(t != PARALLEL for t, s in zip(taken, st1) if s != 0), (taken, st1)
    if not label.endswith("flip3"):  # (an inverted byte may leave a well-formed stream; the others cannot be decoded)
        assert st0[1] > 0 and st0[3] > 0
    assert torch.equal(par, serial)  # a damaged frame's coefficients too: they are the serial walk's up to where it stopped
    got, status = device_decode(lib, device, files, H, W)
    assert status == st1
    for i in (0, 2, 4):
        assert np.array_equal(got[i], pillow_rgb(files[i]))


def test_pipeline_decodes_a_restart_marked_tree_on_the_device(lib, device, tmp_path):
    H, W = 48, 56
    paths, files = [], []
    for v in range(2):
        os.makedirs(str(tmp_path / ("video%d" % v)))
        for k in range(3):
            files.append(_encode_kw(content("noise" if k else "smooth", H, W, 10 * v + k), "RGB", restart_marker_rows=1))
            paths.append(str(tmp_path / ("video%d" % v) / ("%05d.jpg" % k)))
            with open(paths[-1], "wb") as f:
                f.write(files[-1])
    stats = {}
    got = pipeline.decode_frames_device(paths, device, stats=stats)
    assert stats["fallback_frames"] == 0 and stats["status"] == [0] * 6 and got.shape == (6, H, W, 3) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), pipeline.decode_frames(paths))
    _, status, taken = device_entropy(lib, device, files, H, W, 1)
    assert status == [0] * 6 and taken == [PARALLEL] * 6  # 3 MCU rows of 4:2:0 each
