"""CPU side of tests/test_gpu_se_path.py: what that file assumes about its own cases and references, checked without a GPU.

  * orbit_op_dwconv2d_plan (host only) reports, for every depthwise case, the kernel form the case is named after and the row
    chunking it lists - after the fallback of an LDS patch that cannot be laid out, under the case's option triple;
  * the one-sign inputs keep every reference output far enough from 0 that one dropped or doubled output breaks the summation
    bound of a pooling partial - shown on the reference, and by feeding the partial check such a partial;
  * the reference gates of every squeeze-excite case are unsaturated."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib
import test_gpu_se_path as T

DW_IDS = [c[0] for c in T.DW_CASES]


@pytest.mark.parametrize("name,B,C,K,stride,H,W,opts,form,rows", T.DW_CASES, ids=DW_IDS)
def test_plan_query_names_the_form_and_the_chunks(lib, name, B, C, K, stride, H, W, opts, form, rows):
    Ho, Wo = T.same_pad(H, K, stride)[0], T.same_pad(W, K, stride)[0]
    before = [lib.orbit_get_option(k) for k in (b"dw_window", b"dw_lds", b"dw_pipe")]
    with T.options(lib, dw_window=opts[0], dw_lds=opts[1], dw_pipe=opts[2]):
        got_form, chunks, rpc = T.dw_plan(lib, B, C, K, stride, Ho, Wo)
    assert [lib.orbit_get_option(k) for k in (b"dw_window", b"dw_lds", b"dw_pipe")] == before
    assert got_form == form
    assert T.chunk_rows(Ho, rpc) == rows and chunks == len(rows) and sum(rows) == Ho


def test_cases_cover_what_they_are_meant_to():
    cases = T.DW_CASES
    assert {(c[3], c[4]) for c in cases} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    assert {c[8] for c in cases if c[7] == (1, 1, 1) and not c[0].startswith("lds_unfit")} == {T.STREAM, T.PIPE, T.WINDOW, T.LDS}
    assert {c[8] for c in cases if c[7] != (1, 1, 1)} == {T.STREAM, T.PIPE, T.WINDOW, T.LDS}
    assert {c[1] for c in cases} == {1, 3}
    assert {144, 240, 1152, 32, 40} <= {c[2] for c in cases}
    out = [(T.same_pad(c[5], c[3], c[4]), T.same_pad(c[6], c[3], c[4])) for c in cases]
    assert {15, 17, 57, 13} <= {h[0] for h, _ in out}
    assert any(w[0] % 4 != 0 for _, w in out) and all(h[0] != w[0] for h, w in out)  # ragged column groups; no square map
    assert all(h[2] != w[2] for c, (h, w) in zip(cases, out) if c[4] == 2)  # stride 2: pad_top != pad_left


def test_plan_query_refuses_bad_arguments(lib):
    v = ctypes.c_int(0)
    r = ctypes.byref(v)
    assert lib.orbit_op_dwconv2d_plan(1, 32, 3, 1, 8, 8, 0, None, r, r) != 0
    assert lib.orbit_op_dwconv2d_plan(1, 30, 3, 1, 8, 8, 0, r, r, r) != 0  # C % 4
    assert lib.orbit_op_dwconv2d_plan(1, 32, 4, 1, 8, 8, 0, r, r, r) != 0  # K
    assert lib.orbit_op_dwconv2d_plan(1, 32, 3, 3, 8, 8, 0, r, r, r) != 0  # stride
    assert "op_dwconv2d_plan" in _lib.last_error()


@pytest.mark.parametrize("name,B,C,K,stride,H,W,opts,form,rows", T.DW_CASES, ids=DW_IDS)
def test_one_sign_outputs_stay_away_from_zero(name, B, C, K, stride, H, W, opts, form, rows):
    x, w, scale, shift = T.dw_inputs("one_sign", B, C, K, H, W, seed=C + 7 * K + stride)
    y64 = T.dw_ref(x, w, scale, shift, K, stride, torch.float64)
    lo, need = T.one_sign_margin(y64, rows, y64.shape[3])
    assert lo > need, (lo, need)


@pytest.mark.parametrize("pick", ["lds_rule_k3s1_c1152_13x9", "window_rule_k3s1_c32_57x6", "stream_rule_k3s2_c240_34x13"])
def test_partial_check_catches_one_dropped_or_doubled_output(pick):
    """The partial check on stand-in kernel results: fp32 sums of the fp32 reference outputs pass; the same sums with the
    SMALLEST output of one chunk dropped, or added twice, do not (lds_rule_k3s1_c1152_13x9 has the largest chunk, 117 outputs)."""
    name, B, C, K, stride, H, W, opts, form, rows = next(c for c in T.DW_CASES if c[0] == pick)
    x, w, scale, shift = T.dw_inputs("one_sign", B, C, K, H, W, seed=C + 7 * K + stride)
    y = T.nhwc(T.dw_ref(x, w, scale, shift, K, stride, torch.float64)).float()
    starts = [sum(rows[:k]) for k in range(len(rows))]
    partial = torch.stack([y[:, r0:r0 + nr].sum((1, 2)) for r0, nr in zip(starts, rows)], 1)  # [B][chunks][C], fp32 sums
    T.check_partials(pick, y, partial, rows)
    k = rows.index(max(rows))
    blk = y[0, starts[k]:starts[k] + rows[k], :, 5]
    for sign in (-1.0, 1.0):
        bad = partial.clone()
        bad[0, k, 5] += sign * blk.min()
        with pytest.raises(AssertionError):
            T.check_partials(pick, y, bad, rows)


@pytest.mark.parametrize("C,R,chunks", T.SE_CASES)
def test_synthetic_gates_are_unsaturated(C, R, chunks):
    hw = T.se_hw(chunks)
    t = T.se_inputs(3, C, R, chunks, hw, seed=C + chunks)
    _, g64 = T.se_ref(t["partial"], hw, t["w1"], t["b1"], t["w2"], t["b2"], torch.float64)
    assert T.gates_unsaturated(g64) and all(T.gates_unsaturated(g64[b:b + 1]) for b in range(3))
