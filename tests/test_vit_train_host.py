"""Host-side checks of the opt-in ViT FiLM backward: learner flags, the C-ABI symbols, tape / workspace accounting and the
argument validation of the operator entry points (host pointers: every refusal comes before any launch). No GPU."""
import ctypes
import os
import re

import pytest

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("orbit_vit_tape_bytes", "orbit_vit_backward_workspace_bytes", "orbit_vit_train_forward", "orbit_vit_backward",
       "orbit_op_vit_linear_dgrad", "orbit_op_vit_layernorm_bwd", "orbit_op_vit_attention_bwd")


def test_learner_flags_with_the_opt_in():
    from orbit_dataset_amd.learner import build_multistep_parser, build_parser, verify_args
    p, m = build_parser(), build_multistep_parser()
    assert p.parse_args([]).vit_native_backward is False and m.parse_args([]).vit_native_backward is False
    for name in ("vit_s_32", "vit_b_32", "vit_b_32_clip"):
        base = ["--feature_extractor", name, "--vit_native_backward"]
        for ok in (["--mode", "train", "--adapt_features"], ["--mode", "train_test", "--adapt_features", "--with_lite"],
                   ["--mode", "test", "--with_lite"], ["--mode", "test"]):
            verify_args(p.parse_args(base + ok))
        verify_args(m.parse_args(base + ["--adapt_features"]))
        for bad in (["--mode", "train", "--learn_extractor"], ["--mode", "train", "--adapt_features", "--learn_extractor"],
                    ["--learn_extractor"]):
            with pytest.raises(SystemExit, match="learn_extractor"):
                verify_args(p.parse_args(base + bad))
        with pytest.raises(SystemExit, match="learn_extractor"):
            verify_args(m.parse_args(base + ["--adapt_features", "--learn_extractor"]))
        with pytest.raises(SystemExit):  # the reference's own rule still holds
            verify_args(p.parse_args(base + ["--mode", "train"]))
        with pytest.raises(SystemExit):
            verify_args(p.parse_args(base + ["--frame_size", "84"]))
        # without the flag nothing is admitted
        with pytest.raises(SystemExit, match="inference-only"):
            verify_args(p.parse_args(["--feature_extractor", name, "--mode", "train", "--adapt_features"]))
    verify_args(p.parse_args(["--feature_extractor", "resnet18", "--vit_native_backward", "--mode", "train", "--learn_extractor"]))


def test_attribute_defaults_off():
    from orbit_dataset_amd.model.feature_extractors import VisionTransformer
    assert VisionTransformer.native_backward is False


def test_new_symbols_in_header_and_exports(lib):
    src = open(os.path.join(ROOT, "include", "orbit_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n + " is not declared in include/orbit_hip.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n


def _vit(lib, name):
    h = ctypes.c_void_p()
    assert lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(h)) == 0, _lib.last_error()
    return h


@pytest.mark.parametrize("name,D", [("vit_s_32", 384), ("vit_b_32", 768), ("vit_b_32_clip", 768)])
def test_tape_and_workspace_bytes(lib, name, D):
    h = _vit(lib, name)
    try:
        for fn in (lib.orbit_vit_tape_bytes, lib.orbit_vit_backward_workspace_bytes):
            assert [fn(h, B) for B in (-1, 0, 8193)] == [0, 0, 0]
            sizes = [fn(h, B) for B in (1, 2, 3, 67, 68, 8192)]
            assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
            assert all(s % 256 == 0 for s in sizes)
        for B in (1, 3, 67, 8192):
            md = 4 * 50 * B * D
            pad = -md % 256
            # per block the input stream, qkv, the post-attention stream and the fc1 pre-activation: 9 * 50 B * D floats; then
            # the stream entering the final norm; each of the 12 * 4 + 1 segments padded to 256 bytes
            assert lib.orbit_vit_tape_bytes(h, B) == 12 * 9 * (md + pad) + (md + pad)
            # gradient stream + one D-wide and one 4 D-wide buffer + the LayerNorm partial sums
            low = 6 * md + 4 * (-(-50 * B // 64)) * 2 * D
            assert low <= lib.orbit_vit_backward_workspace_bytes(h, B) <= low + 4 * 256
    finally:
        lib.orbit_vit_destroy(h)


def test_entry_points_refuse_before_any_launch(lib):
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 256
    p = ctypes.c_void_p(base)
    off4 = ctypes.c_void_p(base + 4)   # 4-byte but not 16-byte aligned
    off2 = ctypes.c_void_p(base + 2)   # not 4-byte aligned

    def refused(rc, text):
        assert rc != 0 and text in _lib.last_error(), (rc, _lib.last_error())

    dg = lib.orbit_op_vit_linear_dgrad
    refused(dg(p, p, p, None, None, p, 1, 384, 384, 32, None), "tile_rows")
    refused(dg(p, p, p, None, None, p, 1, 384, 384, -64, None), "tile_rows")
    refused(dg(p, p, p, None, None, p, 1, 384, 100, 0, None), "multiple")
    refused(dg(p, p, p, None, None, p, 1, 100, 384, 0, None), "multiple")
    refused(dg(p, p, p, None, None, p, 0, 384, 384, 0, None), "bad shape")
    refused(dg(off4, p, p, None, None, p, 1, 384, 384, 0, None), "16-byte")
    refused(dg(p, off4, p, None, None, p, 1, 384, 384, 0, None), "16-byte")
    refused(dg(p, p, off4, None, None, p, 1, 384, 384, 0, None), "16-byte")
    refused(dg(p, p, p, off2, None, p, 1, 384, 384, 0, None), "4-byte")
    refused(dg(p, p, p, p, p, p, 1, 384, 384, 0, None), "not both")
    refused(dg(p, p, None, None, None, p, 1, 384, 384, 0, None), "null pointer")

    ln = lib.orbit_op_vit_layernorm_bwd
    refused(ln(p, 512, p, 512, p, 1e-6, None, p, 512, 1, 512, p, p, p, 4096, None), "unsupported width")
    refused(ln(p, 384, p, 384, p, 1e-6, None, p, 384, 0, 384, p, p, p, 4096, None), "rows")
    refused(ln(p, 100, p, 384, p, 1e-6, None, p, 384, 1, 384, p, p, p, 4096, None), "strides")
    refused(ln(p, 384, p, 384, p, 1e-6, None, p, 100, 1, 384, p, p, p, 4096, None), "strides")
    refused(ln(p, 384, p, 384, p, 1e-6, p, None, 384, 1, 384, p, p, p, 4096, None), "dres without dx")
    refused(ln(p, 384, p, 384, p, 1e-6, p, p, 50 * 384, 1, 384, p, p, p, 4096, None), "contiguous rows")
    refused(ln(p, 384, p, 384, p, 1e-6, None, p, 384, 65, 384, p, p, p, 2 * 384, None), "partial buffer")
    refused(ln(off2, 384, p, 384, p, 1e-6, None, p, 384, 1, 384, p, p, p, 4096, None), "4-byte")
    refused(ln(p, 384, p, 384, p, -1.0, None, p, 384, 1, 384, p, p, p, 4096, None), "negative eps")

    at = lib.orbit_op_vit_attention_bwd
    refused(at(p, p, p, 1, 512, 8, None), "unsupported width")
    refused(at(p, p, p, 1, 384, 12, None), "heads")
    refused(at(p, p, p, 0, 384, 6, None), "batch")
    refused(at(p, off2, p, 1, 384, 6, None), "4-byte")
    refused(at(p, p, None, 1, 384, 6, None), "null pointer")

    h = _vit(lib, "vit_s_32")
    try:  # a plan that was never finalized, bad batch sizes, film vectors given singly
        refused(lib.orbit_vit_train_forward(h, p, 1, None, None, p, p, 1 << 40, p, 1 << 40, None), "finalize")
        refused(lib.orbit_vit_backward(h, 1, None, None, p, p, 1 << 40, p, p, p, 1 << 40, None), "finalize")
        refused(lib.orbit_vit_train_forward(h, p, 0, None, None, p, p, 1 << 40, p, 1 << 40, None), "batch")
        refused(lib.orbit_vit_backward(h, 8193, None, None, p, p, 1 << 40, p, p, p, 1 << 40, None), "batch")
        refused(lib.orbit_vit_backward(h, 1, None, None, p, None, 1 << 40, p, p, p, 1 << 40, None), "null pointer")
    finally:
        lib.orbit_vit_destroy(h)
