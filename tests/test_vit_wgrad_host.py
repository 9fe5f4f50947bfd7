"""Host-side checks of the native ViT weight gradients (--learn_extractor): learner flags, the C-ABI symbols, the flat gradient
buffer's layout, workspace accounting and the argument validation of the new entry points (host pointers: every refusal comes
before any launch). No GPU."""
import ctypes
import os
import re

import pytest

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("orbit_vit_grad_floats", "orbit_vit_param_offset", "orbit_vit_backward_params_workspace_bytes",
       "orbit_vit_backward_params", "orbit_op_vit_linear_wgrad", "orbit_op_vit_linear_wgrad_workspace_floats",
       "orbit_op_vit_patch_embed_bwd")
VITS = (("vit_s_32", 384), ("vit_b_32", 768), ("vit_b_32_clip", 768))


def test_new_symbols_in_header_and_exports(lib):
    src = open(os.path.join(ROOT, "include", "orbit_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n + " is not declared in include/orbit_hip.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n


def test_attribute_defaults_off():
    from orbit_dataset_amd.model.feature_extractors import VisionTransformer
    assert VisionTransformer.native_weight_backward is False
    assert VisionTransformer.native_backward is False


def test_learner_flags_with_the_second_opt_in():
    from orbit_dataset_amd.learner import build_multistep_parser, build_parser, verify_args
    p, m = build_parser(), build_multistep_parser()
    assert p.parse_args([]).vit_native_weight_backward is False and m.parse_args([]).vit_native_weight_backward is False
    for name, _ in VITS:
        base = ["--feature_extractor", name]
        new = base + ["--vit_native_weight_backward"]
        admitted = (["--mode", "train", "--learn_extractor"], ["--mode", "train_test", "--learn_extractor"],
                    ["--mode", "train", "--learn_extractor", "--with_lite"],
                    ["--mode", "train", "--learn_extractor", "--adapt_features"],
                    ["--mode", "train_test", "--learn_extractor", "--adapt_features", "--with_lite"],
                    # and everything the first opt-in admits
                    ["--mode", "train", "--adapt_features"], ["--mode", "train_test", "--adapt_features", "--with_lite"],
                    ["--mode", "test", "--with_lite"], ["--mode", "test"])
        for ok in admitted:
            verify_args(p.parse_args(new + ok))
            verify_args(p.parse_args(new + ["--vit_native_backward"] + ok))
        verify_args(m.parse_args(new + ["--learn_extractor"]))
        verify_args(m.parse_args(new + ["--adapt_features", "--learn_extractor"]))
        verify_args(m.parse_args(new + ["--adapt_features"]))
        with pytest.raises(SystemExit):  # the reference's own rule still holds
            verify_args(p.parse_args(new + ["--mode", "train"]))
        with pytest.raises(SystemExit):
            verify_args(p.parse_args(new + ["--frame_size", "84"]))
        # the same command lines without the new flag: the old messages
        for line in (["--mode", "train", "--learn_extractor"], ["--mode", "train", "--learn_extractor", "--with_lite"],
                     ["--mode", "train", "--learn_extractor", "--adapt_features"]):
            with pytest.raises(SystemExit, match="inference-only"):
                verify_args(p.parse_args(base + line))
            with pytest.raises(SystemExit, match="--vit_native_backward gives FiLM gradients through a frozen"):
                verify_args(p.parse_args(base + ["--vit_native_backward"] + line))
        with pytest.raises(SystemExit, match="inference-only"):
            verify_args(m.parse_args(base + ["--learn_extractor"]))
        with pytest.raises(SystemExit, match="weight gradients through a ViT\\) is not built"):
            verify_args(m.parse_args(base + ["--vit_native_backward", "--adapt_features", "--learn_extractor"]))
    # accepted and ignored for the other extractors
    verify_args(p.parse_args(["--feature_extractor", "resnet18", "--vit_native_weight_backward", "--mode", "train",
                              "--learn_extractor"]))
    verify_args(p.parse_args(["--feature_extractor", "efficientnet_b0", "--vit_native_weight_backward", "--mode", "test"]))


def _vit(lib, name):
    h = ctypes.c_void_p()
    assert lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(h)) == 0, _lib.last_error()
    return h


@pytest.mark.parametrize("name,D", VITS)
def test_gradient_buffer_layout(lib, name, D):
    h = _vit(lib, name)
    try:
        n = lib.orbit_vit_num_params(h)
        total = lib.orbit_vit_grad_floats(h)
        offs = [lib.orbit_vit_param_offset(h, i) for i in range(n)]
        numel = [lib.orbit_vit_param_numel(h, i) for i in range(n)]
        assert n == (150 if name != "vit_b_32_clip" else 151) and offs[0] == 0
        assert all(o % 64 == 0 for o in offs), "tensors are not 256-byte aligned"
        assert all(a + k <= b for a, k, b in zip(offs, numel, offs[1:])), "ascending, non-overlapping"
        assert all(o + k <= total for o, k in zip(offs, numel))
        assert total >= sum(numel) and total < sum(numel) + 64 * n
        assert lib.orbit_vit_param_offset(h, -1) == 0 and lib.orbit_vit_param_offset(h, n) == 0
        assert lib.orbit_vit_grad_floats(None) == 0
    finally:
        lib.orbit_vit_destroy(h)


@pytest.mark.parametrize("name,D", VITS)
def test_workspace_bytes(lib, name, D):
    h = _vit(lib, name)
    try:
        fn = lib.orbit_vit_backward_params_workspace_bytes
        assert [fn(h, B) for B in (-1, 0, 8193)] == [0, 0, 0] and fn(None, 1) == 0
        batches = (1, 2, 3, 4, 5, 10, 11, 20, 21, 41, 67, 68, 82, 83, 8192)  # (the split count changes inside this list)
        sizes = [fn(h, B) for B in batches]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert all(s % 256 == 0 for s in sizes)
        for B, s in zip(batches, sizes):
            # one D-wide buffer more than the frozen backward, plus the partial tiles of the split weight-gradient GEMMs
            assert s >= lib.orbit_vit_backward_workspace_bytes(h, B) + 4 * 50 * B * D
        # the frozen backward's own accounting is untouched (tests/test_vit_train_host.py pins it)
    finally:
        lib.orbit_vit_destroy(h)


def test_wgrad_workspace_floats_rule(lib):
    fn = lib.orbit_op_vit_linear_wgrad_workspace_floats
    assert fn(0, 128, 32) == 0 and fn(1, 100, 32) == 0 and fn(1, 128, 33) == 0 and fn(50 * 8192 + 1, 128, 32) == 0
    # one split (no workspace) up to 224 rows, then a doubling at 225, 481, 993 and 2017 rows while the grid stays <= 512 blocks
    for N, K, cap in ((128, 32, 512), (1152, 384, 16), (384, 1536, 8), (1536, 384, 8)):
        for M, s in ((1, 1), (224, 1), (225, 2), (480, 2), (481, 4), (992, 4), (993, 8), (2016, 8), (2017, 16), (3350, 16)):
            s = min(s, cap)
            assert fn(M, N, K) == (s * (N * K + N) if s > 1 else 0), (M, N, K)


def test_entry_points_refuse_before_any_launch(lib):
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 256
    p = ctypes.c_void_p(base)
    off4 = ctypes.c_void_p(base + 4)   # 4-byte but not 16-byte aligned
    off2 = ctypes.c_void_p(base + 2)   # not 4-byte aligned
    off16 = ctypes.c_void_p(base + 16)  # 16-byte but not 256-byte aligned
    big = 1 << 40

    def refused(rc, text):
        assert rc != 0 and text in _lib.last_error(), (rc, _lib.last_error())

    wg = lib.orbit_op_vit_linear_wgrad
    refused(wg(None, p, p, p, 1, 128, 32, 0, p, big, None), "null pointer")
    refused(wg(p, None, p, p, 1, 128, 32, 0, p, big, None), "null pointer")
    refused(wg(p, p, None, p, 1, 128, 32, 0, p, big, None), "null pointer")
    refused(wg(p, p, p, None, 225, 128, 32, 0, None, big, None), "null pointer")  # two splits need the workspace
    refused(wg(p, p, p, p, 0, 128, 32, 0, p, big, None), "bad shape")
    refused(wg(p, p, p, p, 50 * 8192 + 1, 128, 32, 0, p, big, None), "bad shape")
    refused(wg(p, p, p, p, 1, 100, 32, 0, p, big, None), "multiple")
    refused(wg(p, p, p, p, 1, 128, 100, 0, p, big, None), "multiple")
    refused(wg(p, p, p, p, 1, 128, 32, 2, p, big, None), "gelu_on_x")
    refused(wg(p, p, p, p, 225, 128, 32, 0, p, 2 * (128 * 32 + 128) - 1, None), "workspace too small")
    for i in (0, 1, 2, 3, 8):
        args = [p, p, p, p, 225, 128, 32, 0, p, big, None]
        args[i] = off4
        refused(wg(*args), "16-byte")

    pe = lib.orbit_op_vit_patch_embed_bwd
    refused(pe(None, p, p, p, p, p, 1, 384, p, big, None), "null pointer")
    refused(pe(p, p, p, None, None, p, 1, 384, p, big, None), "null pointer")
    refused(pe(p, p, p, None, p, None, 1, 384, p, big, None), "null pointer")
    refused(pe(p, p, p, p, p, p, 0, 384, p, big, None), "batch")
    refused(pe(p, p, p, p, p, p, 8193, 384, p, big, None), "batch")
    refused(pe(p, p, p, p, p, p, 1, 512, p, big, None), "unsupported width")
    refused(pe(p, p, p, p, p, p, 5, 384, None, big, None), "null pointer")  # 245 patch rows: two splits
    refused(pe(p, p, p, p, p, p, 5, 384, p, 16, None), "workspace too small")
    refused(pe(off4, p, p, p, p, p, 1, 384, p, big, None), "16-byte")
    refused(pe(p, off4, p, p, p, p, 1, 384, p, big, None), "16-byte")
    refused(pe(p, p, p, off4, p, p, 1, 384, p, big, None), "16-byte")
    refused(pe(p, p, p, p, off2, p, 1, 384, p, big, None), "4-byte")

    bp = lib.orbit_vit_backward_params
    h = _vit(lib, "vit_s_32")
    try:  # a plan that was never finalized comes last of the argument checks that need no plan state
        refused(bp(None, p, 1, None, None, p, p, big, p, p, p, p, big, None), "null pointer")
        refused(bp(h, None, 1, None, None, p, p, big, p, p, p, p, big, None), "null pointer")
        refused(bp(h, p, 1, None, None, p, p, big, None, p, p, p, big, None), "null pointer")
        refused(bp(h, p, 1, None, None, p, None, big, p, p, p, p, big, None), "null pointer")
        refused(bp(h, p, 0, None, None, p, p, big, p, p, p, p, big, None), "batch")
        refused(bp(h, p, 8193, None, None, p, p, big, p, p, p, p, big, None), "batch")
        refused(bp(h, p, 1, None, None, p, p, big, p, p, p, p, big, None), "finalize")
        refused(bp(h, p, 1, p, None, p, p, big, p, p, p, p, big, None), "finalize")
    finally:
        lib.orbit_vit_destroy(h)
    h = _vit(lib, "vit_s_32")
    try:  # a finalized plan (host memory: orbit_vit_load copies synchronously) for the checks behind the state check
        if lib.orbit_device_count() < 1:
            return  # (the parameter pool lives on the device: without one the plan cannot be finalized)
        zeros = (ctypes.c_float * (384 * 3072))()
        for i in range(lib.orbit_vit_num_params(h)):
            assert lib.orbit_vit_load(h, lib.orbit_vit_param_name(h, i), zeros, lib.orbit_vit_param_numel(h, i)) == 0
        assert lib.orbit_vit_finalize(h, None) == 0
        need, tape = lib.orbit_vit_backward_params_workspace_bytes(h, 1), lib.orbit_vit_tape_bytes(h, 1)
        refused(bp(h, p, 1, p, None, p, p, big, p, p, p, p, big, None), "given together")
        refused(bp(h, p, 1, None, None, p, p, big, p, p, p, p, need - 1, None), "workspace too small")
        refused(bp(h, p, 1, None, None, p, p, big, p, p, p, off16, big, None), "workspace must be 256-byte aligned")
        refused(bp(h, p, 1, None, None, p, p, tape - 1, p, p, p, p, big, None), "tape too small")
        refused(bp(h, off4, 1, None, None, p, p, big, p, p, p, p, big, None), "frames must be 16-byte aligned")
        refused(bp(h, p, 1, None, None, p, p, big, off16, p, p, p, big, None), "param_grads must be 256-byte aligned")
        refused(bp(h, p, 1, None, None, off2, p, big, p, p, p, p, big, None), "4-byte aligned")
    finally:
        lib.orbit_vit_destroy(h)
