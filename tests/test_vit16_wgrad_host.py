"""CPU-side checks of the patch-16 transformers' opt-in weight gradients (orbit_vit_enable_weight_backward,
orbit_op_vit_patch_embed_bwd_p, VisionTransformer.native_weight_backward_patch16, learner --vit16_native_weight_backward),
beside tests/test_vit16_host.py and tests/test_vit16_train_host.py, whose refusals hold for every plan, module and command line
that does not opt in. Host pointers only: every refusal comes before any launch or allocation (a launch would fault)."""
import ctypes
import os
import re

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vit_s_16", "vit_b_16", "vit_b_16_clip")
WIDTH = {"vit_s_16": 384, "vit_b_16": 768, "vit_b_16_clip": 768}
MAX_B = 2048
BIG = 1 << 40


def _create(lib, name):
    h = ctypes.c_void_p()
    assert lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(h)) == 0, _lib.last_error()
    return h


def _align_up(n, a):
    return (n + a - 1) // a * a


def _host_pointer():
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 256
    return buf, base


def test_new_symbols_in_header_and_exports(lib):
    src = open(os.path.join(ROOT, "include", "orbit_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in ("orbit_vit_enable_weight_backward", "orbit_op_vit_patch_embed_bwd_p"):
        assert re.search(r"\b%s\s*\(" % n, src), n + " is not declared in include/orbit_hip.h"
        assert n in _lib.EXPORTS and hasattr(lib, n), n


@pytest.mark.parametrize("name", NAMES)
def test_plans_that_did_not_opt_in_behave_as_before(lib, name):
    buf, base = _host_pointer()
    p = ctypes.c_void_p(base)
    h = _create(lib, name)
    try:
        # fresh: forward only
        for B in (1, 16, MAX_B):
            assert lib.orbit_vit_tape_bytes(h, B) == 0 and lib.orbit_vit_backward_params_workspace_bytes(h, B) == 0
        assert lib.orbit_vit_backward_params(h, p, 1, None, None, p, p, BIG, p, p, p, p, BIG, None) == -1
        assert name in _lib.last_error() and "inference-only" in _lib.last_error()
        # FiLM gradients only: weight gradients refused by name, workspace size 0
        assert lib.orbit_vit_enable_backward(h) == 0
        for B in (1, 16, MAX_B):
            assert lib.orbit_vit_tape_bytes(h, B) == 109 * _align_up(B * 197 * WIDTH[name] * 4, 256)
            assert lib.orbit_vit_backward_params_workspace_bytes(h, B) == 0
        assert lib.orbit_vit_backward_params(h, p, 1, None, None, p, p, BIG, p, p, p, p, BIG, None) == -1
        assert name in _lib.last_error() and "weight gradients" in _lib.last_error()
    finally:
        lib.orbit_vit_destroy(h)


@pytest.mark.parametrize("name", NAMES)
def test_opted_in_plan_sizes_and_refusals_without_a_launch(lib, name):
    buf, base = _host_pointer()
    p = ctypes.c_void_p(base)
    h = _create(lib, name)
    try:
        D = WIDTH[name]
        assert lib.orbit_vit_enable_weight_backward(h) == 0  # (implies orbit_vit_enable_backward)
        for B in (1, 16, MAX_B):
            assert lib.orbit_vit_tape_bytes(h, B) == 109 * _align_up(197 * B * D * 4, 256)
            assert lib.orbit_vit_backward_workspace_bytes(h, B) > 0
            need = lib.orbit_vit_backward_params_workspace_bytes(h, B)
            # one D-wide buffer more than the frozen backward, plus the partial tiles of the split weight-gradient GEMMs
            assert need > 0 and need % 256 == 0 and need >= lib.orbit_vit_backward_workspace_bytes(h, B) + 4 * 197 * B * D
        for B in (0, -1, MAX_B + 1):
            assert lib.orbit_vit_tape_bytes(h, B) == 0
            assert lib.orbit_vit_backward_params_workspace_bytes(h, B) == 0
        # the un-finalized plan: the entry point is reached now, and stops at the state check
        assert lib.orbit_vit_backward_params(h, p, 1, None, None, p, p, BIG, p, p, p, p, BIG, None) != 0
        assert "call orbit_vit_finalize first" in _lib.last_error()
        assert lib.orbit_vit_backward_params(h, p, MAX_B + 1, None, None, p, p, BIG, p, p, p, p, BIG, None) != 0
        assert "batch" in _lib.last_error()
        assert lib.orbit_vit_train_forward(h, p, 1, None, None, p, p, BIG, p, BIG, None) != 0
        assert "call orbit_vit_finalize first" in _lib.last_error()
    finally:
        lib.orbit_vit_destroy(h)


def test_the_switch_is_idempotent_per_plan_and_a_no_op_at_patch_32(lib):
    buf, base = _host_pointer()
    p = ctypes.c_void_p(base)
    h, s32 = _create(lib, "vit_s_16"), _create(lib, "vit_s_32")
    try:
        assert lib.orbit_vit_enable_weight_backward(h) == 0
        sizes = [lib.orbit_vit_backward_params_workspace_bytes(h, B) for B in (1, 3, 16)]
        tape = lib.orbit_vit_tape_bytes(h, 3)
        assert lib.orbit_vit_enable_weight_backward(h) == 0 and lib.orbit_vit_enable_backward(h) == 0
        assert [lib.orbit_vit_backward_params_workspace_bytes(h, B) for B in (1, 3, 16)] == sizes
        assert lib.orbit_vit_tape_bytes(h, 3) == tape == 109 * _align_up(3 * 197 * 384 * 4, 256)
        # patch 32: nothing changes
        tapes = [lib.orbit_vit_tape_bytes(s32, B) for B in (1, 16, 8192, 8193)]
        params = [lib.orbit_vit_backward_params_workspace_bytes(s32, B) for B in (1, 16, 8192, 8193)]
        assert tapes[0] == 109 * _align_up(50 * 384 * 4, 256) and tapes[3] == 0 and params[1] > 0 and params[3] == 0
        assert lib.orbit_vit_enable_weight_backward(s32) == 0
        assert [lib.orbit_vit_tape_bytes(s32, B) for B in (1, 16, 8192, 8193)] == tapes
        assert [lib.orbit_vit_backward_params_workspace_bytes(s32, B) for B in (1, 16, 8192, 8193)] == params
        assert lib.orbit_vit_enable_weight_backward(None) != 0 and "null" in _lib.last_error()
        # a second handle created afterwards: the flag is the plan's, not the library's
        fresh = _create(lib, "vit_s_16")
        try:
            assert lib.orbit_vit_tape_bytes(fresh, 3) == 0 and lib.orbit_vit_backward_params_workspace_bytes(fresh, 3) == 0
            assert lib.orbit_vit_enable_backward(fresh) == 0
            assert lib.orbit_vit_backward_params_workspace_bytes(fresh, 3) == 0
            assert lib.orbit_vit_backward_params(fresh, p, 1, None, None, p, p, BIG, p, p, p, p, BIG, None) == -1
            assert "vit_s_16" in _lib.last_error() and "weight gradients" in _lib.last_error()
        finally:
            lib.orbit_vit_destroy(fresh)
    finally:
        lib.orbit_vit_destroy(h)
        lib.orbit_vit_destroy(s32)


def test_patch_embed_bwd_p_refuses_bad_arguments_before_any_launch(lib):
    buf, base = _host_pointer()
    p, off4, off2 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)

    def refused(rc, word):
        assert rc == -1, rc
        assert word in _lib.last_error(), _lib.last_error()

    pe = lib.orbit_op_vit_patch_embed_bwd_p
    ws_floats = lib.orbit_op_vit_linear_wgrad_workspace_floats
    for patch in (0, 8, 14, 24, 64, -16):
        refused(pe(p, p, p, p, p, p, 1, 384, patch, p, BIG, None), "patch size")
    for patch, max_b in ((16, MAX_B), (32, 8192)):
        refused(pe(p, p, p, p, p, p, 1, 512, patch, p, BIG, None), "unsupported width")
        refused(pe(p, p, p, p, p, p, 0, 384, patch, p, BIG, None), "batch")
        refused(pe(p, p, p, p, p, p, max_b + 1, 384, patch, p, BIG, None), "batch")
        refused(pe(None, p, p, p, p, p, 1, 384, patch, p, BIG, None), "null pointer")
        refused(pe(p, None, p, p, p, p, 1, 384, patch, p, BIG, None), "null pointer")
        refused(pe(p, p, None, p, p, p, 1, 384, patch, p, BIG, None), "null pointer")
        refused(pe(p, p, p, p, None, p, 1, 384, patch, p, BIG, None), "null pointer")
        refused(pe(p, p, p, p, p, None, 1, 384, patch, p, BIG, None), "null pointer")
        refused(pe(off4, p, p, p, p, p, 1, 384, patch, p, BIG, None), "16-byte")
        refused(pe(p, off4, p, p, p, p, 1, 384, patch, p, BIG, None), "16-byte")
        refused(pe(p, p, off4, p, p, p, 1, 384, patch, p, BIG, None), "16-byte")
        refused(pe(p, p, p, off4, p, p, 1, 384, patch, p, BIG, None), "16-byte")
        refused(pe(p, p, p, p, off2, p, 1, 384, patch, p, BIG, None), "4-byte")
        refused(pe(p, p, p, p, p, off2, 1, 384, patch, p, BIG, None), "4-byte")
    refused(pe(p, p, p, p, p, p, MAX_B + 1, 768, 16, p, BIG, None), "batch")   # (2049 frames are fine at patch 32 only)
    # the workspace: 392 patch rows at patch 16 are two splits (B = 1 is one split and needs none)
    need = ws_floats(196 * 2, 384, 768)
    assert need == 2 * (384 * 768 + 384) and ws_floats(196, 384, 768) == 0
    refused(pe(p, p, p, p, p, p, 2, 384, 16, None, BIG, None), "null pointer")
    refused(pe(p, p, p, p, p, p, 2, 384, 16, p, need - 1, None), "workspace too small")
    refused(pe(p, p, p, p, p, p, 2, 384, 16, off4, BIG, None), "16-byte")
    need32 = ws_floats(49 * 5, 384, 3072)
    assert need32 > 0
    refused(pe(p, p, p, p, p, p, 5, 384, 32, p, need32 - 1, None), "workspace too small")
    # the patch-32 call forwards to it
    refused(lib.orbit_op_vit_patch_embed_bwd(p, p, p, p, p, p, 8193, 384, p, BIG, None), "batch")
    refused(lib.orbit_op_vit_patch_embed_bwd(p, p, p, p, p, p, 5, 384, p, need32 - 1, None), "workspace too small")


@pytest.mark.parametrize("name", NAMES)
def test_module_scope_with_the_opt_in(lib, name):
    from orbit_dataset_amd.model.feature_extractors import VisionTransformer, create_feature_extractor
    assert VisionTransformer.native_weight_backward_patch16 is False
    fe, _ = create_feature_extractor(name, with_film=False, learn_extractor=True)
    frozen, _ = create_feature_extractor(name, with_film=True, learn_extractor=False)
    # the two older refusals, without the new attribute
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe.wants_grad(None)
    fe.native_backward_patch16 = True
    assert fe._grad_scope == "film"
    with pytest.raises(NotImplementedError, match=r"first: cls_token"):
        fe.wants_grad(None)
    fe.native_backward_patch16 = False
    fe.native_weight_backward_patch16 = frozen.native_weight_backward_patch16 = True  # (implies native_backward_patch16)
    assert fe._grad_scope == "all" and frozen._grad_scope == "all"
    assert fe.wants_grad(None) is True
    with torch.no_grad():
        assert not fe.wants_grad(None)
    g = torch.ones(frozen.film_size, requires_grad=True)
    assert frozen.wants_grad((g, torch.zeros_like(g))) is True  # what the FiLM opt-in admits is admitted
    assert not frozen.wants_grad(None)
    assert not fe._plans and not frozen._plans  # nothing was built for any of this
    # the patch-32 opt-ins still say nothing about a patch-16 module
    fe.native_weight_backward_patch16 = False
    fe.native_backward = fe.native_weight_backward = True
    assert fe._grad_scope == "none"
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe.wants_grad(None)


def test_the_attribute_is_ignored_at_patch_32(lib):
    from orbit_dataset_amd.model.feature_extractors import create_feature_extractor
    fe, _ = create_feature_extractor("vit_s_32", with_film=False, learn_extractor=True)
    fe.native_weight_backward_patch16 = True
    assert fe._grad_scope == "none"
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe.wants_grad(None)
    fe.native_backward = True
    assert fe._grad_scope == "film"
    with pytest.raises(NotImplementedError, match=r"first: cls_token"):
        fe.wants_grad(None)


def test_learner_flag(lib):
    from orbit_dataset_amd.learner import FROZEN_EXTRACTORS, build_multistep_parser, build_parser, verify_args
    p, m = build_parser(), build_multistep_parser()
    assert p.parse_args([]).vit16_native_weight_backward is False and m.parse_args([]).vit16_native_weight_backward is False
    assert "--vit16_native_weight_backward" in p.format_help() and "--vit16_native_weight_backward" in m.format_help()
    flag = ["--vit16_native_weight_backward"]
    admitted = (["--mode", "train", "--learn_extractor"], ["--mode", "train_test", "--learn_extractor"],
                ["--mode", "train", "--learn_extractor", "--with_lite"],
                ["--mode", "train", "--learn_extractor", "--adapt_features"],
                ["--mode", "train_test", "--learn_extractor", "--adapt_features", "--with_lite"],
                # and everything the FiLM opt-in admits
                ["--mode", "train", "--adapt_features"], ["--mode", "train_test", "--adapt_features", "--with_lite"],
                ["--mode", "test", "--with_lite"], ["--mode", "test"])
    for name in NAMES:
        spec = FROZEN_EXTRACTORS[name]
        assert spec.weight16_flag == "vit16_native_weight_backward" and spec.film16_flag == "vit16_native_backward"
        assert spec.film_flag is None and spec.weight_flag is None and spec.frame_size == 224
        base = ["--feature_extractor", name]
        for ok in admitted:
            for also in ([], ["--vit16_native_backward"], ["--vit_native_backward", "--vit_native_weight_backward"]):
                args = p.parse_args(base + flag + also + ok)
                args.frame_norm_method = "untouched"
                verify_args(args)
                assert args.frame_norm_method == spec.frame_norm  # the frame normalisation stays forced
        verify_args(m.parse_args(base + flag + ["--learn_extractor"]))
        verify_args(m.parse_args(base + flag + ["--adapt_features", "--learn_extractor"]))
        verify_args(m.parse_args(base + flag + ["--adapt_features"]))
        verify_args(m.parse_args(base + flag))
        with pytest.raises(SystemExit, match="at least one of"):  # the reference's own rule still holds
            verify_args(p.parse_args(base + flag + ["--mode", "train"]))
        with pytest.raises(SystemExit, match="needs --frame_size 224"):
            verify_args(p.parse_args(base + flag + ["--frame_size", "84"]))
        # the same command lines without the new flag: the old messages, word for word
        for line in (["--mode", "train", "--learn_extractor"], ["--mode", "train", "--learn_extractor", "--with_lite"],
                     ["--mode", "train_test", "--learn_extractor", "--adapt_features"]):
            for old in ([], ["--vit_native_backward"], ["--vit_native_weight_backward"]):
                with pytest.raises(SystemExit) as e:
                    verify_args(p.parse_args(base + old + line))
                assert str(e.value) == ("error: --feature_extractor %s is inference-only here (no backward through a ViT): use "
                                        "--mode test without --learn_extractor / --with_lite" % name)
                with pytest.raises(SystemExit) as e:
                    verify_args(p.parse_args(base + ["--vit16_native_backward"] + old + line))
                assert str(e.value) == ("error: --vit16_native_backward gives FiLM gradients through a frozen %s only: "
                                        "--learn_extractor (weight gradients through a ViT) is not built" % name)
        with pytest.raises(SystemExit, match="inference-only"):
            verify_args(m.parse_args(base + ["--learn_extractor"]))
        with pytest.raises(SystemExit, match="weight gradients through a ViT\\) is not built"):
            verify_args(m.parse_args(base + ["--vit16_native_backward", "--adapt_features", "--learn_extractor"]))
    # elsewhere the flag changes nothing
    for name in ("vit_s_32", "vit_b_32_clip"):
        assert FROZEN_EXTRACTORS[name].weight16_flag is None
        with pytest.raises(SystemExit, match="inference-only"):
            verify_args(p.parse_args(["--feature_extractor", name, "--mode", "train", "--learn_extractor"] + flag))
        with pytest.raises(SystemExit, match="--vit_native_backward gives FiLM gradients"):
            verify_args(p.parse_args(["--feature_extractor", name, "--mode", "train", "--learn_extractor", "--vit_native_backward"]
                                     + flag))
        verify_args(p.parse_args(["--feature_extractor", name, "--mode", "train", "--learn_extractor",
                                  "--vit_native_weight_backward"] + flag))
    assert FROZEN_EXTRACTORS["efficientnet_v2_s"].weight16_flag is None
    verify_args(p.parse_args(["--feature_extractor", "efficientnet_b0", "--mode", "train", "--learn_extractor"] + flag))
    verify_args(p.parse_args(["--feature_extractor", "efficientnet_b0", "--mode", "test"] + flag))
    with pytest.raises(SystemExit, match="inference-only"):
        verify_args(p.parse_args(["--feature_extractor", "efficientnet_v2_s", "--mode", "train", "--learn_extractor"] + flag))
    with pytest.raises(SystemExit, match="--effnetv2_native_backward gives FiLM gradients"):
        verify_args(p.parse_args(["--feature_extractor", "efficientnet_v2_s", "--mode", "train", "--learn_extractor",
                                  "--effnetv2_native_backward"] + flag))


def test_one_map_from_flags_to_attributes(lib):
    from orbit_dataset_amd.learner import FROZEN_EXTRACTORS, build_parser, opted_in
    p = build_parser()
    every = p.parse_args(["--vit16_native_weight_backward", "--vit16_native_backward", "--vit_native_backward",
                          "--vit_native_weight_backward"])
    assert opted_in(every, FROZEN_EXTRACTORS["vit_b_16"]) == ("all", "vit16_native_weight_backward",
                                                              ["native_weight_backward_patch16", "native_backward_patch16"])
    assert opted_in(every, FROZEN_EXTRACTORS["vit_b_32"]) == ("all", "vit_native_weight_backward",
                                                              ["native_weight_backward", "native_backward"])
    assert opted_in(every, FROZEN_EXTRACTORS["efficientnet_v2_s"]) == ("none", None, [])
    new = p.parse_args(["--vit16_native_weight_backward"])
    assert opted_in(new, FROZEN_EXTRACTORS["vit_s_16"]) == ("all", "vit16_native_weight_backward",
                                                            ["native_weight_backward_patch16"])
    assert opted_in(new, FROZEN_EXTRACTORS["vit_s_32"]) == ("none", None, [])
    old = p.parse_args(["--vit16_native_backward"])
    assert opted_in(old, FROZEN_EXTRACTORS["vit_s_16"]) == ("film", "vit16_native_backward", ["native_backward_patch16"])
