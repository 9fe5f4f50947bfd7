"""CPU-side checks of the patch-16 transformers' opt-in FiLM gradients (orbit_vit_enable_backward,
VisionTransformer.native_backward_patch16, learner --vit16_native_backward), beside tests/test_vit16_host.py, whose refusals hold
for every plan, module and command line that does not opt in: an enabled plan reports the patch-32 tape layout at 197 tokens and
keeps refusing weight gradients, the switch is per plan and idempotent, the operator entry point of the 197-token attention
backward refuses bad arguments before any launch, the module's gradient scope becomes "film", and the learner admits exactly the
recipes that need FiLM gradients through the frozen network."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

NAMES = ("vit_s_16", "vit_b_16", "vit_b_16_clip")
WIDTH = {"vit_s_16": 384, "vit_b_16": 768, "vit_b_16_clip": 768}
MAX_B = 2048


def _create(lib, name):
    h = ctypes.c_void_p()
    assert lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(h)) == 0, _lib.last_error()
    return h


def _align_up(n, a):
    return (n + a - 1) // a * a


@pytest.mark.parametrize("name", NAMES)
def test_enabled_plan_sizes_and_refusals_without_a_launch(lib, name):
    """Host pointers throughout: a launch would fault."""
    h = _create(lib, name)
    try:
        assert lib.orbit_vit_tape_bytes(h, 16) == 0  # (fresh: forward only)
        assert lib.orbit_vit_enable_backward(h) == 0
        D = WIDTH[name]
        for B in (1, 16, MAX_B):
            assert lib.orbit_vit_tape_bytes(h, B) == 109 * _align_up(B * 197 * D * 4, 256)
            assert lib.orbit_vit_backward_workspace_bytes(h, B) > 0
            assert lib.orbit_vit_backward_params_workspace_bytes(h, B) == 0
        for B in (0, -1, MAX_B + 1):
            assert lib.orbit_vit_tape_bytes(h, B) == 0
            assert lib.orbit_vit_backward_workspace_bytes(h, B) == 0
            assert lib.orbit_vit_backward_params_workspace_bytes(h, B) == 0
        buf = (ctypes.c_float * 64)()
        p = ctypes.c_void_p(ctypes.addressof(buf))
        assert lib.orbit_vit_backward_params(h, p, 1, None, None, p, p, 1 << 40, p, p, p, p, 1 << 40, None) == -1
        assert name in _lib.last_error() and "weight gradients" in _lib.last_error()
        # the un-finalized plan: the training entry points are reached now, and stop at the state check
        assert lib.orbit_vit_train_forward(h, p, 1, None, None, p, p, 1 << 40, p, 1 << 40, None) != 0
        assert "call orbit_vit_finalize first" in _lib.last_error()
        assert lib.orbit_vit_backward(h, 1, None, None, p, p, 1 << 40, p, p, p, 1 << 40, None) != 0
        assert "call orbit_vit_finalize first" in _lib.last_error()
    finally:
        lib.orbit_vit_destroy(h)


def test_the_switch_is_idempotent_per_plan_and_a_no_op_at_patch_32(lib):
    h = _create(lib, "vit_s_16")
    s32 = _create(lib, "vit_s_32")
    try:
        assert lib.orbit_vit_enable_backward(h) == 0 and lib.orbit_vit_enable_backward(h) == 0
        assert lib.orbit_vit_tape_bytes(h, 3) == 109 * _align_up(3 * 197 * 384 * 4, 256)
        before = [lib.orbit_vit_tape_bytes(s32, B) for B in (1, 16, 8192, 8193)]
        params = lib.orbit_vit_backward_params_workspace_bytes(s32, 16)
        assert before[0] == 109 * _align_up(50 * 384 * 4, 256) and before[3] == 0 and params > 0
        assert lib.orbit_vit_enable_backward(s32) == 0
        assert [lib.orbit_vit_tape_bytes(s32, B) for B in (1, 16, 8192, 8193)] == before
        assert lib.orbit_vit_backward_params_workspace_bytes(s32, 16) == params
        assert lib.orbit_vit_enable_backward(None) != 0 and "null" in _lib.last_error()
        # a second handle created afterwards: the flag is the plan's, not the library's
        fresh = _create(lib, "vit_s_16")
        try:
            buf = (ctypes.c_float * 64)()
            p = ctypes.c_void_p(ctypes.addressof(buf))
            assert lib.orbit_vit_tape_bytes(fresh, 3) == 0 and lib.orbit_vit_backward_workspace_bytes(fresh, 3) == 0
            assert lib.orbit_vit_train_forward(fresh, p, 1, None, None, p, p, 1 << 40, p, 1 << 40, None) == -1
            assert "vit_s_16" in _lib.last_error() and "inference-only" in _lib.last_error()
        finally:
            lib.orbit_vit_destroy(fresh)
    finally:
        lib.orbit_vit_destroy(h)
        lib.orbit_vit_destroy(s32)


def test_attention_bwd_tokens_refuses_bad_arguments_before_any_launch(lib):
    """(the pointers are host addresses: a launch would fault)"""
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, odd, odd2 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)

    def refused(rc, word):
        assert rc == -1, rc
        assert word in _lib.last_error(), _lib.last_error()

    ab = lib.orbit_op_vit_attention_bwd_tokens
    for tokens in (49, 196, 198, 0, 224):
        refused(ab(p, p, p, 1, tokens, 384, 6, None), "tokens")
    for tokens in (50, 197):
        refused(ab(p, p, p, 1, tokens, 512, 8, None), "width")
        refused(ab(p, p, p, 1, tokens, 384, 12, None), "heads")
        refused(ab(p, p, p, 1, tokens, 768, 6, None), "heads")
        refused(ab(p, p, p, 0, tokens, 384, 6, None), "batch")
        refused(ab(odd2, p, p, 1, tokens, 384, 6, None), "aligned")
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            refused(ab(*args, 1, tokens, 384, 6, None), "null")
    refused(ab(p, p, p, MAX_B + 1, 197, 384, 6, None), "batch")
    refused(ab(p, p, p, 8193, 50, 384, 6, None), "batch")
    for args in ((odd, p, p), (p, odd, p), (p, p, odd)):  # the 197-token kernel moves float4
        refused(ab(*args, 1, 197, 384, 6, None), "16-byte")
    refused(lib.orbit_op_vit_attention_bwd(p, p, p, 8193, 384, 6, None), "batch")  # (the 50-token call forwards)


@pytest.mark.parametrize("name", NAMES)
def test_module_scope_with_the_opt_in(lib, name):
    from orbit_dataset_amd.model.feature_extractors import VisionTransformer, create_feature_extractor
    assert VisionTransformer.native_backward_patch16 is False
    fe, _ = create_feature_extractor(name, pretrained=True, with_film=True, learn_extractor=False)
    fe2, _ = create_feature_extractor(name, with_film=False, learn_extractor=True)
    g = torch.ones(fe.film_size, requires_grad=True)
    film = (g, torch.zeros_like(g))
    fe.native_backward_patch16 = fe2.native_backward_patch16 = True
    assert fe._grad_scope == "film"
    assert fe.wants_grad(film) is True
    assert not fe.wants_grad(None)  # frozen, no FiLM vectors: nothing requires a gradient
    with torch.no_grad():
        assert not fe.wants_grad(film)
    with pytest.raises(NotImplementedError, match=r"first: cls_token"):  # weight gradients: refused by name
        fe2.wants_grad(None)
    assert not fe._plans and not fe2._plans  # nothing was built for any of this
    # the patch-32 opt-ins say nothing about a patch-16 module
    for net in (fe, fe2):
        net.native_backward_patch16 = False
        net.native_backward = net.native_weight_backward = True
    assert fe._grad_scope == "none"
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe.wants_grad(film)
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe2.wants_grad(None)


def test_the_opt_in_is_ignored_at_patch_32(lib):
    from orbit_dataset_amd.model.feature_extractors import create_feature_extractor
    fe, _ = create_feature_extractor("vit_s_32", with_film=True, learn_extractor=False)
    fe.native_backward_patch16 = True
    g = torch.ones(fe.film_size, requires_grad=True)
    assert fe._grad_scope == "none"
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe.wants_grad((g, torch.zeros_like(g)))


def test_learner_flag(lib):
    from orbit_dataset_amd.learner import FROZEN_EXTRACTORS, build_multistep_parser, build_parser, verify_args
    p, m = build_parser(), build_multistep_parser()
    assert p.parse_args([]).vit16_native_backward is False and m.parse_args([]).vit16_native_backward is False
    assert "--vit16_native_backward" in p.format_help()
    flag = ["--vit16_native_backward"]
    for name in NAMES:
        spec = FROZEN_EXTRACTORS[name]
        assert spec.film_flag is None and spec.weight_flag is None and spec.film16_flag == "vit16_native_backward"
        base = ["--feature_extractor", name]
        for mode in ("train", "train_test"):
            for lite in ([], ["--with_lite"]):
                verify_args(p.parse_args(base + flag + ["--mode", mode, "--adapt_features"] + lite))
                for old in ([], ["--vit_native_backward"], ["--vit_native_weight_backward"]):  # and still refused without it
                    with pytest.raises(SystemExit, match="inference-only"):
                        verify_args(p.parse_args(base + old + ["--mode", mode, "--adapt_features"] + lite))
        verify_args(p.parse_args(base + flag + ["--mode", "test"]))
        verify_args(m.parse_args(base + flag + ["--adapt_features"]))
        verify_args(m.parse_args(base + flag))
        with pytest.raises(SystemExit, match="inference-only"):
            verify_args(m.parse_args(base + ["--adapt_features"]))
        for line in (["--mode", "train", "--learn_extractor"], ["--mode", "train", "--learn_extractor", "--adapt_features"],
                     ["--mode", "train_test", "--learn_extractor", "--with_lite"], ["--learn_extractor"]):
            for old in ([], ["--vit_native_backward"], ["--vit_native_weight_backward"]):
                with pytest.raises(SystemExit, match="--vit16_native_backward gives FiLM gradients through a frozen %s only: "
                                                     "--learn_extractor \\(weight gradients" % name):
                    verify_args(p.parse_args(base + flag + old + line))
        with pytest.raises(SystemExit, match="weight gradients"):
            verify_args(m.parse_args(base + flag + ["--adapt_features", "--learn_extractor"]))
        with pytest.raises(SystemExit, match="224"):
            verify_args(p.parse_args(base + flag + ["--frame_size", "84"]))
    # elsewhere the flag changes nothing
    for name in ("vit_s_32", "vit_b_32_clip"):
        assert FROZEN_EXTRACTORS[name].film16_flag is None
        with pytest.raises(SystemExit, match="inference-only"):
            verify_args(p.parse_args(["--feature_extractor", name, "--mode", "train", "--adapt_features"] + flag))
        verify_args(p.parse_args(["--feature_extractor", name, "--mode", "train", "--adapt_features", "--vit_native_backward"] + flag))
        with pytest.raises(SystemExit, match="--vit_native_backward gives FiLM gradients"):
            verify_args(p.parse_args(["--feature_extractor", name, "--mode", "train", "--learn_extractor", "--vit_native_backward"]
                                     + flag))
    verify_args(p.parse_args(["--feature_extractor", "efficientnet_b0", "--mode", "train", "--learn_extractor"] + flag))
    verify_args(p.parse_args(["--feature_extractor", "efficientnet_b0", "--mode", "test"] + flag))
    with pytest.raises(SystemExit, match="inference-only"):
        verify_args(p.parse_args(["--feature_extractor", "efficientnet_v2_s", "--mode", "train", "--adapt_features"] + flag))


def test_one_map_from_flags_to_attributes(lib):
    from orbit_dataset_amd.learner import FROZEN_EXTRACTORS, build_parser, opted_in
    p = build_parser()
    a = p.parse_args(["--vit16_native_backward", "--vit_native_backward", "--vit_native_weight_backward"])
    assert opted_in(a, FROZEN_EXTRACTORS["vit_b_16"]) == ("film", "vit16_native_backward", ["native_backward_patch16"])
    assert opted_in(a, FROZEN_EXTRACTORS["vit_b_32"]) == ("all", "vit_native_weight_backward",
                                                          ["native_weight_backward", "native_backward"])
    assert opted_in(a, FROZEN_EXTRACTORS["efficientnet_v2_s"]) == ("none", None, [])
    assert opted_in(p.parse_args(["--vit_native_backward"]), FROZEN_EXTRACTORS["vit_b_16"]) == ("none", None, [])
