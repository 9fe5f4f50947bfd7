"""CPU-side checks of the opt-in FiLM backward through the frozen efficientnet_v2_s: the plan flag ORBIT_PLAN_RES_POST_BACKWARD
opens the training-size queries for this network alone and changes nothing for the others, the learner flag
--effnetv2_native_backward admits exactly the recipes that need FiLM gradients and nothing that needs weight gradients, and the
module with native_backward = True still refuses weight gradients and train() mode before a plan exists. The pins of the
default behaviour (flags 0 and 1, no learner flag, native_backward = False) are tests/test_effnetv2_host.py."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib
from orbit_dataset_amd.model.feature_extractors import EfficientNetV2S, create_feature_extractor

import effnetv2_pin

NAME = "efficientnet_v2_s"
UNFUSED, RES_POST_BACKWARD = 1, 2  # ORBIT_PLAN_UNFUSED, ORBIT_PLAN_RES_POST_BACKWARD


def _create(lib, name, flags, size=64):
    h = ctypes.c_void_p()
    assert lib.orbit_extractor_create_ex(name.encode(), size, size, flags, ctypes.byref(h)) == 0, _lib.last_error()
    return h


def _sizes(lib, h, B=8):
    return (lib.orbit_extractor_supports_training(h), lib.orbit_extractor_tape_bytes(h, B),
            lib.orbit_extractor_backward_workspace_bytes(h, B))


def test_the_flag_opens_the_training_queries_with_the_same_parameters(lib):
    pin = effnetv2_pin.EfficientNet().eval()
    assert len(pin.state_dict()) == 780  # the pin's key list; the plan holds all of it but the 110 step counters
    keys = [k for k in pin.state_dict() if not k.endswith("num_batches_tracked")]
    assert len(keys) == 670
    sizes = {}
    for flags in (RES_POST_BACKWARD, UNFUSED | RES_POST_BACKWARD):
        h = _create(lib, NAME, flags)
        try:
            assert [lib.orbit_extractor_param_name(h, i).decode() for i in range(lib.orbit_extractor_num_params(h))] == keys
            assert lib.orbit_extractor_output_size(h) == 1280 and lib.orbit_extractor_film_slots(h) == 42
            sup, tape, ws = sizes[flags] = _sizes(lib, h)
            assert sup == 1 and tape > 0 and ws > 0
            # the tape holds at least the raw output and the activation of every conv: here just the stem's 32 x 32 x 24 pair
            assert tape > 8 * 2 * 32 * 32 * 24 * 4
            assert lib.orbit_extractor_tape_bytes(h, 0) == 0 and lib.orbit_extractor_backward_workspace_bytes(h, 0) == 0
        finally:
            lib.orbit_extractor_destroy(h)
    assert sizes[RES_POST_BACKWARD] == sizes[UNFUSED | RES_POST_BACKWARD]  # no fused op in this plan: one op list


def test_without_the_flag_nothing_is_reported(lib):
    for flags in (0, UNFUSED):
        h = _create(lib, NAME, flags)
        try:
            assert _sizes(lib, h) == (0, 0, 0)
        finally:
            lib.orbit_extractor_destroy(h)


@pytest.mark.parametrize("other", ["efficientnet_b0", "resnet18", "set_encoder"])
def test_the_flag_changes_nothing_for_the_other_networks(lib, other):
    got = {}
    for flags in (UNFUSED, UNFUSED | RES_POST_BACKWARD):
        h = _create(lib, other, flags)
        try:
            names = [lib.orbit_extractor_param_name(h, i).decode() for i in range(lib.orbit_extractor_num_params(h))]
            got[flags] = (names, _sizes(lib, h), lib.orbit_extractor_workspace_bytes(h, 8), lib.orbit_extractor_macs_per_frame(h))
        finally:
            lib.orbit_extractor_destroy(h)
    assert got[UNFUSED] == got[UNFUSED | RES_POST_BACKWARD]
    assert got[UNFUSED][1][0] == 1 and got[UNFUSED][1][1] > 0


def test_learner_flag_matrix(lib):
    from orbit_dataset_amd.learner import build_multistep_parser, build_parser, verify_args
    p, m = build_parser(), build_multistep_parser()
    assert p.parse_args([]).effnetv2_native_backward is False and m.parse_args([]).effnetv2_native_backward is False
    base = ["--feature_extractor", NAME, "--effnetv2_native_backward"]
    for ok in (["--mode", "train", "--adapt_features"], ["--mode", "train_test", "--adapt_features"],
               ["--mode", "train", "--adapt_features", "--with_lite"], ["--mode", "test", "--adapt_features"],
               ["--mode", "test", "--with_lite"], ["--mode", "test"]):
        a = p.parse_args(base + ok)
        verify_args(a)
        assert a.frame_norm_method == "imagenet_inception"  # still forced (reference utils/args.py:187-188)
    for ok in ([], ["--adapt_features"]):  # the finetuner: head-only steps, and its gradient steps on the FiLM layers
        a = m.parse_args(base + ok)
        verify_args(a)
        assert a.frame_norm_method == "imagenet_inception"
    for bad in (["--mode", "train", "--learn_extractor"], ["--mode", "train", "--adapt_features", "--learn_extractor"],
                ["--learn_extractor"]):
        with pytest.raises(SystemExit, match="--effnetv2_native_backward gives FiLM gradients through a frozen " + NAME):
            verify_args(p.parse_args(base + bad))
    with pytest.raises(SystemExit, match=NAME):
        verify_args(m.parse_args(base + ["--learn_extractor"]))
    # training still needs something to train (reference utils/args.py:203-205)
    with pytest.raises(SystemExit, match="at least one of"):
        verify_args(p.parse_args(base + ["--mode", "train"]))
    # without the flag the refusals of tests/test_effnetv2_host.py hold
    for bad in (["--mode", "train", "--adapt_features"], ["--with_lite"], ["--mode", "train", "--adapt_features", "--with_lite"]):
        with pytest.raises(SystemExit, match="inference-only"):
            verify_args(p.parse_args(["--feature_extractor", NAME] + bad))
    with pytest.raises(SystemExit, match="inference-only"):
        verify_args(m.parse_args(["--feature_extractor", NAME, "--adapt_features"]))
    # ignored for the other extractors
    a = p.parse_args(["--feature_extractor", "resnet18", "--effnetv2_native_backward", "--mode", "train", "--learn_extractor"])
    verify_args(a)
    assert a.frame_norm_method == "imagenet"
    with pytest.raises(SystemExit, match="inference-only"):
        verify_args(p.parse_args(["--feature_extractor", "vit_s_32", "--effnetv2_native_backward", "--mode", "train",
                                  "--adapt_features"]))


def test_module_still_refuses_weight_gradients_and_train_mode(lib):
    assert EfficientNetV2S.native_backward is False
    x = torch.zeros(1, 3, 64, 64)
    fe, _ = create_feature_extractor(NAME, with_film=True, learn_extractor=True)
    assert fe.native_backward is False
    fe.native_backward = True
    fe.eval()
    with pytest.raises(NotImplementedError, match="weight gradients"):
        fe(x)  # every own parameter requires a gradient
    g = torch.ones(fe.film_size, requires_grad=True)
    with pytest.raises(NotImplementedError, match="weight gradients"):
        fe(x, film=(g, torch.zeros(fe.film_size)))
    fe.requires_grad_(False)
    fe.conv_stem.weight.requires_grad_(True)  # one filter is enough
    with pytest.raises(NotImplementedError, match="conv_stem.weight"):
        fe(x, film=(g, torch.zeros(fe.film_size)))
    fe.requires_grad_(False)
    fe.train()
    with pytest.raises(NotImplementedError, match="batch-statistics"):
        fe(x, film=(g, torch.zeros(fe.film_size)))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="train\\(\\) mode"):
        fe(x)
    assert not fe._plans, "a plan was built before the refusal"
    # and the class default still refuses FiLM gradients as an inference-only extractor
    fe2, _ = create_feature_extractor(NAME, with_film=True, learn_extractor=False)
    fe2.eval()
    with pytest.raises(NotImplementedError, match="inference-only"):
        fe2(x, film=(g, torch.zeros(fe2.film_size)))
    assert not fe2._plans
