"""CPU-side checks of the second efficientnet_v2_s opt-in: the plan flag ORBIT_PLAN_RES_POST_TRAINING (= 4, implies
ORBIT_PLAN_RES_POST_BACKWARD) opens the training-size queries with the same 670 parameters and changes nothing for the other
networks; the learner flag --effnetv2_native_weight_backward admits what the other extractors train (--learn_extractor, with or
without --with_lite / --adapt_features) and still forces the frame normalisation; the module with native_weight_backward = True
has the gradient scope "all", and a plan key of its own per scope. The pins of the defaults and of the first opt-in are
tests/test_effnetv2_host.py and tests/test_effnetv2_train_host.py; without the new attribute their refusals hold (called here)."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib
from orbit_dataset_amd.model.feature_extractors import EfficientNetV2S, create_feature_extractor

import effnetv2_pin
import test_effnetv2_train_host as first_opt_in

NAME = "efficientnet_v2_s"
UNFUSED, RES_POST_BACKWARD, RES_POST_TRAINING = 1, 2, 4


def _create(lib, name, flags, size=64):
    h = ctypes.c_void_p()
    assert lib.orbit_extractor_create_ex(name.encode(), size, size, flags, ctypes.byref(h)) == 0, _lib.last_error()
    return h


def _sizes(lib, h, B=8):
    return (lib.orbit_extractor_supports_training(h), lib.orbit_extractor_tape_bytes(h, B),
            lib.orbit_extractor_backward_workspace_bytes(h, B))


def test_the_flag_opens_the_training_queries_with_the_same_parameters(lib):
    pin = effnetv2_pin.EfficientNet().eval()
    keys = [k for k in pin.state_dict() if not k.endswith("num_batches_tracked")]
    assert len(keys) == 670
    sizes = {}
    for flags in (4, 5, 6, 7):
        h = _create(lib, NAME, flags)
        try:
            assert [lib.orbit_extractor_param_name(h, i).decode() for i in range(lib.orbit_extractor_num_params(h))] == keys
            sup, tape, ws = sizes[flags] = _sizes(lib, h)
            assert sup == 1 and tape > 0 and ws > 0
            assert lib.orbit_extractor_tape_bytes(h, 0) == 0 and lib.orbit_extractor_backward_workspace_bytes(h, 0) == 0
        finally:
            lib.orbit_extractor_destroy(h)
    assert len(set(sizes.values())) == 1  # one op list, one layout under every combination
    # ... which is the layout of the first opt-in: the new flag sizes nothing differently
    h = _create(lib, NAME, UNFUSED | RES_POST_BACKWARD)
    try:
        assert _sizes(lib, h) == sizes[4]
    finally:
        lib.orbit_extractor_destroy(h)


@pytest.mark.parametrize("other", ["efficientnet_b0", "resnet18", "set_encoder"])
def test_the_flag_changes_nothing_for_the_other_networks(lib, other):
    """Names, sizes, workspace and MACs under the flag equal those without it: on the tape-recording plan (flag 1 against 5) and
    on the default plan (0 against 4; efficientnet_b0's holds the fused fronts and reports no training path either way)."""
    got = {}
    for flags in (0, RES_POST_TRAINING, UNFUSED, UNFUSED | RES_POST_TRAINING, UNFUSED | RES_POST_BACKWARD | RES_POST_TRAINING):
        h = _create(lib, other, flags)
        try:
            names = [lib.orbit_extractor_param_name(h, i).decode() for i in range(lib.orbit_extractor_num_params(h))]
            numel = [lib.orbit_extractor_param_numel(h, i) for i in range(len(names))]
            got[flags] = (names, numel, _sizes(lib, h), lib.orbit_extractor_workspace_bytes(h, 8), lib.orbit_extractor_macs_per_frame(h))
        finally:
            lib.orbit_extractor_destroy(h)
    assert got[UNFUSED] == got[UNFUSED | RES_POST_TRAINING] == got[7]
    assert got[0] == got[RES_POST_TRAINING]
    assert got[UNFUSED][2][0] == 1 and got[UNFUSED][2][1] > 0


def test_learner_flag_matrix(lib):
    from orbit_dataset_amd.learner import build_multistep_parser, build_parser, verify_args
    p, m = build_parser(), build_multistep_parser()
    assert p.parse_args([]).effnetv2_native_weight_backward is False
    assert m.parse_args([]).effnetv2_native_weight_backward is False
    for both in ([], ["--effnetv2_native_backward"]):  # the new flag alone, or together with the FiLM flag
        base = ["--feature_extractor", NAME, "--effnetv2_native_weight_backward"] + both
        for ok in (["--mode", "train", "--learn_extractor"], ["--mode", "train", "--learn_extractor", "--with_lite"],
                   ["--mode", "train", "--adapt_features", "--learn_extractor"], ["--mode", "train", "--adapt_features"],
                   ["--mode", "test"], ["--mode", "test", "--with_lite"]):
            a = p.parse_args(base + ok)
            verify_args(a)
            assert a.frame_norm_method == "imagenet_inception"  # still forced (reference utils/args.py:187-188)
        for ok in (["--learn_extractor"], ["--adapt_features"], []):  # the finetuner
            a = m.parse_args(base + ok)
            verify_args(a)
            assert a.frame_norm_method == "imagenet_inception"
        with pytest.raises(SystemExit, match="at least one of"):
            verify_args(p.parse_args(base + ["--mode", "train"]))
    # ignored for the other extractors
    a = p.parse_args(["--feature_extractor", "resnet18", "--effnetv2_native_weight_backward", "--mode", "train", "--learn_extractor"])
    verify_args(a)
    assert a.frame_norm_method == "imagenet"
    for vit in ("vit_s_32", "vit_b_32", "vit_b_32_clip"):
        with pytest.raises(SystemExit, match="inference-only"):
            verify_args(p.parse_args(["--feature_extractor", vit, "--effnetv2_native_weight_backward", "--mode", "train",
                                      "--learn_extractor"]))


def test_learner_sets_the_attribute(lib):
    from orbit_dataset_amd.learner import FROZEN_EXTRACTORS
    spec = FROZEN_EXTRACTORS[NAME]
    assert spec.film_flag == "effnetv2_native_backward" and spec.weight_flag == "effnetv2_native_weight_backward"
    assert spec.frame_norm == "imagenet_inception" and spec.frame_size is None


def test_module_scope_and_plan_keys(lib):
    assert EfficientNetV2S.native_weight_backward is False
    fe, _ = create_feature_extractor(NAME, with_film=True, learn_extractor=True)
    assert fe._grad_scope == "none"
    keys = {fe._plan_key(64, 64, True)}
    fe.native_backward = True
    assert fe._grad_scope == "film"
    keys.add(fe._plan_key(64, 64, True))
    fe.native_weight_backward = True  # implies the first
    assert fe._grad_scope == "all"
    keys.add(fe._plan_key(64, 64, True))
    fe.native_backward = False
    assert fe._grad_scope == "all" and fe._plan_key(64, 64, True) in keys
    assert len(keys) == 3, "two scopes share a training plan key"
    # the inference plan carries no flag: one key whatever the scope
    infer = fe._plan_key(64, 64, False)
    fe.native_weight_backward = False
    assert fe._plan_key(64, 64, False) == infer
    # flipping the attribute between two calls never lands on the other scope's plan
    fe.native_backward = True
    a = fe._plan_key(64, 64, True)
    fe.native_weight_backward = True
    b = fe._plan_key(64, 64, True)
    assert a != b
    # the plans built for the keys carry the flags of their scope (built on the host: no device is touched)
    plan_all = fe._plan(64, 64, trainable=True)
    fe.native_weight_backward = False
    plan_film = fe._plan(64, 64, trainable=True)
    assert plan_all is not plan_film and len(fe._plans) == 2
    assert lib.orbit_extractor_supports_training(plan_all.handle) == 1
    assert lib.orbit_extractor_supports_training(plan_film.handle) == 1


def test_with_the_attribute_nothing_is_refused_before_the_device(lib):
    """train() mode and own parameters that require a gradient pass the module's scope rule (wants_grad) under the opt-in."""
    fe, _ = create_feature_extractor(NAME, with_film=True, learn_extractor=True)
    fe.native_weight_backward = True
    fe.train()
    assert fe.wants_grad(None) is True  # every own parameter requires a gradient: admitted
    g = torch.ones(fe.film_size, requires_grad=True)
    assert fe.wants_grad((g, torch.zeros(fe.film_size))) is True
    fe.requires_grad_(False)
    fe.conv_stem.weight.requires_grad_(True)
    assert fe.wants_grad(None) is True
    if not torch.cuda.is_available():  # the forward itself gets as far as asking for the device
        with pytest.raises(_lib.OrbitHipError):
            fe(torch.zeros(1, 3, 64, 64))


def test_without_the_attribute_every_refusal_holds(lib):
    first_opt_in.test_module_still_refuses_weight_gradients_and_train_mode(lib)
    first_opt_in.test_learner_flag_matrix(lib)
    first_opt_in.test_without_the_flag_nothing_is_reported(lib)
