"""CPU-side checks of the efficientnet_v2_s extractor: the native plan enumerates timm's `tf_efficientnetv2_s_in21k` state_dict in
its order and the reference's FiLM slots without touching the device, the Python module mirrors the parameter tree of the CPU
pin (tests/effnetv2_pin.py), the plan's MAC count equals the pin's, training is refused (the plan reports no training path, the
module raises before anything is launched) and the learners accept the name with the reference's per-backbone settings."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib
from orbit_dataset_amd.model.feature_extractors import create_feature_extractor

import effnetv2_pin

NAME = "efficientnet_v2_s"


@pytest.fixture(scope="module")
def pin():
    return effnetv2_pin.EfficientNet().eval()


def _shapes(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


def test_factory_mirrors_the_pin_and_loads_its_state_dict(lib, pin):
    fe, film_names = create_feature_extractor(NAME, pretrained=True, with_film=False, learn_extractor=False)
    assert film_names is None and fe.output_size == 1280
    assert _shapes(fe) == _shapes(pin)  # keys, order and shapes
    assert sum(p.numel() for p in fe.parameters()) == sum(p.numel() for p in pin.parameters())
    src = effnetv2_pin.EfficientNet()
    with torch.no_grad():
        for t in src.state_dict().values():
            t.copy_(torch.randn(t.shape) if t.is_floating_point() else torch.tensor(7))
    fe.load_state_dict(src.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(fe.state_dict().values(), src.state_dict().values()))
    assert not any(p.requires_grad for p in fe.parameters()) and not fe.wants_grad(None)  # frozen


def test_film_names_follow_the_reference_rule(lib, pin):
    fe, film_names = create_feature_extractor(NAME, pretrained=True, with_film=True, learn_extractor=False)
    slots = effnetv2_pin.film_slot_names(pin)
    assert [n for n, _ in fe.film_slot_modules()] == slots
    assert film_names == [s + leaf for s in slots for leaf in (".weight", ".bias")]
    assert slots[0] == "bn1" and slots[1] == "blocks.0.0.bn1" and slots[-1] == "bn2"
    sizes = [pin.get_submodule(s).num_features for s in slots]
    assert [m.weight.numel() for _, m in fe.film_slot_modules()] == sizes
    assert fe.film_size == sum(sizes)
    assert (len(slots), len(film_names), fe.film_size) == (42, 84, 36712)
    assert all(getattr(m, "film", False) for _, m in fe.film_slot_modules())


def test_plan_macs_equal_the_pins_hook_count(lib, pin):
    fe, _ = create_feature_extractor(NAME, with_film=False, learn_extractor=False)
    for H, W in ((224, 224), (70, 54)):
        assert fe.macs_per_frame(H, W) == effnetv2_pin.count_macs(pin, H, W), (H, W)
    assert abs(fe.macs_per_frame(224, 224) - 2.8486e9) < 1e5


def test_plan_has_no_training_path_under_either_flag(lib, pin):
    keys = [k for k, _ in _shapes(pin) if not k.endswith("num_batches_tracked")]
    for flags in (0, 1):  # 1 = ORBIT_PLAN_UNFUSED
        h = ctypes.c_void_p()
        assert lib.orbit_extractor_create_ex(NAME.encode(), 64, 64, flags, ctypes.byref(h)) == 0, _lib.last_error()
        try:
            assert [lib.orbit_extractor_param_name(h, i).decode() for i in range(lib.orbit_extractor_num_params(h))] == keys
            assert lib.orbit_extractor_output_size(h) == 1280 and lib.orbit_extractor_film_slots(h) == 42
            assert lib.orbit_extractor_supports_training(h) == 0
            assert lib.orbit_extractor_tape_bytes(h, 8) == 0 and lib.orbit_extractor_backward_workspace_bytes(h, 8) == 0
            assert lib.orbit_extractor_workspace_bytes(h, 8) > 8 * 32 * 32 * 24 * 4
        finally:
            lib.orbit_extractor_destroy(h)
    for other in ("efficientnet_b0", "resnet18"):  # the plans that train keep their training path
        h = ctypes.c_void_p()
        assert lib.orbit_extractor_create_ex(other.encode(), 64, 64, 1, ctypes.byref(h)) == 0
        assert lib.orbit_extractor_supports_training(h) == 1 and lib.orbit_extractor_tape_bytes(h, 8) > 0
        lib.orbit_extractor_destroy(h)


def test_grad_requiring_forward_is_refused(lib):
    x = torch.zeros(1, 3, 64, 64)
    fe, _ = create_feature_extractor(NAME, with_film=True, learn_extractor=True)
    fe.eval()
    with pytest.raises(NotImplementedError, match=NAME):
        fe(x)
    fe.requires_grad_(False)
    g = torch.ones(fe.film_size, requires_grad=True)
    with pytest.raises(NotImplementedError, match=NAME):
        fe(x, film=(g, torch.zeros(fe.film_size)))
    fe.train()  # batch-statistics BatchNorm goes through the training runtime too
    with torch.no_grad(), pytest.raises(NotImplementedError, match=NAME):
        fe(x)
    assert not fe._plans, "a plan was built before the refusal"


def test_learner_flags(lib):
    from orbit_dataset_amd.learner import build_multistep_parser, build_parser, verify_args
    p = build_parser()
    a = p.parse_args(["--mode", "test", "--feature_extractor", NAME, "--adapt_features", "--classifier", "proto_cosine",
                      "--frame_norm_method", "imagenet"])
    verify_args(a)
    assert a.frame_norm_method == "imagenet_inception"  # reference utils/args.py:187-188
    for size in ("64", "84", "300"):  # any frame size, as efficientnet_b0
        verify_args(p.parse_args(["--feature_extractor", NAME, "--frame_size", size]))
    a = p.parse_args(["--feature_extractor", "efficientnet_b0"])
    verify_args(a)
    assert a.frame_norm_method == "imagenet"  # the existing names keep their behaviour
    for bad in (["--mode", "train", "--adapt_features"], ["--mode", "train_test", "--learn_extractor"], ["--learn_extractor"],
                ["--with_lite"], ["--mode", "train", "--adapt_features", "--with_lite"]):
        with pytest.raises(SystemExit) as e:
            verify_args(p.parse_args(["--feature_extractor", NAME] + bad))
        assert NAME in str(e.value)
    m = build_multistep_parser()
    a = m.parse_args(["--feature_extractor", NAME])
    verify_args(a)  # the finetuner's head-only steps on frozen features
    assert a.frame_norm_method == "imagenet_inception"
    for bad in (["--adapt_features"], ["--learn_extractor"]):  # its gradient steps through the extractor
        with pytest.raises(SystemExit) as e:
            verify_args(m.parse_args(["--feature_extractor", NAME] + bad))
        assert NAME in str(e.value)
