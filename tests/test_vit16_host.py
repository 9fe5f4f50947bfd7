"""CPU-side checks of the patch-16 transformer extractors (vit_s_16, vit_b_16, vit_b_16_clip), as tests/test_vit_host.py for the
patch-32 ones: the orbit_vit_* plan enumerates timm's state_dict and the FiLM slots without touching the device and reports the
197-token geometry (MACs, workspace, batch cap), it has no tape and no backward, the Python module mirrors the pin's parameter
tree and refuses every gradient, the learner sets the reference's normalisation and refuses training, the two new operator entry
points refuse bad arguments before any launch, and the CPU pin (tests/vit16_pin.py) equals Hugging Face's ViTModel /
CLIPVisionModel at patch_size=16."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

import vit16_pin

NAMES = ("vit_s_16", "vit_b_16", "vit_b_16_clip")
# the patch-32 totals minus 2157 D: the patch filter shrinks by 3 * (1024 - 256) D = 2304 D, the position table grows by 147 D
TOTALS = {"vit_s_16": 21665664, "vit_b_16": 85798656, "vit_b_16_clip": 85799424}
# include/orbit_hip.h's definition at 197 tokens: 12 * 12 D^2 * 197 + 196 * 768 * D + 2 * 197^2 * 64 * heads * 12
MACS = {"vit_s_16": 4.5985e9, "vit_b_16": 1.75631e10, "vit_b_16_clip": 1.75631e10}
MAX_B = 2048  # the patch-16 plans' batch cap (include/orbit_hip.h)


def _create(lib, name, H=224, W=224):
    h = ctypes.c_void_p()
    rc = lib.orbit_vit_create(name.encode(), H, W, ctypes.byref(h))
    return rc, h


def _pin_shapes(name):
    return {k: tuple(v.shape) for k, v in vit16_pin.TimmViT16(name).state_dict().items()}


@pytest.mark.parametrize("name", NAMES)
def test_plan_enumerates_the_pin_state_dict_at_197_tokens(lib, name):
    rc, h = _create(lib, name)
    assert rc == 0, _lib.last_error()
    try:
        keys = [lib.orbit_vit_param_name(h, i).decode() for i in range(lib.orbit_vit_num_params(h))]
        numels = [lib.orbit_vit_param_numel(h, i) for i in range(lib.orbit_vit_num_params(h))]
        shapes = _pin_shapes(name)
        assert keys == list(shapes)  # timm's state_dict order
        for k, n in zip(keys, numels):
            assert n == torch.Size(shapes[k]).numel(), k
        assert sum(numels) == TOTALS[name]
        D = lib.orbit_vit_output_size(h)
        assert D == vit16_pin.VIT16[name][0]
        assert dict(zip(keys, numels))["pos_embed"] == 197 * D
        assert dict(zip(keys, numels))["patch_embed.proj.weight"] == D * 3 * 16 * 16
        assert ("patch_embed.proj.bias" in keys) == (name != "vit_b_16_clip")
        assert ("norm_pre.weight" in keys) == (name == "vit_b_16_clip")
        n = lib.orbit_vit_film_slots(h)
        slots = [lib.orbit_vit_film_slot_name(h, i).decode() for i in range(n)]
        assert n == 25 and slots == vit16_pin.TimmViT16(name).film_slot_names()
        assert all(lib.orbit_vit_film_slot_channels(h, i) == D for i in range(n))
        assert lib.orbit_vit_film_size(h) == 25 * D
        macs = lib.orbit_vit_macs_per_frame(h)
        assert abs(macs - MACS[name]) / MACS[name] < 2e-3, macs
        assert lib.orbit_vit_workspace_bytes(h, 200) >= 200 * 197 * 6 * D * 4
    finally:
        lib.orbit_vit_destroy(h)


def test_create_rejects_other_sizes_and_names(lib):
    for name in NAMES:
        for size in (64, 128, 256, 384):
            rc, _ = _create(lib, name, size, size)
            assert rc != 0 and "224" in _lib.last_error()
    for bad in ("vit_l_16", "vit_s_8", "vit_b_16_clip_laion"):
        rc, _ = _create(lib, bad)
        assert rc != 0 and "Invalid feature_extractor_name" in _lib.last_error()
    for name in ("vit_s_32", "vit_b_32", "vit_b_32_clip") + NAMES:  # the error text lists all six
        assert name in _lib.last_error()
    h = ctypes.c_void_p()
    for name in NAMES:
        assert lib.orbit_extractor_create(name.encode(), 224, 224, ctypes.byref(h)) != 0
        assert "Invalid feature_extractor_name" in _lib.last_error()


@pytest.mark.parametrize("name", NAMES)
def test_batch_cap_and_training_entry_points_are_refused_without_a_launch(lib, name):
    """Host pointers throughout: a launch (or a device allocation's use) would fault. The plan holds no parameters, and the
    refusals come before that is even looked at."""
    rc, h = _create(lib, name)
    assert rc == 0
    try:
        buf = (ctypes.c_float * 64)()
        p = ctypes.c_void_p(ctypes.addressof(buf))
        assert lib.orbit_vit_workspace_bytes(h, MAX_B) > 0
        for B in (MAX_B + 1, 3549, 8192, 0, -1):
            assert lib.orbit_vit_workspace_bytes(h, B) == 0
            assert lib.orbit_vit_forward(h, p, B, None, None, p, p, 1 << 40, None) == -1
            assert "batch" in _lib.last_error()
        for B in (1, 16, 200, MAX_B):
            assert lib.orbit_vit_tape_bytes(h, B) == 0
            assert lib.orbit_vit_backward_workspace_bytes(h, B) == 0
            assert lib.orbit_vit_backward_params_workspace_bytes(h, B) == 0
        assert lib.orbit_vit_train_forward(h, p, 1, None, None, p, p, 1 << 40, p, 1 << 40, None) == -1
        assert name in _lib.last_error() and "inference-only" in _lib.last_error()
        assert lib.orbit_vit_backward(h, 1, None, None, p, p, 1 << 40, p, p, p, 1 << 40, None) == -1
        assert name in _lib.last_error() and "inference-only" in _lib.last_error()
        assert lib.orbit_vit_backward_params(h, p, 1, None, None, p, p, 1 << 40, p, p, p, p, 1 << 40, None) == -1
        assert name in _lib.last_error() and "inference-only" in _lib.last_error()
    finally:
        lib.orbit_vit_destroy(h)


def test_patch_32_plans_keep_their_cap_and_their_tape(lib):
    rc, h = _create(lib, "vit_s_32")
    assert rc == 0
    try:
        assert lib.orbit_vit_workspace_bytes(h, 8192) > 0 and lib.orbit_vit_workspace_bytes(h, 8193) == 0
        assert lib.orbit_vit_tape_bytes(h, 4) > 0 and lib.orbit_vit_backward_workspace_bytes(h, 4) > 0
    finally:
        lib.orbit_vit_destroy(h)


@pytest.mark.parametrize("name", NAMES)
def test_module_mirrors_the_pin_and_refuses_every_gradient(lib, name):
    from orbit_dataset_amd.model.feature_extractors import create_feature_extractor
    fe, film_names = create_feature_extractor(name, pretrained=True, with_film=True, learn_extractor=False)
    D = vit16_pin.VIT16[name][0]
    assert fe.output_size == D and fe.film_size == 25 * D and fe.patch_size == 16
    assert {k: tuple(v.shape) for k, v in fe.state_dict().items()} == _pin_shapes(name)
    assert len(film_names) == 50 and film_names[:2] == ["blocks.0.norm1.weight", "blocks.0.norm1.bias"]
    assert film_names[-2:] == ["norm.weight", "norm.bias"]
    pin = vit16_pin.TimmViT16(name)
    assert [n for n, _ in fe.film_slot_modules()] == pin.film_slot_names()
    with torch.no_grad():
        for p in pin.parameters():
            p.normal_()
    fe.load_state_dict(pin.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(fe.state_dict().values(), pin.state_dict().values()))
    assert not fe.wants_grad(None)  # frozen
    g = torch.ones(fe.film_size, requires_grad=True)
    fe2, _ = create_feature_extractor(name, with_film=False, learn_extractor=True)
    for attrs in ({}, {"native_backward": True}, {"native_weight_backward": True},
                  {"native_backward": True, "native_weight_backward": True}):
        for net in (fe, fe2):
            net.native_backward = net.native_weight_backward = False
            for k, v in attrs.items():
                setattr(net, k, v)
        with pytest.raises(NotImplementedError, match=name):
            fe2.wants_grad(None)  # own parameters
        with pytest.raises(NotImplementedError, match=name):
            fe.wants_grad((g, torch.zeros_like(g)))  # FiLM vectors of the frozen network
        with torch.no_grad():
            assert not fe2.wants_grad(None)


def test_learner_flags(lib):
    from orbit_dataset_amd.learner import FROZEN_EXTRACTORS, build_multistep_parser, build_parser, verify_args
    p = build_parser()
    for name, norm in (("vit_s_16", "imagenet_inception"), ("vit_b_16", "imagenet_inception"), ("vit_b_16_clip", "openai_clip")):
        spec = FROZEN_EXTRACTORS[name]
        assert spec.frame_size == 224 and spec.film_flag is None and spec.weight_flag is None
        for extra in ([], ["--adapt_features", "--classifier", "versa"]):
            a = p.parse_args(["--mode", "test", "--feature_extractor", name] + extra)
            verify_args(a)
            assert a.frame_norm_method == norm
        with pytest.raises(SystemExit, match="224"):
            verify_args(p.parse_args(["--feature_extractor", name, "--frame_size", "84"]))
        for bad in (["--mode", "train", "--adapt_features"], ["--mode", "train_test", "--learn_extractor"], ["--learn_extractor"],
                    ["--with_lite"]):
            for opt_in in ([], ["--vit_native_backward"], ["--vit_native_weight_backward"]):
                with pytest.raises(SystemExit, match="inference-only"):
                    verify_args(p.parse_args(["--feature_extractor", name] + bad + opt_in))
    m = build_multistep_parser()
    for name in NAMES:
        verify_args(m.parse_args(["--feature_extractor", name]))
        for opt_in in ([], ["--vit_native_backward"], ["--vit_native_weight_backward"]):
            with pytest.raises(SystemExit, match="inference-only"):
                verify_args(m.parse_args(["--feature_extractor", name, "--adapt_features"] + opt_in))


@pytest.mark.parametrize("name", NAMES)
def test_cpu_pin_equals_hugging_face(name):
    """The bar of tests/test_vit_host.py: 1e-5, plain and with FiLM."""
    from orbit_dataset_amd import synthetic
    from torch.func import functional_call
    pin = vit16_pin.TimmViT16(name).eval()
    synthetic.init_parameters_(pin)
    hf = vit16_pin.load_hf(name, vit16_pin.hf_model(name), pin.state_dict())
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    film = {}
    for slot in pin.film_slot_names():
        film[slot + ".weight"] = 1 + 0.1 * torch.randn(pin.output_size)
        film[slot + ".bias"] = 0.1 * torch.randn(pin.output_size)
    with torch.no_grad():
        assert (pin(x) - vit16_pin.hf_features(name, hf, x)).abs().max().item() <= 1e-5
        a = functional_call(pin, film, (x,))
        b = vit16_pin.film_features_hf(name, hf, film, x)
        assert (a - b).abs().max().item() <= 1e-5
        assert (a - pin(x)).abs().max().item() > 0.1  # FiLM reaches the features


def test_new_operator_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """orbit_op_vit_attention_tokens / orbit_op_vit_patch_embed_p: the checks of their siblings plus the token count / patch size
    (the pointers are host addresses: a launch would fault)."""
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, odd, odd4 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)

    def refused(rc, word):
        assert rc == -1, rc
        assert word in _lib.last_error(), _lib.last_error()

    at = lib.orbit_op_vit_attention_tokens
    for tokens in (49, 196, 198, 0, 224):
        refused(at(p, p, 1, tokens, 384, 6, None), "tokens")
    for tokens in (50, 197):
        refused(at(p, p, 1, tokens, 512, 8, None), "width")
        refused(at(p, p, 1, tokens, 384, 12, None), "heads")
        refused(at(p, p, 1, tokens, 768, 6, None), "heads")
        refused(at(p, p, 0, tokens, 384, 6, None), "batch")
        refused(at(odd4, p, 1, tokens, 384, 6, None), "aligned")
        refused(at(p, None, 1, tokens, 384, 6, None), "null")
    refused(at(p, p, MAX_B + 1, 197, 384, 6, None), "batch")
    refused(at(p, p, 8193, 50, 384, 6, None), "batch")
    refused(at(odd, p, 1, 197, 384, 6, None), "16-byte")  # the 197-token kernel moves float4
    refused(at(p, odd, 1, 197, 384, 6, None), "16-byte")

    pe = lib.orbit_op_vit_patch_embed_p
    for patch in (0, 8, 14, 24, 64):
        refused(pe(p, p, None, p, p, p, 1, 384, patch, 0, None), "patch")
    for patch in (32, 16):
        for D in (0, 128, 512, 1024):
            refused(pe(p, p, None, p, p, p, 1, D, patch, 0, None), "width")
        refused(pe(p, p, None, p, p, p, 1, 384, patch, 32, None), "tile_rows")
        refused(pe(p, p, None, p, p, p, 0, 384, patch, 0, None), "batch")
        refused(pe(odd, p, None, p, p, p, 1, 384, patch, 0, None), "aligned")
        refused(pe(p, odd, None, p, p, p, 1, 384, patch, 0, None), "aligned")
        refused(pe(p, p, None, None, p, p, 1, 384, patch, 0, None), "null")
    refused(pe(p, p, None, p, p, p, MAX_B + 1, 384, 16, 0, None), "batch")
