"""CPU-side checks of the transformer extractors at other frame sizes than 224 (orbit_vit_create_sized;
VisionTransformer.resample_pos_embed; --vit_resample_pos_embed): the geometry of the sized plans, every refusal of the plan and
of the new operator entry points with host pointers (a launch would fault: the refusals come first), orbit_vit_create still
refusing, the module's gradient refusal before any device use, the learner's flag matrix, and the sized CPU pin
(tests/vit_sized_pin.py) against Hugging Face's ViTModel / CLIPVisionModel under interpolate_pos_encoding=True."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

import vit_sized_pin

NAMES = ("vit_s_32", "vit_b_32", "vit_b_32_clip", "vit_s_16", "vit_b_16", "vit_b_16_clip")
SIZES = (32, 96, 224, 384, 512)
ROWS_CAP = 8192 * 50  # token rows the caps at 224 allow (include/orbit_hip.h)


def _sized(lib, name, H, W=None):
    h = ctypes.c_void_p()
    rc = lib.orbit_vit_create_sized(name.encode(), H, H if W is None else W, ctypes.byref(h))
    return rc, h


def _params(lib, h):
    n = lib.orbit_vit_num_params(h)
    return [(lib.orbit_vit_param_name(h, i).decode(), lib.orbit_vit_param_numel(h, i)) for i in range(n)]


@pytest.mark.parametrize("name", NAMES)
def test_geometry_of_sized_plans(lib, name):
    patch = vit_sized_pin.patch_of(name)
    ref = ctypes.c_void_p()
    assert lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(ref)) == 0, _lib.last_error()
    try:
        want = _params(lib, ref)
        D = lib.orbit_vit_output_size(ref)
        for S in SIZES:
            rc, h = _sized(lib, name, S)
            assert rc == 0, _lib.last_error()
            try:
                assert _params(lib, h) == want, "S=%d: other parameters than orbit_vit_create's" % S
                assert dict(want)["pos_embed"] == ((224 // patch) ** 2 + 1) * D  # the checkpoint's table at every size
                assert lib.orbit_vit_output_size(h) == D and lib.orbit_vit_film_size(h) == 25 * D
                P = (S // patch) ** 2
                N = P + 1
                macs = P * 3 * patch * patch * D + 12 * (12 * D * D * N + 2 * N * N * D)
                assert lib.orbit_vit_macs_per_frame(h) == float(macs), (S, lib.orbit_vit_macs_per_frame(h), macs)
                # batch cap: the largest B with B * N <= 8192 * 50; at 224 the plan is an orbit_vit_create plan, caps included
                max_b = ROWS_CAP // N if S != 224 else (8192 if patch == 32 else 2048)
                assert lib.orbit_vit_workspace_bytes(h, max_b) >= max_b * N * 6 * D * 4
                assert lib.orbit_vit_workspace_bytes(h, max_b + 1) == 0 and lib.orbit_vit_workspace_bytes(h, 0) == 0
                if S == 224:
                    assert lib.orbit_vit_macs_per_frame(h) == lib.orbit_vit_macs_per_frame(ref)
                    for B in (1, 7, max_b, max_b + 1):
                        assert lib.orbit_vit_workspace_bytes(h, B) == lib.orbit_vit_workspace_bytes(ref, B)
                        assert lib.orbit_vit_tape_bytes(h, B) == lib.orbit_vit_tape_bytes(ref, B)
                        assert lib.orbit_vit_backward_workspace_bytes(h, B) == lib.orbit_vit_backward_workspace_bytes(ref, B)
            finally:
                lib.orbit_vit_destroy(h)
    finally:
        lib.orbit_vit_destroy(ref)


def test_create_sized_refusals(lib):
    def refused(rc, *words):
        assert rc == -1, rc
        for w in words:
            assert w in _lib.last_error(), _lib.last_error()

    refused(_sized(lib, "vit_s_32", 96, 128)[0], "square", "96x128")
    refused(_sized(lib, "vit_s_16", 224, 208)[0], "square")
    refused(_sized(lib, "vit_s_32", 80)[0], "multiple", "32", "64 and 96")
    refused(_sized(lib, "vit_b_32_clip", 240)[0], "multiple", "224 and 256")
    refused(_sized(lib, "vit_s_16", 100)[0], "multiple", "16", "96 and 112")
    refused(_sized(lib, "vit_s_16", 16)[0], "below 32")
    refused(_sized(lib, "vit_s_32", 0)[0], "below 32")
    refused(_sized(lib, "vit_s_32", -32)[0], "below 32")
    refused(_sized(lib, "vit_s_32", 544)[0], "above 512")
    refused(_sized(lib, "vit_b_16", 528)[0], "above 512")
    refused(_sized(lib, "vit_l_16", 224)[0], "Invalid feature_extractor_name")
    refused(_sized(lib, "resnet18", 224)[0], "Invalid feature_extractor_name")
    assert lib.orbit_vit_create_sized(None, 224, 224, ctypes.byref(ctypes.c_void_p())) == -1
    assert lib.orbit_vit_create_sized(b"vit_s_32", 224, 224, None) == -1 and "null" in _lib.last_error()


def test_create_keeps_refusing_other_sizes(lib):
    for name in NAMES:
        for size in (96, 128, 256, 384):
            h = ctypes.c_void_p()
            assert lib.orbit_vit_create(name.encode(), size, size, ctypes.byref(h)) == -1
            assert "224x224 frames only (fixed position table)" in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("name", ["vit_s_32", "vit_b_16_clip"])
def test_training_paths_are_refused_by_frame_size_before_any_launch(lib, name):
    """Host pointers throughout. A sized plan at 224 opens the backward entry points on orbit_vit_create's terms."""
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    q = ctypes.c_void_p(base + (-base % 256))
    rc, h = _sized(lib, name, 96)
    assert rc == 0, _lib.last_error()
    try:
        calls = {"vit_enable_backward": lambda: lib.orbit_vit_enable_backward(h),
                 "vit_enable_weight_backward": lambda: lib.orbit_vit_enable_weight_backward(h),
                 "vit_train_forward": lambda: lib.orbit_vit_train_forward(h, q, 1, None, None, q, q, 1 << 40, q, 1 << 40, None),
                 "vit_backward": lambda: lib.orbit_vit_backward(h, 1, None, None, q, q, 1 << 40, q, q, q, 1 << 40, None),
                 "vit_backward_params": lambda: lib.orbit_vit_backward_params(h, q, 1, None, None, q, q, 1 << 40, q, q, q, q,
                                                                              1 << 40, None)}
        for who, call in calls.items():
            assert call() == -1, who
            err = _lib.last_error()
            assert who in err and "96x96" in err and "frame size 96" in err, err
        for B in (1, 2, 64):
            assert lib.orbit_vit_tape_bytes(h, B) == 0
            assert lib.orbit_vit_backward_workspace_bytes(h, B) == 0
            assert lib.orbit_vit_backward_params_workspace_bytes(h, B) == 0
            assert lib.orbit_vit_workspace_bytes(h, B) > 0
        assert lib.orbit_vit_enable_bf16(h) == 0, _lib.last_error()  # allowed
        assert lib.orbit_vit_bf16_enabled(h) == 1
        assert lib.orbit_vit_train_forward(h, q, 1, None, None, q, q, 1 << 40, q, 1 << 40, None) == -1
        assert "frame size 96" in _lib.last_error()  # (still the frame size, with bf16 on top)
        # a forward before the parameters are loaded is a state error, not a launch
        assert lib.orbit_vit_forward(h, q, 1, None, None, q, q, 1 << 40, None) != 0 and "finalize" in _lib.last_error()
    finally:
        lib.orbit_vit_destroy(h)
    rc, h = _sized(lib, name, 224)
    ref = ctypes.c_void_p()
    assert rc == 0 and lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(ref)) == 0
    try:
        for plan in (h, ref):
            assert lib.orbit_vit_enable_weight_backward(plan) == 0, _lib.last_error()
        for B in (1, 5):
            assert lib.orbit_vit_tape_bytes(h, B) == lib.orbit_vit_tape_bytes(ref, B) > 0
            assert (lib.orbit_vit_backward_params_workspace_bytes(h, B)
                    == lib.orbit_vit_backward_params_workspace_bytes(ref, B) > 0)
        # the training entry points get as far on the sized plan as on the other: the state check (nothing is loaded)
        for plan in (h, ref):
            assert lib.orbit_vit_train_forward(plan, q, 1, None, None, q, q, 1 << 40, q, 1 << 40, None) != 0
            assert "finalize" in _lib.last_error(), _lib.last_error()
    finally:
        lib.orbit_vit_destroy(h)
        lib.orbit_vit_destroy(ref)


def test_sized_operator_entry_points_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, odd, odd4, p2 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 64)

    def refused(rc, word):
        assert rc == -1, rc
        assert word in _lib.last_error(), _lib.last_error()

    at = lib.orbit_op_vit_attention_n
    for tokens in (0, -1, ROWS_CAP + 1):
        refused(at(p, p2, 1, tokens, 384, 6, None), "tokens")
    for tokens in (1, 5, 50, 197, 577):
        refused(at(p, p2, 1, tokens, 512, 8, None), "width")
        refused(at(p, p2, 1, tokens, 384, 12, None), "heads")
        refused(at(p, p2, 1, tokens, 768, 6, None), "heads")
        refused(at(p, p2, 0, tokens, 384, 6, None), "batch")
        refused(at(p, p2, ROWS_CAP // tokens + 1, tokens, 384, 6, None), "batch")
        refused(at(odd, p2, 1, tokens, 384, 6, None), "16-byte")
        refused(at(p, odd, 1, tokens, 384, 6, None), "16-byte")
        refused(at(p, None, 1, tokens, 384, 6, None), "null")
        refused(at(None, p2, 1, tokens, 384, 6, None), "null")

    rs = lib.orbit_op_vit_pos_resample
    for g in (0, 6, 8, 13, 28):
        refused(rs(p, p2, g, 4, 384, None), "source grid")
    for G in (0, -1, 33):
        refused(rs(p, p2, 7, G, 384, None), "target grid")
    for D in (0, 128, 512, 1024):
        refused(rs(p, p2, 14, 5, D, None), "width")
    refused(rs(odd4, p2, 7, 3, 384, None), "aligned")
    refused(rs(p, odd4, 7, 3, 384, None), "aligned")
    refused(rs(p, p, 7, 3, 384, None), "alias")
    refused(rs(None, p2, 7, 3, 384, None), "null")
    refused(rs(p, None, 7, 3, 384, None), "null")

    pe = lib.orbit_op_vit_patch_embed_sized
    for patch in (0, 8, 14, 24, 64):
        refused(pe(p, p, None, p, p, p, 1, 384, patch, 224, 0, None), "patch")
    for patch in (32, 16):
        for S in (0, 16, 100, 225, 528, 1024):
            refused(pe(p, p, None, p, p, p, 1, 384, patch, S, 0, None), "frame size")
        for D in (0, 128, 512, 1024):
            refused(pe(p, p, None, p, p, p, 1, D, patch, 96, 0, None), "width")
        refused(pe(p, p, None, p, p, p, 1, 384, patch, 96, 32, None), "tile_rows")
        refused(pe(p, p, None, p, p, p, 0, 384, patch, 96, 0, None), "batch")
        refused(pe(p, p, None, p, p, p, ROWS_CAP // ((96 // patch) ** 2 + 1) + 1, 384, patch, 96, 0, None), "batch")
        refused(pe(odd, p, None, p, p, p, 1, 384, patch, 96, 0, None), "aligned")
        refused(pe(p, odd, None, p, p, p, 1, 384, patch, 96, 0, None), "aligned")
        refused(pe(p, p, None, None, p, p, 1, 384, patch, 96, 0, None), "null")
    refused(pe(p, p, None, p, p, p, 1, 384, 32, 48, 0, None), "frame size")  # a multiple of 16, not of 32


@pytest.mark.parametrize("name", ["vit_s_32", "vit_s_16"])
def test_module_attribute_keys_and_gradient_refusal_before_any_device_use(lib, name):
    from orbit_dataset_amd.model.feature_extractors import VisionTransformer, create_feature_extractor
    assert VisionTransformer.resample_pos_embed is False
    fe, _ = create_feature_extractor(name, with_film=True, learn_extractor=True)
    shapes = {k: tuple(v.shape) for k, v in fe.state_dict().items()}
    plain = fe._plan_key(224, 224, False)
    with pytest.raises(ValueError, match="224"):
        fe._plan(96, 96)  # without the attribute today's refusal stands
    fe.resample_pos_embed = True
    assert "resample_pos_embed" in fe.__dict__ and VisionTransformer.resample_pos_embed is False  # per instance
    assert {k: tuple(v.shape) for k, v in fe.state_dict().items()} == shapes  # pos_embed stays the checkpoint's
    assert fe._plan_key(224, 224, False) == plain + ("sized",)  # a sized plan is a plan of its own, at 224 too
    fe.bf16_inference = True
    assert fe._plan_key(96, 96, False) == (96, 96, False, "sized", "bf16")
    fe.bf16_inference = False
    x = torch.zeros(1, 3, 96, 96)  # a host tensor: the refusals below come before the device is asked for
    for opt_in in ((), ("native_backward",), ("native_weight_backward",), ("native_backward_patch16",),
                   ("native_weight_backward_patch16",)):
        for attr in opt_in:
            setattr(fe, attr, True)
        with pytest.raises(NotImplementedError, match="resample_pos_embed"):
            fe(x)
        g = torch.ones(fe.film_size, requires_grad=True)
        fe.requires_grad_(False)
        with pytest.raises(NotImplementedError, match="resample_pos_embed"):
            fe(x, film=(g, torch.zeros_like(g)))
        fe.requires_grad_(True)
        for attr in opt_in:
            setattr(fe, attr, False)
    assert not fe._plans, "a plan was built before the refusal"
    patch = fe.patch_size
    for bad, word in (((96, 128), "square"), ((16, 16), "32..512"), ((544, 544), "32..512"), ((104, 104), "multiple")):
        with pytest.raises(ValueError, match=word):
            fe(torch.zeros(1, 3, *bad))
    with pytest.raises(ValueError, match="%d and %d" % (104 // patch * patch, (104 // patch + 1) * patch)):
        fe(torch.zeros(1, 3, 104, 104))
    # plans through orbit_vit_create_sized: built on the host, nothing launched
    assert fe.macs_per_frame(96, 96) < fe.macs_per_frame(224, 224) < fe.macs_per_frame(384, 384)
    fe.resample_pos_embed = False
    assert fe._plan_key(224, 224, False) == plain
    with pytest.raises(ValueError, match="224"):
        fe._plan(96, 96)


def test_learner_flag_matrix(lib, capsys):
    from orbit_dataset_amd.learner import FROZEN_EXTRACTORS, build_multistep_parser, build_parser, verify_args
    p, m = build_parser(), build_multistep_parser()
    flag = "--vit_resample_pos_embed"
    for name in NAMES:
        assert FROZEN_EXTRACTORS[name].frame_size == 224
        patch = vit_sized_pin.patch_of(name)
        base = ["--mode", "test", "--feature_extractor", name]
        assert p.parse_args(base).vit_resample_pos_embed is False
        for S in (96, 128, 224, 384, 512):
            a = p.parse_args(base + ["--frame_size", str(S), flag])
            verify_args(a)
            assert a.vit_resample_pos_embed is True and a.frame_size == S
            verify_args(m.parse_args(["--feature_extractor", name, "--frame_size", str(S), flag]))
        with pytest.raises(SystemExit, match="needs --frame_size 224"):  # without the flag: today's message
            verify_args(p.parse_args(base + ["--frame_size", "96"]))
        bad = 96 + patch // 2
        with pytest.raises(SystemExit, match="nearest valid sizes are %d and %d" % (bad // patch * patch, (bad // patch + 1) * patch)):
            verify_args(p.parse_args(base + ["--frame_size", str(bad), flag]))
        with pytest.raises(SystemExit, match="32..512"):
            verify_args(p.parse_args(base + ["--frame_size", "544", flag]))
        for mode in ("train", "train_test"):
            for opt_in in ([], ["--vit_native_backward"], ["--vit_native_weight_backward"], ["--vit16_native_backward"],
                           ["--vit16_native_weight_backward"]):
                with pytest.raises(SystemExit, match="vit_resample_pos_embed"):
                    verify_args(p.parse_args(["--feature_extractor", name, "--mode", mode, "--adapt_features", "--frame_size", "96",
                                              flag] + opt_in))
        for grads in (["--learn_extractor"], ["--adapt_features"]):
            with pytest.raises(SystemExit, match="vit_resample_pos_embed"):
                verify_args(m.parse_args(["--feature_extractor", name, "--frame_size", "96", flag] + grads))
    # at 224 the flag changes nothing that is admitted or refused
    verify_args(p.parse_args(["--feature_extractor", "vit_s_32", "--mode", "train", "--adapt_features", "--vit_native_backward", flag]))
    with pytest.raises(SystemExit, match="inference-only"):
        verify_args(p.parse_args(["--feature_extractor", "vit_s_32", "--mode", "train", "--adapt_features", flag]))
    # composes with --vit_bf16
    verify_args(p.parse_args(["--mode", "test", "--feature_extractor", "vit_b_16_clip", "--frame_size", "128", flag, "--vit_bf16"]))
    capsys.readouterr()
    a = p.parse_args(["--mode", "train", "--learn_extractor", "--feature_extractor", "resnet18", "--frame_size", "84", flag])
    verify_args(a)
    out = capsys.readouterr().out
    assert a.vit_resample_pos_embed is False and out.count("\n") == 1 and "--vit_resample_pos_embed is ignored" in out
    assert "resnet18" in out


HF_CASES = [("vit_s_32", (64, 96, 160, 384)), ("vit_b_32_clip", (96, 288)), ("vit_s_16", (32, 80, 256)), ("vit_b_16_clip", (48, 160))]


@pytest.mark.parametrize("name,sizes", HF_CASES, ids=[c[0] for c in HF_CASES])
def test_sized_cpu_pin_equals_hugging_face(name, sizes):
    """The bar of tests/test_vit_host.py: 1e-5, on the parameters of synthetic.init_parameters_."""
    from orbit_dataset_amd import synthetic
    pin = vit_sized_pin.SizedViT(name).eval()
    synthetic.init_parameters_(pin)
    hf = vit_sized_pin.load_hf(name, vit_sized_pin.hf_model(name), pin.state_dict())
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for S in sizes:
            x = torch.randn(2, 3, S, S, generator=gen)
            err = (pin(x) - vit_sized_pin.hf_features(name, hf, x)).abs().max().item()
            print("[vit-sized] %s %dx%d: |pin - hf| %.3g" % (name, S, S, err))
            assert err <= 1e-5, (name, S, err)
        # at 224 the sized pin is the parent pin: the table is used as loaded
        x = torch.randn(1, 3, 224, 224, generator=gen)
        assert torch.equal(pin(x), type(pin).__mro__[1].forward(pin, x))
