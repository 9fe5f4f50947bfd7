"""CPU-side checks of the opt-in bf16 inference mode of the transformer extractors: the C-ABI declares and binds the new
symbols, the plan flag and its refusals need no device, the learner's --vit_bf16 is refused where a gradient would be needed,
the module refuses before a plan is built, and the emulation helper of the GPU test rounds as the kernel promises."""
import ctypes
import os
import re

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

from vit_bf16_emulation import emulate_bf16_linears, round_bf16
import vit_pin

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbit_hip.h")
P = ctypes.c_void_p
DECLARED = {
    "orbit_vit_enable_bf16": ("int", ["orbit_vit_t*"], (ctypes.c_int, [P])),
    "orbit_vit_bf16_enabled": ("int", ["const orbit_vit_t*"], (ctypes.c_int, [P])),
    "orbit_op_vit_pack_bf16": ("int", ["const float*", "uint16_t*", "size_t", "orbit_stream_t"],
                               (ctypes.c_int, [P, P, ctypes.c_size_t, P])),
    "orbit_op_vit_linear_bf16": ("int", ["const float*", "const uint16_t*", "const float*", "const float*", "float*", "int", "int",
                                         "int", "int", "int", "orbit_stream_t"], (ctypes.c_int, [P] * 5 + [ctypes.c_int] * 5 + [P])),
}


def test_header_declares_and_lib_binds_the_new_symbols(lib):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name, (ret, params, (restype, argtypes)) in DECLARED.items():
        m = re.search(r"(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/orbit_hip.h" % name
        assert m.group(1).split() == ret.split(), (name, m.group(1))
        got = [re.sub(r"\s*\b\w+$", "", " ".join(p.split())) for p in m.group(2).split(",")]  # drop the parameter names
        assert got == params, (name, got)
        assert _lib._SIGNATURES[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def test_plan_flag_and_its_refusals_need_no_device(lib):
    def create(name):
        h = P()
        assert lib.orbit_vit_create(name.encode(), 224, 224, ctypes.byref(h)) == 0, _lib.last_error()
        return h

    for name in ("vit_s_32", "vit_b_32", "vit_b_32_clip", "vit_s_16", "vit_b_16", "vit_b_16_clip"):
        h, taped = create(name), create(name)
        try:
            assert lib.orbit_vit_bf16_enabled(h) == 0
            ws, macs = lib.orbit_vit_workspace_bytes(h, 7), lib.orbit_vit_macs_per_frame(h)
            assert lib.orbit_vit_enable_bf16(h) == 0 and lib.orbit_vit_enable_bf16(h) == 0  # before finalize, idempotent
            assert lib.orbit_vit_bf16_enabled(h) == 1
            assert lib.orbit_vit_workspace_bytes(h, 7) == ws and lib.orbit_vit_macs_per_frame(h) == macs
            for enable in (lib.orbit_vit_enable_backward, lib.orbit_vit_enable_weight_backward):
                assert enable(h) == -1 and "orbit_vit_enable_bf16" in _lib.last_error()
            buf = (ctypes.c_float * 64)()
            q = P(ctypes.addressof(buf))
            assert lib.orbit_vit_train_forward(h, q, 1, None, None, q, q, 1 << 40, q, 1 << 40, None) == -1
            assert "orbit_vit_enable_bf16" in _lib.last_error()
            assert lib.orbit_vit_backward(h, 1, None, None, q, q, 1 << 40, q, q, q, 1 << 40, None) == -1
            assert "orbit_vit_enable_bf16" in _lib.last_error()
            assert lib.orbit_vit_backward_params(h, q, 1, None, None, q, q, 1 << 40, q, q, q, q, 1 << 40, None) == -1
            assert "orbit_vit_enable_bf16" in _lib.last_error()
            assert lib.orbit_vit_enable_weight_backward(taped) == 0
            assert lib.orbit_vit_enable_bf16(taped) == -1 and "orbit_vit_enable_weight_backward" in _lib.last_error()
            assert lib.orbit_vit_bf16_enabled(taped) == 0
        finally:
            lib.orbit_vit_destroy(h)
            lib.orbit_vit_destroy(taped)
    assert lib.orbit_vit_enable_bf16(None) == -1 and lib.orbit_vit_bf16_enabled(None) == 0


def test_operator_entry_points_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, odd = P(base), P(base + 4)

    def refused(rc, *words):
        assert rc == -1, rc
        assert all(w in _lib.last_error() for w in words), _lib.last_error()

    lin = lib.orbit_op_vit_linear_bf16
    refused(lin(p, p, p, None, p, 50, 384, 384 + 32, 0, 0, None), "multiple", "K=416", "N=384", "M=50")  # K % 64 (fp32 takes it)
    refused(lin(p, p, p, None, p, 50, 384 + 64, 384, 0, 0, None), "multiple", "N=448")
    refused(lin(p, p, p, None, p, 0, 384, 384, 0, 0, None), "shape")
    refused(lin(p, p, p, None, p, 50, 384, 384, 0, 96, None), "tile_rows")
    refused(lin(p, p, p, None, p, 50, 384, 384, 3, 0, None), "epilogue")
    refused(lin(p, p, p, None, p, 50, 384, 384, 2, 0, None), "residual")
    refused(lin(p, p, p, p, p, 50, 384, 384, 1, 0, None), "residual")
    refused(lin(odd, p, p, None, p, 50, 384, 384, 0, 0, None), "aligned")
    refused(lin(p, odd, p, None, p, 50, 384, 384, 0, 0, None), "aligned")
    refused(lin(None, p, p, None, p, 50, 384, 384, 0, 0, None), "null")
    refused(lib.orbit_op_vit_pack_bf16(None, p, 8, None), "null")
    refused(lib.orbit_op_vit_pack_bf16(p, p, 0, None), "numel")


def test_learner_flag_is_refused_where_a_gradient_would_be_needed(lib, capsys):
    from orbit_dataset_amd.learner import build_multistep_parser, build_parser, verify_args
    p = build_parser()
    for name in ("vit_s_32", "vit_b_32_clip", "vit_s_16", "vit_b_16_clip"):
        a = p.parse_args(["--mode", "test", "--feature_extractor", name, "--vit_bf16"])
        verify_args(a)
        assert a.vit_bf16 is True
    assert p.parse_args(["--mode", "test", "--feature_extractor", "vit_s_32"]).vit_bf16 is False
    for mode in ("train", "train_test"):
        for opt_in in ([], ["--vit_native_backward"], ["--vit_native_weight_backward", "--learn_extractor"]):
            with pytest.raises(SystemExit, match="vit_bf16"):
                verify_args(p.parse_args(["--feature_extractor", "vit_s_32", "--mode", mode, "--adapt_features", "--vit_bf16"] + opt_in))
    with pytest.raises(SystemExit, match="vit_bf16"):
        verify_args(p.parse_args(["--feature_extractor", "vit_s_16", "--mode", "train", "--adapt_features", "--vit_bf16",
                                  "--vit16_native_backward"]))
    m = build_multistep_parser()
    verify_args(m.parse_args(["--feature_extractor", "vit_s_32", "--vit_bf16"]))
    for flags in (["--adapt_features", "--vit_native_backward"], ["--learn_extractor", "--vit_native_weight_backward"]):
        with pytest.raises(SystemExit, match="vit_bf16"):
            verify_args(m.parse_args(["--feature_extractor", "vit_s_32", "--vit_bf16"] + flags))
    capsys.readouterr()
    a = p.parse_args(["--mode", "train", "--learn_extractor", "--feature_extractor", "resnet18", "--vit_bf16"])
    verify_args(a)  # ignored, even in a training mode: the flag says nothing to a CNN
    out = capsys.readouterr().out
    assert a.vit_bf16 is False and out.count("\n") == 1 and "--vit_bf16 is ignored" in out and "resnet18" in out


@pytest.mark.parametrize("opt_in", [(), ("native_backward",), ("native_weight_backward",), ("native_backward_patch16",),
                                    ("native_weight_backward_patch16",)])
@pytest.mark.parametrize("name", ["vit_s_32", "vit_s_16"])
def test_module_refuses_a_gradient_before_a_plan_is_built(lib, name, opt_in):
    """On the CPU, with no device in reach: the refusal comes before a plan is built or the device is asked for."""
    from orbit_dataset_amd.model.feature_extractors import VisionTransformer, create_feature_extractor
    assert VisionTransformer.bf16_inference is False
    fe, _ = create_feature_extractor(name, with_film=True, learn_extractor=True)
    for attr in opt_in:
        setattr(fe, attr, True)
    plain_key = fe._plan_key(224, 224, False)
    fe.bf16_inference = True
    assert "bf16_inference" in fe.__dict__ and VisionTransformer.bf16_inference is False  # per instance
    assert fe._plan_key(224, 224, False) != plain_key and fe._plan_key(224, 224, False)[:len(plain_key)] == plain_key
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(NotImplementedError, match="bf16_inference"):
        fe(x)  # own parameters require a gradient
    fe.requires_grad_(False)
    g = torch.ones(fe.film_size, requires_grad=True)
    with pytest.raises(NotImplementedError, match="bf16_inference"):
        fe(x, film=(g, torch.zeros_like(g)))
    assert not fe._plans, "a plan was built before the refusal"
    with torch.no_grad():
        assert not fe.wants_grad((g, g))
    fe.bf16_inference = False
    assert fe._plan_key(224, 224, False) == plain_key


def test_emulation_helper_rounds_ties_to_even_and_keeps_dtypes():
    # 1 + 2^-8 is a tie between 1 (even) and 1 + 2^-7 (odd); 1 + 3 * 2^-8 between 1 + 2^-7 (odd) and 1 + 2^-6 (even)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20])
    want = torch.tensor([1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 1 + 2.0 ** -7])
    for dtype in (torch.float32, torch.float64):
        got = round_bf16(ties.to(dtype))
        assert got.dtype == dtype and torch.equal(got, want.to(dtype))
    pin = vit_pin.TimmViT("vit_s_32").eval()
    with torch.no_grad():
        for prm in pin.parameters():
            prm.normal_(0, 0.05)
    before = {k: v.clone() for k, v in pin.state_dict().items()}
    emu = emulate_bf16_linears(pin.double())
    seen = []
    emu.blocks[0].attn.qkv.register_forward_hook(lambda m, args, out: seen.append(args[0]))
    with torch.no_grad():
        out = emu(torch.randn(1, 3, 224, 224, dtype=torch.float64, generator=torch.Generator().manual_seed(0)))
    assert out.dtype == torch.float64 and seen[0].dtype == torch.float64
    assert torch.equal(seen[0], round_bf16(seen[0]))  # the Linear saw a rounded input
    for k, v in emu.state_dict().items():
        assert v.dtype == torch.float64
        linear_weight = k.startswith("blocks.") and k.endswith(".weight") and (".attn." in k or ".mlp." in k)
        assert torch.equal(v, round_bf16(before[k].double()) if linear_weight else before[k].double()), k
