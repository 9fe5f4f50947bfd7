"""GPU parity of the streaming gated projection (csrc/pw_stream.hip; option conv_rgemm != 0) against the path it replaces,
se_gate2 + the LDS-tiled conv kernel (conv_rgemm = 0): bit-identical squeeze-excite gates, projections within 1e-5, the same bits in
any batch, and an EfficientNet-B0 forward that matches the other path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402

# EfficientNet-B0's narrow gated projections at 224x224: (name, H, Cin, Cout, R, chunks, residual)
# (block 3.1, 240 -> 40 @28, stays on se_gate2 + conv: test_layers_left_on_the_pair)
SHAPES = [("b1.0_32x16", 112, 32, 16, 8, 98, False), ("b2.0_96x24", 56, 96, 24, 4, 49, False),
          ("b2.1_144x24", 56, 144, 24, 6, 49, True), ("b3.0_144x40", 28, 144, 40, 6, 14, False)]
OUT_TOL = 1e-5


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    prev = lib.orbit_get_option(b"conv_rgemm")
    yield lib
    lib.orbit_set_option(b"conv_rgemm", prev)


def _inputs(B, H, Cin, Cout, R, chunks, residual, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    t = {"x": r(B, H, H, Cin), "w": r(Cout, Cin, 1, 1) * Cin ** -0.5, "scale": 1.0 + 0.1 * r(Cout), "shift": 0.1 * r(Cout),
         "res": r(B, H, H, Cout) if residual else None,
         # pooling partials of a SiLU activation: column sums of chunks of H * H / chunks pixels
         "partial": (0.3 + 0.5 * r(B, chunks, Cin)) * (H * H / chunks),
         "w1": r(R, Cin) * Cin ** -0.5, "b1": 0.1 * r(R), "w2t": r(R, Cin) * R ** -0.5, "b2": 0.1 * r(Cin)}
    return t


def _run(lib, t, B, H, Cin, Cout, R, chunks, opt):
    lib.orbit_set_option(b"conv_rgemm", opt)
    y = torch.full((B, H, H, Cout), float("nan"), device="cuda")
    gate = torch.full((B, Cin), float("nan"), device="cuda")
    d = _lib.dptr
    _lib.check(lib.orbit_op_pw_stream(d(t["x"]), d(t["w"]), d(t["scale"]), d(t["shift"]),
                                      d(t["res"]) if t["res"] is not None else None, d(t["partial"]), chunks, d(t["w1"]),
                                      d(t["b1"]), d(t["w2t"]), d(t["b2"]), R, d(y), d(gate), B, H, H, Cin, Cout,
                                      _lib.stream_handle()), "orbit_op_pw_stream")
    torch.cuda.synchronize()
    return y, gate


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("name,H,Cin,Cout,R,chunks,residual", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
def test_matches_the_gate_and_conv_pair(device, lib, name, H, Cin, Cout, R, chunks, residual, with_res):
    assert lib.orbit_pw_stream_supported(Cin, Cout, H, H) == 1
    B = 200
    t = _inputs(B, H, Cin, Cout, R, chunks, with_res)
    want_y, want_g = _run(lib, t, B, H, Cin, Cout, R, chunks, 0)
    got_y, got_g = _run(lib, t, B, H, Cin, Cout, R, chunks, 1)
    assert torch.isfinite(want_y).all() and torch.isfinite(got_y).all()
    assert torch.equal(got_g, want_g), f"{name}: gates differ (max {(got_g - want_g).abs().max().item():.3g})"
    err = _rel(got_y, want_y)
    assert err < OUT_TOL, f"{name}: max rel err {err:.3g}"


@pytest.mark.parametrize("name,H,Cin,Cout,R,chunks,residual", SHAPES, ids=[s[0] for s in SHAPES])
def test_same_bits_in_any_batch(device, lib, name, H, Cin, Cout, R, chunks, residual):
    """200 frames in one launch give the bits of 8 launches of 25 (the kernel and its K order are a function of the layer)."""
    B = 200
    t = _inputs(B, H, Cin, Cout, R, chunks, residual, seed=1)
    big, gbig = _run(lib, t, B, H, Cin, Cout, R, chunks, 1)
    parts, gparts = [], []
    for i in range(0, B, 25):
        s = {k: (v[i:i + 25].contiguous() if k in ("x", "res", "partial") and v is not None else v) for k, v in t.items()}
        y, g = _run(lib, s, 25, H, Cin, Cout, R, chunks, 1)
        parts.append(y), gparts.append(g)
    assert torch.equal(big, torch.cat(parts)) and torch.equal(gbig, torch.cat(gparts))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,H,Cin,Cout,R,chunks,residual", SHAPES, ids=[s[0] for s in SHAPES])
def test_small_batches(device, lib, B, name, H, Cin, Cout, R, chunks, residual):
    t = _inputs(B, H, Cin, Cout, R, chunks, residual, seed=2)
    want_y, want_g = _run(lib, t, B, H, Cin, Cout, R, chunks, 0)
    got_y, got_g = _run(lib, t, B, H, Cin, Cout, R, chunks, 1)
    assert torch.equal(got_g, want_g)
    assert _rel(got_y, want_y) < OUT_TOL


@pytest.mark.parametrize("H,Cin,Cout,R,chunks,residual,fused", [
    (100, 32, 16, 8, 50, False, True),    # 200x200 frames, block 1.0: 100 x 100 = 625 tiles of 16 pixels -> streamed
    (50, 144, 24, 6, 25, True, False),    # block 2.1: 50 x 50 = 2500 pixels, not a multiple of 16 -> se_gate2 + conv
    (25, 144, 40, 6, 7, False, False),    # block 3.0: 625 pixels -> se_gate2 + conv
    (28, 240, 40, 10, 14, True, False)])  # block 3.1 at 224x224: no streaming variant (slower there) -> se_gate2 + conv
def test_layers_left_on_the_pair(device, lib, H, Cin, Cout, R, chunks, residual, fused):
    """At 200x200 the 100x100 layer is streamed; the 50x50 and 25x25 layers (H * W % 16 != 0) and 240 -> 40 take the previous
    path, so the option changes nothing there, bit for bit."""
    assert lib.orbit_pw_stream_supported(Cin, Cout, H, H) == int(fused)
    B = 6
    t = _inputs(B, H, Cin, Cout, R, chunks, residual, seed=3)
    want_y, want_g = _run(lib, t, B, H, Cin, Cout, R, chunks, 0)
    got_y, got_g = _run(lib, t, B, H, Cin, Cout, R, chunks, 1)
    assert torch.equal(got_g, want_g)
    if fused:
        assert _rel(got_y, want_y) < OUT_TOL
    else:
        assert torch.equal(got_y, want_y)


@pytest.mark.parametrize("size,n", [(224, 6), (200, 3)])
def test_efficientnet_forward_matches_previous_path(device, lib, size, n):
    """The whole extractor with conv_rgemm 1 vs 0 (graph capture on: the option epoch is part of the graph key). At 0 the
    narrow projections run as se_gate2 + the LDS-tiled conv (and the 1152 -> 320 projection leaves pw_rgemm too)."""
    from orbit_dataset_amd import synthetic
    from orbit_dataset_amd.model.feature_extractors import create_feature_extractor
    fe, _ = create_feature_extractor("efficientnet_b0", True, False, False)
    synthetic.init_parameters_(fe)
    fe = fe.cuda().eval()
    x = torch.randn(n, 3, size, size, device=device, generator=torch.Generator(device=device).manual_seed(5))
    outs = {}
    with torch.no_grad():
        for opt in (0, 1, 0, 1):
            lib.orbit_set_option(b"conv_rgemm", opt)
            out = torch.empty(n, fe.output_size, device=device)
            outs.setdefault(opt, []).append([fe(x, out=out).clone() for _ in range(3)][-1])
    base, got = outs[0][0], outs[1][0]
    assert torch.equal(outs[0][0], outs[0][1]) and torch.equal(outs[1][0], outs[1][1])
    err = (got - base).abs().max().item() / max(1.0, base.abs().max().item())
    assert err < 2e-5, f"efficientnet_b0@{size}: conv_rgemm 1 vs 0 max feature err {err:.3g}"
