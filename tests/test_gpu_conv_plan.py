"""The two kernel families tests/test_gpu_conv_forms.py switches off, against the plan: with conv_rgemm = 2 a pointwise and a gated
pointwise conv, with conv_bf3 = 1 a pointwise and a 3x3 conv must each produce, under the profiler, exactly the one row
orbit_op_conv2d_plan (host only; conv_plan of csrc/conv_igemm.hip) names for the launch. The shapes are the smallest that
tests/test_gpu_ops.py runs on these kernels (RGEMM_CASES, BF3_CASES, BF3_GENERAL_CASES); what they compute is checked there."""
import pytest

pytestmark = pytest.mark.gpu

import test_gpu_conv_forms as T  # noqa: E402
from test_conv_forms_reference import plan  # noqa: E402

# name, options, family prefix, geom (B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo), epilogue
CASES = [
    ("rgemm_pw_16to44", dict(conv_rgemm=2, conv_bf3=0), "conv_pw_rgemm<", (2, 16, 9, 5, 44, 1, 1, 1, 0, 0, 9, 5), "scale,shift,relu"),
    ("rgemm_gated_32to64", dict(conv_rgemm=2, conv_bf3=0), "conv_pw_rgemm<", (1, 32, 3, 3, 64, 1, 1, 1, 0, 0, 3, 3), "scale,shift,gate"),
    ("bf3_pw_96to44", dict(conv_rgemm=0, conv_bf3=1), "conv_bf3<", (2, 96, 9, 5, 44, 1, 1, 1, 0, 0, 9, 5), "scale,shift,res"),
    ("bf3_k3_64to64", dict(conv_rgemm=0, conv_bf3=1), "conv_bf3<", (3, 64, 14, 14, 64, 3, 3, 1, 1, 1, 14, 14), "scale,shift,res,relu"),
]


@pytest.mark.parametrize("name,opts,prefix,geom,epi", CASES, ids=[c[0] for c in CASES])
def test_launch_produces_the_row_the_plan_names(lib, device, name, opts, prefix, geom, epi):
    flags = set(epi.split(","))
    act = T.RELU if "relu" in flags else 0
    d = T.upload(device, geom, flags, T.conv_inputs(name, geom, flags, "normal"))
    with T.options(lib, **opts):
        rc, row, ksplit, per, m_tiles = plan(lib, geom, gated=int("gate" in flags), residual=int("res" in flags))
        assert rc == 0 and row.startswith(prefix) and (ksplit, per, m_tiles) == (1, 0, 0), (rc, row, ksplit, per, m_tiles)
        assert ("gate" in row) == ("gate" in flags)
        _, rows = T.profiled(lib, lambda: T.run_conv(lib, device, geom, flags, act, d))
    assert rows == {row: 1}, (name, row, rows)
