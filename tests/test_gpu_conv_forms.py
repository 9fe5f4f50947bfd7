"""The implicit-GEMM convolution of csrc/conv_igemm.hip, instantiation by instantiation, against float64 on the CPU.

One table (CASES) names, for every case, the geometry, the fused epilogue, the option overrides and the LITERAL profiler row
the launch must produce: conv_igemm<BM,BN,BK,nhwc|nchw[,pool2][,gate][,pw][,splitk|,k4]>. A case runs under the profiler,
must produce exactly that row once (plus one conv_splitk_reduce row where the name ends in ,splitk), runs again and must
repeat its bits. conv_rgemm and conv_bf3 are 0 for the whole file, so the implicit-GEMM kernel is what runs.

Reference: ref_conv of tests/test_gpu_ops.py (F.conv2d + the epilogue) in float64; e32 is the error of the identical
evaluation in float32 on the CPU. Gate: gate() of tests/test_gpu_vit_ops.py, max |got - ref64| <= max(4 e32, 8 u max |ref64|),
u = 2^-24. Every output is NaN-filled and followed by a sentinel tail (Guarded of tests/test_gpu_se_path.py): no NaN may
remain and the tail must come back untouched. Two input families per case: `normal` (zero-mean Gaussians) and `one_sign`
(x, w, gate, residual, scale and shift positive and bounded away from 0: a dropped K step has no cancellation to hide behind;
tests/test_conv_forms_reference.py shows on the CPU that the smallest 8-deep K-group of every such case moves an output by
at least 100 gates). The two `neg` pool2 cases are one_sign with a shift below -3: every pre-activation is negative, so the
-INFINITY start of the fused max is what act = 0 returns a maximum over, and ReLU must return exact zeros.

The SiLU cases are held to the same gate, although the kernel's SiLU goes through v_exp_f32 / v_rcp_f32: none of them needed
the wider elementwise gate of tests/test_gpu_se_path.py (figures below).

Statistics (orbit_op_conv2d_train, STATS_CASES): *stat_blocks == ceil(M / BM) of the form that ran, and every column sum / sum
of squares within 2 n u A of the float64 sums of the outputs the kernel wrote (the summation bound of test_gpu_se_path.py).

What the launch rules make of the table (found while writing it; the profiler assertion is the check):
  * conv_splitk takes every conv with Cout > 32 and >= 16 K-tiles on a small map - a 3x3 from 64, 48 or 24 channels included - so
    the whole-tile KxK cases set conv_splitk = 0;
  * Cout = 68 never reaches the heuristic's 32x32 choice: the waste rule (128 - 96) / 68 >= 0.15 hands it to 128x32 first
    (case k3_rule_cout68_is_128x32). The heuristic's ,k4 is reached with Cout = 36, Cout = 68 runs it under conv_tile = 6;
  * a pointwise conv has no padding, so the stride-2 pointwise cases cannot have pad_t != pad_l; nor can the ResNet stem
    (7x7/2, pad 3) and the 8x160 stem_fast shape (TF-SAME pads nothing in front of an even size).
KH != KW (3x1 and 1x3, padded on the long side only) is computed correctly; nothing had to be fixed or refused.

Largest err / e32 per tile form on the MI355X where 4 e32 is the bound, largest err / (8 u max |ref64|) where the floor is
(each case prints "[conv-forms] name/family: err, e32, err/e32"; run with -s):
  64x64       err / e32 3.49  (pool_11x9_drops_last_row_col/normal)    floor: err 8.1e-07, 0.79 of it (k3_64x64_bk8_cout4/normal)
  128x32      err / e32 3.15  (k3_rule_cout68_is_128x32/one_sign)      floor: err 5.0e-07, 0.25 of it (stem3_same_128x32/normal)
  32x32,k4    err / e32 1.46  (k3_k4_forced_cout68/normal)             floor: never the bound
No SiLU case needed the elementwise gate: the largest SiLU ratio is the 128x32 row's 3.15 err / e32. The
statistics sit within 0.07 of their bound 2 n u A. Every case named the instantiation the table gives it, and no case failed.
"""
import ctypes
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from test_gpu_ops import nchw, nhwc, ref_conv  # noqa: E402
from test_gpu_se_path import Guarded, options  # noqa: E402
from test_gpu_vit_ops import U, _prof_rows, gate  # noqa: E402

RELU, SILU = 1, 2


def _st():
    return _lib.stream_handle()


def C(name, geom, expect, epi="", **opts):
    """One case. geom = (B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo); epi: comma-separated subset of scale, shift,
    res, gate, relu, silu, pool2, nchw, neg (one_sign only, shift below -3); opts: conv_tile / conv_bk / conv_splitk."""
    flags = set(f for f in epi.split(",") if f)
    assert flags <= {"scale", "shift", "res", "gate", "relu", "silu", "pool2", "nchw", "neg"}, flags
    assert set(opts) <= {"conv_tile", "conv_bk", "conv_splitk"}, opts
    return {"name": name, "geom": geom, "flags": flags, "opts": opts, "expect": expect,
            "act": RELU if "relu" in flags else SILU if "silu" in flags else 0}


BN = "scale,shift"
# Maps: 5x13 = 65 rows, 3x43 = 129, 10x13 = 130, 3x11 = 33, 3 x 2x3 = 18, 3 x 1x25 = 75 (a 64-row tile spans three frames' gates and
# the clamped rows beyond M sit in the last frame). Stride 2 on H even, W odd: TF-SAME pads (0, 1) for 3x3 and (1, 2) for 5x5.
CASES = [
    # ---- NHWC 3x3, no gate: 64x64 at BK 32 / 16 / 8
    C("k3_64x64_bk32", (1, 64, 5, 13, 68, 3, 3, 1, 1, 1, 5, 13), "conv_igemm<64,64,32,nhwc>", BN + ",relu", conv_tile=3, conv_splitk=0),
    C("k3_64x64_bk16", (3, 48, 2, 3, 36, 3, 3, 1, 1, 1, 2, 3), "conv_igemm<64,64,16,nhwc>", BN + ",res,relu", conv_splitk=0),
    C("k3_64x64_bk8", (1, 24, 5, 13, 36, 3, 3, 1, 1, 1, 5, 13), "conv_igemm<64,64,8,nhwc>", BN + ",silu", conv_splitk=0),
    C("k3_64x64_bk8_cout4", (3, 24, 2, 3, 4, 3, 3, 1, 1, 1, 2, 3), "conv_igemm<64,64,8,nhwc>", "shift", conv_tile=3),
    # 128x32: by the rule (Cout <= 32; Cout = 80 and 68, the waste rule) and forced
    C("k3_128x32_bk32_rule_cout4", (1, 64, 3, 43, 4, 3, 3, 1, 1, 1, 3, 43), "conv_igemm<128,32,32,nhwc>", BN + ",res"),
    C("k3_128x32_bk16_rule_cout80", (3, 48, 2, 3, 80, 3, 3, 1, 1, 1, 2, 3), "conv_igemm<128,32,16,nhwc>", BN + ",relu", conv_splitk=0),
    C("k3_128x32_bk8_forced", (1, 24, 3, 43, 36, 3, 3, 1, 1, 1, 3, 43), "conv_igemm<128,32,8,nhwc>", "scale", conv_tile=4, conv_splitk=0),
    C("k3_rule_cout68_is_128x32", (3, 64, 4, 5, 68, 3, 3, 1, 1, 1, 4, 5), "conv_igemm<128,32,32,nhwc>", BN + ",silu", conv_splitk=0),
    # 32x32 with four K-waves: by the rule (fewer than 256 64x64 tiles) and forced
    C("k3_k4_rule", (1, 64, 3, 11, 36, 3, 3, 1, 1, 1, 3, 11), "conv_igemm<32,32,32,nhwc,k4>", BN + ",res,relu", conv_splitk=0),
    C("k3_k4_forced_cout68", (3, 64, 2, 3, 68, 3, 3, 1, 1, 1, 2, 3), "conv_igemm<32,32,32,nhwc,k4>", BN + ",silu", conv_tile=6, conv_splitk=0),
    C("k3_k4_forced_cout4", (1, 32, 3, 11, 4, 3, 3, 1, 1, 1, 3, 11), "conv_igemm<32,32,32,nhwc,k4>", "", conv_tile=6),
    C("k3_s2_k4_forced", (3, 64, 8, 11, 68, 3, 3, 2, 0, 1, 4, 6), "conv_igemm<32,32,32,nhwc,k4>", BN + ",relu", conv_tile=6, conv_splitk=0),
    # conv_tile = 6 below BK 32 falls through to the rule
    C("k3_tile6_bk16_falls_through", (1, 48, 5, 13, 36, 3, 3, 1, 1, 1, 5, 13), "conv_igemm<64,64,16,nhwc>", BN, conv_tile=6, conv_splitk=0),
    # ---- cin_pad > Cin (12 -> 16, 20 -> 24): the K-padding predicate; UL = false on the pointwise form
    C("pw_cin12", (3, 12, 3, 7, 36, 1, 1, 1, 0, 0, 3, 7), "conv_igemm<64,64,8,nhwc,pw>", BN + ",silu"),
    C("pw_cin20", (1, 20, 5, 13, 4, 1, 1, 1, 0, 0, 5, 13), "conv_igemm<128,32,8,nhwc,pw>", BN),
    C("k3_cin12", (1, 12, 5, 13, 36, 3, 3, 1, 1, 1, 5, 13), "conv_igemm<64,64,8,nhwc>", BN + ",relu", conv_splitk=0),
    C("k3_cin20", (3, 20, 2, 3, 68, 3, 3, 1, 1, 1, 2, 3), "conv_igemm<64,64,8,nhwc>", BN + ",res", conv_tile=3, conv_splitk=0),
    # ---- pointwise
    C("pw_64x64_bk32", (1, 64, 5, 13, 68, 1, 1, 1, 0, 0, 5, 13), "conv_igemm<64,64,32,nhwc,pw>", BN + ",silu", conv_tile=3),
    C("pw_64x64_bk16", (3, 48, 2, 3, 36, 1, 1, 1, 0, 0, 2, 3), "conv_igemm<64,64,16,nhwc,pw>", BN + ",res"),
    C("pw_128x32_bk32", (1, 160, 3, 43, 4, 1, 1, 1, 0, 0, 3, 43), "conv_igemm<128,32,32,nhwc,pw>", BN + ",relu"),
    C("pw_k4_rule", (1, 64, 3, 11, 36, 1, 1, 1, 0, 0, 3, 11), "conv_igemm<32,32,32,nhwc,pw,k4>", BN + ",silu"),
    C("pw_bk16_override_32to16", (1, 32, 10, 13, 16, 1, 1, 1, 0, 0, 10, 13), "conv_igemm<128,32,16,nhwc,pw>", BN),
    C("pw_s2_7x9_ul", (3, 48, 7, 9, 36, 1, 1, 2, 0, 0, 4, 5), "conv_igemm<64,64,16,nhwc,pw>", BN + ",relu"),
    C("pw_s2_7x9_cin20", (1, 20, 7, 9, 36, 1, 1, 2, 0, 0, 4, 5), "conv_igemm<64,64,8,nhwc,pw>", BN),
    # ---- gated pointwise, B = 3, Ho * Wo = 25
    C("gpw_64x64_bk32", (3, 64, 1, 25, 68, 1, 1, 1, 0, 0, 1, 25), "conv_igemm<64,64,32,nhwc,gate,pw>", BN + ",gate", conv_tile=3),
    C("gpw_64x64_bk16", (3, 48, 1, 25, 36, 1, 1, 1, 0, 0, 1, 25), "conv_igemm<64,64,16,nhwc,gate,pw>", BN + ",gate,res"),
    C("gpw_64x64_bk8", (3, 24, 1, 25, 36, 1, 1, 1, 0, 0, 1, 25), "conv_igemm<64,64,8,nhwc,gate,pw>", BN + ",gate,silu"),
    C("gpw_128x32_bk16_override_96to24", (3, 96, 1, 25, 24, 1, 1, 1, 0, 0, 1, 25), "conv_igemm<128,32,16,nhwc,gate,pw>", BN + ",gate"),
    C("gpw_k4", (3, 64, 1, 25, 36, 1, 1, 1, 0, 0, 1, 25), "conv_igemm<32,32,32,nhwc,gate,pw,k4>", BN + ",gate,res"),
    C("gpw_cin20", (3, 20, 1, 25, 36, 1, 1, 1, 0, 0, 1, 25), "conv_igemm<64,64,8,nhwc,gate,pw>", BN + ",gate"),
    # ---- gated 3x3
    C("gk3_40to48", (3, 40, 4, 5, 48, 3, 3, 1, 1, 1, 4, 5), "conv_igemm<64,64,8,nhwc,gate>", BN + ",gate,silu", conv_splitk=0),
    # ---- fused 2x2 max-pool
    C("pool_12x10", (1, 64, 12, 10, 64, 3, 3, 1, 1, 1, 12, 10), "conv_igemm<64,64,32,nhwc,pool2>", BN + ",relu,pool2"),
    C("pool_11x9_drops_last_row_col", (3, 64, 11, 9, 64, 3, 3, 1, 1, 1, 11, 9), "conv_igemm<64,64,32,nhwc,pool2>", BN + ",relu,pool2"),
    C("pool_128x32", (1, 64, 12, 10, 32, 3, 3, 1, 1, 1, 12, 10), "conv_igemm<128,32,32,nhwc,pool2>", BN + ",silu,pool2"),
    C("pool_neg_relu", (1, 64, 11, 9, 36, 3, 3, 1, 1, 1, 11, 9), "conv_igemm<64,64,32,nhwc,pool2>", BN + ",relu,pool2,neg"),
    C("pool_neg_act0", (1, 64, 11, 9, 36, 3, 3, 1, 1, 1, 11, 9), "conv_igemm<64,64,32,nhwc,pool2>", BN + ",pool2,neg"),
    # ---- NCHW stems. stem7_14x224 and stem3_8x160_64x64 have 64-row waves on both sides of the interior fast path
    C("stem7_14x224", (1, 3, 14, 224, 64, 7, 7, 2, 3, 3, 7, 112), "conv_igemm<64,64,32,nchw>", BN + ",relu,nchw"),
    C("stem7_9x13", (3, 3, 9, 13, 64, 7, 7, 2, 3, 3, 5, 7), "conv_igemm<64,64,32,nchw>", BN + ",relu,nchw"),
    C("stem3_same_128x32", (3, 3, 8, 11, 32, 3, 3, 2, 0, 1, 4, 6), "conv_igemm<128,32,32,nchw>", BN + ",silu,nchw"),
    C("stem3_8x160_64x64", (2, 3, 8, 160, 32, 3, 3, 2, 0, 0, 4, 80), "conv_igemm<64,64,32,nchw>", BN + ",silu,nchw", conv_tile=3),
    C("stem_pool_even", (3, 3, 8, 6, 64, 3, 3, 1, 1, 1, 8, 6), "conv_igemm<64,64,32,nchw,pool2>", BN + ",relu,pool2,nchw"),
    C("stem_pool_odd", (1, 3, 9, 7, 64, 3, 3, 1, 1, 1, 9, 7), "conv_igemm<64,64,32,nchw,pool2>", BN + ",relu,pool2,nchw"),
    C("stem_pool_14x38", (1, 3, 14, 38, 64, 3, 3, 1, 1, 1, 14, 38), "conv_igemm<64,64,32,nchw,pool2>", BN + ",relu,pool2,nchw"),
    # ---- split-K (K-tiles per range in SPLITK_RANGES below): the reduce kernel's epilogue with SiLU, scale only, shift only,
    # residual + ReLU, residual alone
    C("sk_s3_short_last_512pw_gate", (3, 512, 1, 25, 36, 1, 1, 1, 0, 0, 1, 25), "conv_igemm<64,64,32,nhwc,gate,pw,splitk>", BN + ",gate,silu"),
    C("sk_s3_even_64to36", (1, 64, 5, 6, 36, 3, 3, 1, 1, 1, 5, 6), "conv_igemm<64,64,32,nhwc,splitk>", "scale"),
    C("sk_s4_midtap_96to68", (3, 96, 2, 3, 68, 3, 3, 1, 1, 1, 2, 3), "conv_igemm<64,64,32,nhwc,splitk>", "shift"),
    C("sk_bk16_48", (1, 48, 5, 13, 36, 3, 3, 1, 1, 1, 5, 13), "conv_igemm<64,64,16,nhwc,splitk>", BN + ",res,relu"),
    C("sk_bk8_24_5x5", (3, 24, 4, 5, 68, 5, 5, 1, 2, 2, 4, 5), "conv_igemm<64,64,8,nhwc,splitk>", BN + ",res"),
    # ---- 5x5 stride 2, TF-SAME (1, 2) on a 10x13 map; KH != KW, padded on the long side only
    C("k5_s2_same_10x13", (1, 24, 10, 13, 36, 5, 5, 2, 1, 2, 5, 7), "conv_igemm<64,64,8,nhwc>", BN + ",silu", conv_splitk=0),
    C("k3x1", (1, 64, 5, 13, 36, 3, 1, 1, 1, 0, 5, 13), "conv_igemm<32,32,32,nhwc,k4>", BN + ",relu"),
    C("k1x3", (3, 24, 2, 3, 36, 1, 3, 1, 0, 1, 2, 3), "conv_igemm<64,64,8,nhwc>", BN + ",relu"),
]
CASE_IDS = [c["name"] for c in CASES]

# K-tiles per split range, as (Cin, KH * KW, BK) give them by arithmetic (tests/test_conv_forms_reference.py): S ranges of
# ceil(tiles / S). sk_s4_midtap: range 1 starts at K-tile 7 = tap 2, channel 32.
SPLITK_RANGES = {"sk_s3_short_last_512pw_gate": [6, 6, 4], "sk_s3_even_64to36": [6, 6, 6], "sk_s4_midtap_96to68": [7, 7, 7, 6],
                 "sk_bk16_48": [7, 7, 7, 6], "sk_bk8_24_5x5": [19, 19, 19, 18]}
STEM_FAST_CASES = ("stem7_14x224", "stem3_8x160_64x64", "stem_pool_14x38")
# stride-2 cases the issue fixes with pad_t == pad_l (module docstring)
SYMMETRIC_STRIDE2 = ("pw_s2_7x9_ul", "pw_s2_7x9_cin20", "stem7_14x224", "stem7_9x13", "stem3_8x160_64x64")

# name, geometry, gated, nchw, conv_tile, row the launch must produce, BM
STATS_CASES = [
    ("st_rule_64x64_bk8", (1, 24, 5, 13, 36, 3, 3, 1, 1, 1, 5, 13), False, 0, 0, "conv_igemm<64,64,8,nhwc>", 64),
    ("st_rule_k4", (3, 64, 3, 7, 36, 3, 3, 1, 1, 1, 3, 7), False, 0, 0, "conv_igemm<32,32,32,nhwc,k4>", 32),
    ("st_64x64_bk32", (1, 64, 5, 13, 68, 3, 3, 1, 1, 1, 5, 13), False, 0, 3, "conv_igemm<64,64,32,nhwc>", 64),
    ("st_128x32_bk16", (1, 48, 3, 43, 36, 3, 3, 1, 1, 1, 3, 43), False, 0, 4, "conv_igemm<128,32,16,nhwc>", 128),
    ("st_k4_cout68", (1, 64, 3, 11, 68, 3, 3, 1, 1, 1, 3, 11), False, 0, 6, "conv_igemm<32,32,32,nhwc,k4>", 32),
    ("st_gpw_64x64", (3, 64, 1, 25, 68, 1, 1, 1, 0, 0, 1, 25), True, 0, 3, "conv_igemm<64,64,32,nhwc,gate,pw>", 64),
    ("st_gpw_128x32", (3, 96, 1, 43, 24, 1, 1, 1, 0, 0, 1, 43), True, 0, 4, "conv_igemm<128,32,16,nhwc,gate,pw>", 128),
    ("st_stem3_128x32", (3, 3, 8, 11, 32, 3, 3, 2, 0, 1, 4, 6), False, 1, 0, "conv_igemm<128,32,32,nchw>", 128),
]


def families(case):
    return ("one_sign",) if "neg" in case["flags"] else ("normal", "one_sign")


def conv_inputs(name, geom, flags, family):
    """fp32 CPU tensors of one case: x NCHW, w OIHW, scale / shift [Cout], res NCHW, gate [B][Cin] (None where unused)."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)
    K = Cin * KH * KW
    if family == "normal":
        t = {"x": torch.randn(B, Cin, H, W, generator=g), "w": torch.randn(Cout, Cin, KH, KW, generator=g) / K ** 0.5,
             "scale": torch.rand(Cout, generator=g) + 0.5, "shift": torch.randn(Cout, generator=g) * 0.1,
             "res": torch.randn(B, Cout, Ho, Wo, generator=g), "gate": torch.rand(B, Cin, generator=g)}
    else:
        assert family == "one_sign"
        t = {"x": torch.rand(B, Cin, H, W, generator=g) + 0.5, "w": (torch.rand(Cout, Cin, KH, KW, generator=g) + 0.5) / K,
             "scale": torch.rand(Cout, generator=g) + 0.5, "shift": torch.rand(Cout, generator=g) * 0.5 + 0.5,
             "res": torch.rand(B, Cout, Ho, Wo, generator=g) + 0.5, "gate": torch.rand(B, Cin, generator=g) * 0.5 + 0.5}
        if "neg" in flags:
            t["shift"] = -3.0 - t["shift"]
    for k in ("scale", "shift", "res", "gate"):
        if k not in flags:
            t[k] = None
    return t


def reference(geom, flags, act, t, dtype, w=None):
    """ref_conv of the case in `dtype`, NCHW (pooled where pool2); `w` replaces the filter (the K-group margins)."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    c = lambda v: None if v is None else v.to(dtype)  # noqa: E731
    return ref_conv(c(t["x"]), c(t["w"] if w is None else w), stride, pad_t, pad_l, Ho, Wo, scale=c(t["scale"]), shift=c(t["shift"]),
                    residual=c(t["res"]), gate=c(t["gate"]), act=act, pool2=1 if "pool2" in flags else 0)


def tolerance(ref64, ref32):
    """(e32, the module's gate) from the two CPU references alone."""
    e32 = (ref32.double() - ref64).abs().max().item()
    return e32, max(4 * e32, 8 * U * ref64.abs().max().item())


def form_of(expect):
    """'64x64', '128x32' or '32x32,k4' from a profiler row."""
    f = expect[len("conv_igemm<"):-1].split(",")
    return "%sx%s%s" % (f[0], f[1], ",k4" if "k4" in f else "")


_worst = {}  # (tile form, "4e32" | "floor") -> largest err / that bound's unit


def report(name, expect, got, ref64, e32):
    err = (got.double() - ref64).abs().max().item()
    floor = 8 * U * ref64.abs().max().item()
    key = (form_of(expect), "4e32" if 4 * e32 >= floor else "floor")
    unit = e32 if key[1] == "4e32" else floor
    if unit > 0:
        _worst[key] = max(_worst.get(key, 0.0), err / unit)
    print("\n[conv-forms] %s: err %.3g, e32 %.3g, err/e32 %.2f   (worst %s: %s)"
          % (name, err, e32, err / e32 if e32 > 0 else 0.0, form_of(expect),
             ", ".join("err/%s %.2f" % (k[1], v) for k, v in sorted(_worst.items()) if k[0] == key[0])))
    return err


def upload(device, geom, flags, t):
    d = {k: (None if v is None else v.to(device).contiguous()) for k, v in t.items()}
    d["x"] = (t["x"] if "nchw" in flags else nhwc(t["x"])).to(device).contiguous()
    if t["res"] is not None:
        d["res"] = nhwc(t["res"]).to(device)
    return d


def run_conv(lib, device, geom, flags, act, d):
    """orbit_op_conv2d into a guarded buffer; the result NCHW on the CPU after the guard checks."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    pool2 = 1 if "pool2" in flags else 0
    y = Guarded((B, Ho // 2, Wo // 2, Cout) if pool2 else (B, Ho, Wo, Cout), device)
    p = _lib.dptr
    _lib.check(lib.orbit_op_conv2d(p(d["x"]), 1 if "nchw" in flags else 0, p(d["w"]), p(y.t), p(d["scale"]), p(d["shift"]), p(d["res"]),
                                   p(d["gate"]), B, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, act, pool2, _st()),
               "orbit_op_conv2d")
    torch.cuda.synchronize()
    return nchw(y.cpu("y"))


def profiled(lib, fn):
    """(fn(), {conv_* profiler row: launches}) of one call under the profiler."""
    lib.orbit_prof_enable(1)
    try:
        out = fn()
        rows = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    return out, {k: v for k, v in rows.items() if k.startswith("conv_")}


@pytest.fixture(scope="module", autouse=True)
def igemm_only(lib):
    """conv_rgemm = 0 and conv_bf3 = 0 for the whole file: the implicit-GEMM kernel runs; both come back afterwards."""
    with options(lib, conv_rgemm=0, conv_bf3=0):
        yield


PARAMS = [pytest.param(c, f, id="%s-%s" % (c["name"], f)) for c in CASES for f in families(c)]


@pytest.mark.parametrize("case,family", PARAMS)
def test_conv_form(lib, device, case, family):
    name, geom, flags, act, expect = case["name"], case["geom"], case["flags"], case["act"], case["expect"]
    what = "%s/%s" % (name, family)
    t = conv_inputs(name, geom, flags, family)
    ref64 = reference(geom, flags, act, t, torch.float64)
    e32, _ = tolerance(ref64, reference(geom, flags, act, t, torch.float32))
    d = upload(device, geom, flags, t)
    split = expect.endswith(",splitk>")
    with options(lib, **dict({"conv_tile": 0, "conv_bk": 0, "conv_splitk": 1}, **case["opts"])):
        got, rows = profiled(lib, lambda: run_conv(lib, device, geom, flags, act, d))
        assert rows == dict({expect: 1}, **({"conv_splitk_reduce": 1} if split else {})), (what, rows)
        again = run_conv(lib, device, geom, flags, act, d)
        assert torch.equal(got, again), what + ": two runs differ in bits"
        assert got.shape == ref64.shape
        report(what, expect, got, ref64, e32)
        gate(got, ref64, e32, what)
        if split:  # the unsplit kernel sums in another order: close, and not the same bits
            with options(lib, conv_splitk=0):
                unsplit, urows = profiled(lib, lambda: run_conv(lib, device, geom, flags, act, d))
            assert "conv_splitk_reduce" not in urows and not any(k.endswith(",splitk>") for k in urows), urows
            gate(unsplit, ref64, e32, what + " (conv_splitk = 0)")
            assert not torch.equal(got, unsplit), what + ": split-K produced the unsplit kernel's bits"
    if "neg" in flags:
        assert bool((ref64 < 0).all()) if act == 0 else bool((got == 0).all())


@pytest.mark.parametrize("family", ["normal", "one_sign"])
@pytest.mark.parametrize("name,geom,gated,x_nchw,tile,expect,BM", STATS_CASES, ids=[c[0] for c in STATS_CASES])
def test_conv_statistics_epilogue(lib, device, name, geom, gated, x_nchw, tile, expect, BM, family):
    """ConvParams::stats on every tile form: the raw conv output against float64, one partial per row block of the form that
    ran, and the reduced column sums / sums of squares against the float64 sums of what the kernel wrote."""
    B, Cin, H, W, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo = geom
    flags = set(["gate"] if gated else []) | set(["nchw"] if x_nchw else [])
    what = "%s/%s" % (name, family)
    t = conv_inputs(name, geom, flags, family)
    ref64 = reference(geom, flags, 0, t, torch.float64)
    e32, _ = tolerance(ref64, reference(geom, flags, 0, t, torch.float32))
    d = upload(device, geom, flags, t)
    M = B * Ho * Wo

    def run():
        y, stats = Guarded((B, Ho, Wo, Cout), device), Guarded((2, Cout), device)
        nblk = ctypes.c_int(-1)
        p = _lib.dptr
        _lib.check(lib.orbit_op_conv2d_train(p(d["x"]), x_nchw, p(d["w"]), p(y.t), p(d["gate"]), B, H, W, Cin, Cout, KH, KW, stride,
                                             pad_t, pad_l, Ho, Wo, p(stats.t), ctypes.byref(nblk), _st()), "orbit_op_conv2d_train")
        torch.cuda.synchronize()
        return y.cpu("y"), stats.cpu("stats"), nblk.value

    with options(lib, conv_tile=tile, conv_bk=0):
        (y, stats, nblk), rows = profiled(lib, run)
        y2, stats2, _ = run()
    assert {k: v for k, v in rows.items() if k.startswith("conv_igemm")} == {expect: 1}, (what, rows)
    assert nblk == -(-M // BM), (what, nblk, M, BM)
    assert torch.equal(y, y2) and torch.equal(stats, stats2), what + ": two runs differ in bits"
    report(what, expect, nchw(y), ref64, e32)
    gate(nchw(y), ref64, e32, what)
    yd = y.double().reshape(M, Cout)
    for k, v in enumerate((yd, yd * yd)):
        S, A = v.sum(0), v.abs().sum(0)
        err, bound = (stats[k].double() - S).abs(), 2.0 * M * U * A
        print("[conv-forms] %s: %s within %.3g of its bound 2 n u A" % (what, ("column sums", "sums of squares")[k], (err / bound).max().item()))
        assert not (err > bound).any(), (what, k, (err / bound).max().item())
