// Device helpers shared by the kernel files: the ONLY definition of each. Several bit-identity promises (pw_stream's gate
// equals se_gate2's, the fused fronts equal the conv + depthwise pair, features are batch-invariant) rest on every kernel
// using the same arithmetic in the same order, so a kernel file never keeps a private copy of one of these.
#pragma once
#include "common.h"

namespace orbit {

// wave64 sum on the VALU with DPP lane permutes (quad swaps, half-row / row mirrors, then row broadcasts), result
// broadcast from lane 63: wave-uniform. __shfl_xor lowers to ds_bpermute_b32, an LDS-pipe round trip per step: with 20
// reductions per wave in the head's distance kernel those 120 dependent round trips, not HBM, set the kernel time.
// NOT the summation order of wave_sum_xor: the two are not interchangeable where bits are compared.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = dpp_add<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xf>(v);  // row_half_mirror
    v = dpp_add<0x140, 0xf>(v);  // row_mirror: every lane of a 16-lane row holds the row sum
    v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3: lane 63 holds the wave sum
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// wave64 butterfly reductions (__shfl_xor, offsets 32 .. 1): every lane ends with the result
__device__ __forceinline__ float wave_sum_xor(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max_xor(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// One step of a running argmax over ascending columns c, started from best = -INFINITY, best_c = 0: the FIRST maximal column
// wins, as torch.argmax. The only definition of the rule: the head's `argmax` output and the evaluation metrics
// (csrc/eval.hip) must name the same class for the same logits.
__device__ __forceinline__ void argmax_step(float v, int c, float& best, int& best_c) {
    if (v > best) best = v, best_c = c;
}

// XCD-aware remap: hardware places block i on XCD i % 8, each XCD with its own L2; give each XCD a contiguous run of
// logical blocks so that the blocks sharing an operand (the n-tiles of one A row-panel, the row blocks of one task's
// weights) hit the same L2 (bijective for any grid size).
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, slot = bid >> 3;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + slot;
}

// the library's activation (named apply_act, not act: the kernels' own `int act` parameters would hide that name)
__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == ORBIT_ACT_RELU) return fmaxf(v, 0.f);
    if (act == ORBIT_ACT_SILU) return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));  // v_exp_f32 + v_rcp_f32, ~1 ulp each
    return v;
}

}  // namespace orbit
