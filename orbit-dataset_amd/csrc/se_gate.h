// Squeeze-excite gate of one frame from the pooling partials (shared by se_gate2_kernel in ops.hip and the gated
// projection kernel in pw_stream.hip, which must produce the same bits).
#pragma once
#include "common.h"
#include "device_util.h"

namespace orbit {

using v4f = __attribute__((ext_vector_type(4))) float;

// squeeze-excite gate from pooling partials: pooled[c] = (sum_chunks partial[b][chunk][c]) / HW, then
// g = sigmoid(W2 silu(W1 pooled + b1) + b2). w2t is W2 transposed to [R][C] so the second layer reads coalesced.
// One block per frame; the block pulls both weight matrices (up to 2 x 221 KB at C = 1152) through one CU's L1, so the
// kernel is a chain of L2 latencies: everything is float4 and every phase keeps 16-20 independent loads per lane in
// flight (layer 1: one wave per hidden unit, four units at a time; layer 2: eight hidden units per step).
// NT threads cooperate; U = hidden units a wave works on at a time. `partial`, `gate`, `pooled_out` point at THIS frame's
// rows; sm2 needs ((C + R + 3) & ~3) + 4 * NT floats.
template <int NT, int U>
__device__ __forceinline__ void se_gate_frame(const float* __restrict__ partial, int chunks, float inv_hw,
                                              const float* __restrict__ w1, const float* __restrict__ b1,
                                              const float* __restrict__ w2t, const float* __restrict__ b2,
                                              float* __restrict__ gate, int C, int R, float* __restrict__ pooled_out, float* sm2) {
    v4f* sp4 = reinterpret_cast<v4f*>(sm2);
    float* hid = sm2 + C;
    const int tid = threadIdx.x;
    const int C4 = C >> 2;
    const v4f* part4 = reinterpret_cast<const v4f*>(partial);  // this frame's [chunks][C]
    const int parts = C4 <= NT / 2 ? NT / C4 : 1;  // thread groups sharing the chunk list of a channel quad
    if (parts > 1 && chunks > 8) {
        // many partials (the fused MBConv front writes one per 8x8 / 4x8 tile: up to 98) and few channels: 256 / C4 threads
        // per quad take every parts-th chunk, the groups' sums are added in group order (fixed order, deterministic)
        v4f* tmp = reinterpret_cast<v4f*>(sm2 + ((C + R + 3) & ~3));  // [parts][C4]
        const int q = tid % C4, part = tid / C4;
        if (part < parts) {
            v4f s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int k = part; k < chunks; k += parts) s += part4[(size_t)k * C4 + q];
            tmp[part * C4 + q] = s;
        }
        __syncthreads();
        if (tid < C4) {
            v4f s = tmp[tid];
            for (int g = 1; g < parts; ++g) s += tmp[g * C4 + tid];
            sp4[tid] = s * inv_hw;
        }
    } else {
        for (int c4 = tid; c4 < C4; c4 += NT) {
            v4f s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int k = 0; k < chunks; ++k) s += part4[(size_t)k * C4 + c4];  // loads batched, adds in chunk order
            sp4[c4] = s * inv_hw;
        }
    }
    __syncthreads();
    if (pooled_out != nullptr)  // training: the pooled means go on the tape (input of the gate MLP's backward)
        for (int c4 = tid; c4 < C4; c4 += NT) reinterpret_cast<v4f*>(pooled_out)[c4] = sp4[c4];
    // layer 1: wave w takes hidden units w, w + 4, ...; four units at a time, lanes stride the channel quads
    const int lane = tid & 63, wave = tid >> 6;
    const v4f* w14 = reinterpret_cast<const v4f*>(w1);
    for (int r0 = wave; r0 < R; r0 += U * (NT / 64)) {  // each wave takes units r0, r0 + NW, .. (U at a time)
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = 0.f;
        for (int cb = 0; cb < C4; cb += 320) {  // 5 quads per lane per pass: C <= 1280 is a single pass
            v4f wv[U][5], pv[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int c4 = cb + lane + 64 * j;
                const bool ok = c4 < C4;
                pv[j] = ok ? sp4[c4] : (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int r = r0 + (NT / 64) * u;
                    wv[u][j] = (ok && r < R) ? w14[(size_t)r * C4 + c4] : (v4f){0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const v4f t = wv[u][j] * pv[j];
                    acc[u] += (t[0] + t[1]) + (t[2] + t[3]);
                }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = r0 + (NT / 64) * u;
            const float sum = wave_sum_dpp(acc[u]);
            if (r < R && lane == 0) {
                const float t = sum + b1[r];
                hid[r] = t / (1.0f + expf(-t));
            }
        }
    }
    __syncthreads();
    // layer 2: thread = channel quad, eight hidden units (eight independent 16-byte loads) per step
    const v4f* w24 = reinterpret_cast<const v4f*>(w2t);
    for (int c4 = tid; c4 < C4; c4 += NT) {
        v4f a = *reinterpret_cast<const v4f*>(b2 + 4 * c4);
        int r = 0;
        for (; r + 8 <= R; r += 8) {
            v4f wv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wv[u] = w24[(size_t)(r + u) * C4 + c4];
#pragma unroll
            for (int u = 0; u < 8; ++u) a += wv[u] * hid[r + u];
        }
        for (; r < R; ++r) a += w24[(size_t)r * C4 + c4] * hid[r];
        v4f g;
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = 1.0f / (1.0f + expf(-a[q]));
        reinterpret_cast<v4f*>(gate)[c4] = g;
    }
}

}  // namespace orbit
