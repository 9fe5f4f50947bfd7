// Training-side elementwise / reduction kernels of the LITE meta-training step:
//   train-mode BatchNorm forward (batch statistics, running-stat update) and BatchNorm backward (train + eval form),
//   max-pool with recorded argmax + its backward, average-pool backward, zero-insertion upsampling (input of the
//   strided-convolution data gradient), prototype-head backward.
// Reference call sites: model/few_shot_recognisers.py:176-183 (_set_batch_norm_state: the extractor runs BatchNorm in
// train() mode while meta-training an unfrozen extractor), :328-437 (LITE forward), single-step-learner.py:212-243
// (loss.backward() through predict_a_batch -> extractor), model/classifier_heads.py:202-230 (head forward whose
// gradient w.r.t. the query features is orbit_proto_predict_backward).
// All tensors are NHWC fp32 viewed as [M][C] matrices (M = B*H*W); every kernel is HBM-bound: one pass, float4 per
// thread, fixed reduction order (no atomics) so that gradients are run-to-run deterministic.
#include "common.h"
#include "device_util.h"

namespace orbit {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// column layout shared by the per-channel reductions: G threads cover G float4 channel-quads, R = 256 / G row lanes
struct ColLayout {
    int Q, G, R, ygroups;
};
static ColLayout col_layout(int C) {
    ColLayout L;
    L.Q = C / 4;
    L.G = L.Q < 256 ? L.Q : 256;
    L.R = 256 / L.G;
    L.ygroups = cdiv(L.Q, L.G);
    return L;
}

int bn_reduce_blocks(int M, int C) {
    const ColLayout L = col_layout(C);
    // enough blocks to fill the chip, at least 4 rows per row lane
    int rows_per_block = cdiv(M, 1024);
    if (rows_per_block < 4 * L.R) rows_per_block = 4 * L.R;
    return cdiv(M, rows_per_block);
}
static int bn_rows_per_block(int M, int C) { return cdiv(M, bn_reduce_blocks(M, C)); }

// partial[blk][0][c] = sum_m y, partial[blk][1][c] = sum_m y^2 over the block's rows
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ y, int M, int C,
                                                               int rows_per_block, int G, int R,
                                                               float* __restrict__ partial) {
    __shared__ f32x4 red[2][256];
    const int tid = threadIdx.x;
    const int rl = tid / G, qi = tid - rl * G, q = blockIdx.y * G + qi;
    const bool active = rl < R && q < (C >> 2);
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, ss = {0.f, 0.f, 0.f, 0.f};
    if (active) {
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += R) {  // 4 rows' loads in flight (rolled: one HBM round trip per row and thread)
            const f32x4 v = *reinterpret_cast<const f32x4*>(y + (size_t)r * C + q * 4);
            s += v;
            ss += v * v;
        }
    }
    red[0][tid] = s, red[1][tid] = ss;
    __syncthreads();
    if (rl == 0 && q < (C >> 2)) {
        for (int j = 1; j < R; ++j) s += red[0][j * G + qi], ss += red[1][j * G + qi];
        *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 0) * C + q * 4) = s;
        *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 1) * C + q * 4) = ss;
    }
}

// Sum of the [nblk][2][C] partials for BN_FIN_CH channels per block: BN_FIN_LANES lanes per channel take every
// BN_FIN_LANES-th partial (double accumulation, fixed order), then an LDS reduction in lane order. (A one-thread-per-channel
// loop over ~1000 partials is a 200 us latency chain; 16 lanes per channel were ~8 us, of which the launch is ~3: these
// kernels run 200 times per LITE step, so the chain is cut to nblk / 64 dependent round trips with 8 loads in flight.)
constexpr int BN_FIN_CH = 4, BN_FIN_LANES = 64;
__device__ __forceinline__ bool reduce_partials(const float* __restrict__ partial, int nblk, int C, double& s0,
                                                double& s1, int& c_out) {
    __shared__ double sh[2][BN_FIN_LANES][BN_FIN_CH];
    const int cl = threadIdx.x % BN_FIN_CH, ln = threadIdx.x / BN_FIN_CH;
    const int c = blockIdx.x * BN_FIN_CH + cl;
    double a0 = 0.0, a1 = 0.0;
    if (c < C) {
#pragma unroll 4
        for (int b = ln; b < nblk; b += BN_FIN_LANES) {
            a0 += (double)partial[((size_t)b * 2 + 0) * C + c];
            a1 += (double)partial[((size_t)b * 2 + 1) * C + c];
        }
    }
    sh[0][ln][cl] = a0, sh[1][ln][cl] = a1;
    __syncthreads();
    if (ln != 0 || c >= C) return false;
    for (int j = 1; j < BN_FIN_LANES; ++j) a0 += sh[0][j][cl], a1 += sh[1][j][cl];
    s0 = a0, s1 = a1, c_out = c;
    return true;
}

// one channel's batch mean / biased variance -> invstd, folded scale / shift, running statistics (shared by the finalize
// kernels: from [nblk][2][C] partial sums, and from the Gram matrix of a pointwise conv's input)
__device__ __forceinline__ void bn_finalize_channel(int c, double mean, double var, int M, float eps, float momentum,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    const float* __restrict__ conv_bias, float* __restrict__ mean_out,
                                                    float* __restrict__ invstd_out, float* __restrict__ scale,
                                                    float* __restrict__ shift, float* __restrict__ running_mean,
                                                    float* __restrict__ running_var) {
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    mean_out[c] = (float)mean;
    invstd_out[c] = invstd;
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    if (scale) {
        const float sc = g * invstd;
        scale[c] = sc;
        shift[c] = b - (float)mean * sc;
    }
    if (running_mean) {
        // y holds the convolution WITHOUT its bias; the module's input to BatchNorm includes it
        const float cb = conv_bias ? conv_bias[c] : 0.f;
        const double unbiased = M > 1 ? var * (double)M / (double)(M - 1) : var;
        if (momentum >= 1.f) {
            // momentum 1 (also the deferred form of the training forwards: the slot on the tape is uninitialised memory and
            // 0 * NaN would poison it): the statistics replace the old value, which is never read
            running_mean[c] = (float)mean + cb;
            running_var[c] = (float)unbiased;
        } else {
            running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * ((float)mean + cb);
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
        }
    }
}

// mean / biased variance -> invstd, folded scale/shift, running statistics (momentum update with the unbiased
// variance, torch.nn.BatchNorm2d semantics). gamma/beta point at the layer's own or the per-task FiLM vectors.
__global__ __launch_bounds__(256) void bn_stats_finalize_kernel(const float* __restrict__ partial, int nblk, int M,
                                                                int C, float eps, float momentum,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta,
                                                                const float* __restrict__ conv_bias,
                                                                float* __restrict__ mean_out,
                                                                float* __restrict__ invstd_out,
                                                                float* __restrict__ scale, float* __restrict__ shift,
                                                                float* __restrict__ running_mean,
                                                                float* __restrict__ running_var) {
    double s, ss;
    int c;
    if (!reduce_partials(partial, nblk, C, s, ss, c)) return;
    const double mean = s / M;
    bn_finalize_channel(c, mean, ss / M - mean * mean, M, eps, momentum, gamma, beta, conv_bias, mean_out, invstd_out, scale,
                        shift, running_mean, running_var);
}

// ---- BatchNorm statistics of a POINTWISE conv's output from the second moments of its input (round 6) -----------------
// y = W x (1x1 conv, no bias) is linear, so over the P pixels of a batch  mean(y_c) = w_c . mean(x)  and
// E[y_c^2] = w_c^T E[x x^T] w_c: the batch statistics of the first BatchNorm of an MBConv block (6x expanded: 96 .. 240
// channels) follow from the Cin x Cin Gram matrix of the block's input (16 .. 40 channels) - a pass over a tensor six times
// smaller than the one the statistics describe, and no matrix-core work. It replaces the statistics sweep of the expansion
// conv in front of the two-sweep fused front (csrc/extractor_train.hip train_forms: 229 -> ~35 us for 16 -> 96 at
// 112x112). Sums: fp32 per thread over <= ~64 pixels, fp32 over a block's 256 threads in a fixed order, double over the
// blocks and through the quadratic form; the variance is E[y^2] - mean^2 in double, as in bn_stats_finalize_kernel.
// partial[blk][CIN * CIN + CIN]: G row-major, then the column sums. Grid (nblk, CIN / RS): a block owns RS rows of G.

template <int CIN, int RS>
__global__ __launch_bounds__(256) void gram_partial_kernel(const float* __restrict__ x, int P, int pixels_per_block,
                                                           float* __restrict__ partial) {
    constexpr int Q = CIN / 4;
    __shared__ float red[4][RS * CIN + RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.y * RS;
    const int p0 = blockIdx.x * pixels_per_block, p1 = min(P, p0 + pixels_per_block);
    float acc[RS][CIN], rs[RS];
#pragma unroll
    for (int i = 0; i < RS; ++i) {
        rs[i] = 0.f;
#pragma unroll
        for (int j = 0; j < CIN; ++j) acc[i][j] = 0.f;
    }
    // four pixels' loads in flight per thread (a pixel at a time, every pixel paid an HBM round trip of its own: the first form
    // of this kernel took 115 us for the 160 MB of block 1.0's input)
    constexpr int U = 4;
    for (int pb = p0 + tid; pb < p1; pb += 256 * U) {
        f32x4 v[U][Q];
        float xr[U][RS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = min(pb + 256 * u, p1 - 1);  // (a clamped pixel is loaded and not accumulated)
#pragma unroll
            for (int q = 0; q < Q; ++q) v[u][q] = *reinterpret_cast<const f32x4*>(x + (size_t)p * CIN + 4 * q);
            // the block's own RS row values come through loads of their own (same cache lines as v: L1 hits) - indexing the
            // register array v with the block-uniform r0 would send it through scratch memory
#pragma unroll
            for (int i = 0; i < RS; ++i) xr[u][i] = x[(size_t)p * CIN + r0 + i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (pb + 256 * u < p1) {
#pragma unroll
                for (int i = 0; i < RS; ++i) {
                    const float xi = xr[u][i];
                    rs[i] += xi;
#pragma unroll
                    for (int j = 0; j < CIN; ++j) acc[i][j] += xi * v[u][j >> 2][j & 3];
                }
            }
        }
    }
    // block sum in a fixed order: DPP reduction over the wave's lanes, then the four waves in wave order
#pragma unroll
    for (int i = 0; i < RS; ++i) {
#pragma unroll
        for (int j = 0; j < CIN; ++j) {
            const float t = wave_sum_dpp(acc[i][j]);
            if (lane == 0) red[wave][i * CIN + j] = t;
        }
        const float t = wave_sum_dpp(rs[i]);
        if (lane == 0) red[wave][RS * CIN + i] = t;
    }
    __syncthreads();
    float* out = partial + (size_t)blockIdx.x * (CIN * CIN + CIN);
    for (int e = tid; e < RS * CIN + RS; e += 256) {
        const float t = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
        if (e < RS * CIN) out[(r0 + e / CIN) * CIN + e % CIN] = t;
        else out[CIN * CIN + r0 + (e - RS * CIN)] = t;
    }
}

// one block (1024 threads) per 64 output channels: the partials are summed in double - every entry by four lanes that take
// every fourth block, combined in lane order (every block of this kernel re-sums them: <= 1640 entries x nblk L2-resident
// floats) - then thread c evaluates its channel's mean and quadratic form and finishes like bn_stats_finalize_kernel
template <int CIN>
__global__ __launch_bounds__(1024) void gram_bn_finalize_kernel(const float* __restrict__ partial, int nblk, int P,
                                                                const float* __restrict__ w /* [C][CIN] */, int C, float eps,
                                                                float momentum, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ mean_out,
                                                                float* __restrict__ invstd_out, float* __restrict__ scale,
                                                                float* __restrict__ shift, float* __restrict__ running_mean,
                                                                float* __restrict__ running_var) {
    constexpr int NE = CIN * CIN + CIN;
    __shared__ double G[4][NE];
    for (int idx = threadIdx.x; idx < 4 * NE; idx += 1024) {
        const int part = idx / NE, e = idx - part * NE;
        double a = 0.0;
#pragma unroll 8
        for (int b = part; b < nblk; b += 4) a += (double)partial[(size_t)b * NE + e];
        G[part][e] = a;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NE; e += 1024) G[0][e] = (G[0][e] + G[1][e]) + (G[2][e] + G[3][e]);
    __syncthreads();
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (threadIdx.x >= 64 || c >= C) return;
    float wc[CIN];
#pragma unroll
    for (int q = 0; q < CIN / 4; ++q) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(w + (size_t)c * CIN + 4 * q);
        wc[4 * q] = t[0], wc[4 * q + 1] = t[1], wc[4 * q + 2] = t[2], wc[4 * q + 3] = t[3];
    }
    double m = 0.0, q2 = 0.0;
#pragma unroll
    for (int i = 0; i < CIN; ++i) {
        m += (double)wc[i] * G[0][CIN * CIN + i];
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < CIN; ++j) row += G[0][i * CIN + j] * (double)wc[j];
        q2 += (double)wc[i] * row;
    }
    const double mean = m / P;
    bn_finalize_channel(c, mean, q2 / P - mean * mean, P, eps, momentum, gamma, beta, nullptr, mean_out, invstd_out, scale,
                        shift, running_mean, running_var);
}

// a = act(y * scale + shift + residual); RPOST (compile-time form, the post-activation skip of timm's ConvBnAct):
// a = act(y * scale + shift) + residual, residual required
template <bool RPOST = false>
__global__ __launch_bounds__(256) void scale_shift_act_kernel(const float* __restrict__ y,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift,
                                                              const float* __restrict__ residual, int act,
                                                              size_t total4, int C4, float* __restrict__ out) {
    // channel quad of element i = i mod C4, walked incrementally: a 64-bit modulo per 16-byte element is ~100 instructions
    // and made these streaming kernels instruction-bound
    const unsigned stride = gridDim.x * 256u, stride_mod = stride % (unsigned)C4;
    unsigned q = (blockIdx.x * 256u + threadIdx.x) % (unsigned)C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4;
         i += stride, q = q + stride_mod >= (unsigned)C4 ? q + stride_mod - C4 : q + stride_mod) {
        f32x4 v = reinterpret_cast<const f32x4*>(y)[i];
        if (scale) v = v * reinterpret_cast<const f32x4*>(scale)[q] + reinterpret_cast<const f32x4*>(shift)[q];
        if (!RPOST && residual) v += reinterpret_cast<const f32x4*>(residual)[i];
        if (act == ORBIT_ACT_RELU) {
            v[0] = fmaxf(v[0], 0.f), v[1] = fmaxf(v[1], 0.f), v[2] = fmaxf(v[2], 0.f), v[3] = fmaxf(v[3], 0.f);
        } else if (act == ORBIT_ACT_SILU) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = v[k] * __builtin_amdgcn_rcpf(1.0f + __expf(-v[k]));
        }
        if (RPOST) v += reinterpret_cast<const f32x4*>(residual)[i];
        reinterpret_cast<f32x4*>(out)[i] = v;
    }
}

// Partials that come from a producing kernel's epilogue (conv_igemm: one per 32-128 output rows; the depthwise kernels: one
// per frame and row chunk) can number tens of thousands; the finalize kernel walks them with 16 lanes per channel. Above
// BN_COMPACT_ABOVE blocks a first pass adds groups of GS consecutive blocks (fixed order): out[g][2][C], float4 columns.
constexpr int BN_COMPACT_ABOVE = 2048, BN_COMPACT_TO = 1024;
__global__ __launch_bounds__(256) void bn_partial_compact_kernel(const float* __restrict__ partial, int nblk, int cols4,
                                                                 int GS, int nout, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nout * cols4) return;
    const int g = (int)(i / cols4), q = (int)(i - (size_t)g * cols4);
    const int b0 = g * GS, b1 = min(nblk, b0 + GS);
    const f32x4* src = reinterpret_cast<const f32x4*>(partial) + (size_t)b0 * cols4 + q;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int b = b0; b < b1; ++b, src += cols4) acc += *src;
    reinterpret_cast<f32x4*>(out)[i] = acc;
}

// a = act(y * scale + shift) with the squeeze-excite pooling partials of a from the same pass (the train-mode depthwise
// BatchNorm of an MBConv block: timm SqueezeExcite starts with x.mean((2, 3)) of exactly this tensor). Block = (row chunk,
// column group, frame); thread = one channel quad x one row lane, walking its rows 4 at a time; pool[b][chunk][C] holds the
// chunk's column sums (fixed order: row lanes combined through LDS), which se_gate2 adds up and scales by 1 / HW.
__global__ __launch_bounds__(256) void scale_shift_act_pool_kernel(const float* __restrict__ y,
                                                                   const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, int act, int HW, int C,
                                                                   int rows_per_chunk, int G, int R,
                                                                   float* __restrict__ out, float* __restrict__ pool) {
    __shared__ f32x4 red[256];
    const int tid = threadIdx.x;
    const int rl = tid / G, qi = tid - rl * G, q = blockIdx.y * G + qi;
    const bool active = rl < R && q < (C >> 2);
    const int chunk = blockIdx.x, b = blockIdx.z;
    const int r0 = chunk * rows_per_chunk, r1 = min(HW, r0 + rows_per_chunk);
    f32x4 psum = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + q * 4), sh = *reinterpret_cast<const f32x4*>(shift + q * 4);
        const size_t base = (size_t)b * HW * C + q * 4;
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += R) {
            f32x4 v = *reinterpret_cast<const f32x4*>(y + base + (size_t)r * C) * sc + sh;
            if (act == ORBIT_ACT_RELU) {
                v[0] = fmaxf(v[0], 0.f), v[1] = fmaxf(v[1], 0.f), v[2] = fmaxf(v[2], 0.f), v[3] = fmaxf(v[3], 0.f);
            } else if (act == ORBIT_ACT_SILU) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = v[k] * __builtin_amdgcn_rcpf(1.0f + __expf(-v[k]));
            }
            *reinterpret_cast<f32x4*>(out + base + (size_t)r * C) = v;
            psum += v;
        }
    }
    red[tid] = psum;
    __syncthreads();
    if (rl == 0 && q < (C >> 2)) {
        for (int j = 1; j < R; ++j) psum += red[j * G + qi];
        *reinterpret_cast<f32x4*>(pool + ((size_t)b * gridDim.x + chunk) * C + q * 4) = psum;
    }
}

// d silu(z) / dz = s (1 + z (1 - s)), s = sigmoid(z); same fast exp/rcp as the forward activation
__device__ __forceinline__ f32x4 silu_grad(f32x4 g, f32x4 z) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-z[k]));
        g[k] *= sg * (1.0f + z[k] * (1.0f - sg));
    }
    return g;
}

__device__ __forceinline__ f32x4 relu_mask(f32x4 g, f32x4 a) {
    g[0] = a[0] > 0.f ? g[0] : 0.f, g[1] = a[1] > 0.f ? g[1] : 0.f;
    g[2] = a[2] > 0.f ? g[2] : 0.f, g[3] = a[3] > 0.f ? g[3] : 0.f;
    return g;
}

// partial[blk][0][c] = sum_m g, partial[blk][1][c] = sum_m g * xhat, with g = dout * act'(.) and
// xhat = (y - mean) * invstd. RPOST (compile-time form): out = act(z) + residual, z = y * scale + shift - g is the same
// expression, but `out` no longer tells ReLU's mask: it is taken from z (scale / shift required for every activation)
template <bool RPOST = false>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ dout,
                                                             const float* __restrict__ out,
                                                             const float* __restrict__ y,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift, int act, int M, int C,
                                                             int rows_per_block, int G, int R,
                                                             float* __restrict__ partial) {
    __shared__ f32x4 red[2][256];
    const int tid = threadIdx.x;
    const int rl = tid / G, qi = tid - rl * G, q = blockIdx.y * G + qi;
    const bool active = rl < R && q < (C >> 2);
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(M, r0 + rows_per_block);
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, sx = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + q * 4);
        const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + q * 4);
        f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (act == ORBIT_ACT_SILU || (RPOST && act == ORBIT_ACT_RELU)) {
            sc = *reinterpret_cast<const f32x4*>(scale + q * 4), sh = *reinterpret_cast<const f32x4*>(shift + q * 4);
        }
#pragma unroll 2
        for (int r = r0 + rl; r < r1; r += R) {  // two rows' loads in flight
            const size_t o = (size_t)r * C + q * 4;
            f32x4 g = *reinterpret_cast<const f32x4*>(dout + o);
            const f32x4 yv = *reinterpret_cast<const f32x4*>(y + o);
            if (RPOST && act == ORBIT_ACT_RELU) g = relu_mask(g, yv * sc + sh);
            else if (act == ORBIT_ACT_RELU) g = relu_mask(g, *reinterpret_cast<const f32x4*>(out + o));
            else if (act == ORBIT_ACT_SILU) g = silu_grad(g, yv * sc + sh);
            const f32x4 xh = (yv - mu) * is;
            s += g;
            sx += g * xh;
        }
    }
    red[0][tid] = s, red[1][tid] = sx;
    __syncthreads();
    if (rl == 0 && q < (C >> 2)) {
        for (int j = 1; j < R; ++j) s += red[0][j * G + qi], sx += red[1][j * G + qi];
        *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 0) * C + q * 4) = s;
        *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 1) * C + q * 4) = sx;
    }
}

// dbeta = sum g, dgamma = sum g*xhat; coefficients of the apply pass: dy = k1 * (g - k2 - xhat * k3)
//   train: k1 = gamma*invstd, k2 = dbeta/M, k3 = dgamma/M         eval: k2 = k3 = 0
// dbias (bias of the convolution in front of an eval-mode BatchNorm) = sum dy = k1 * dbeta
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nblk, int M,
                                                              int C, int train, const float* __restrict__ gamma,
                                                              const float* __restrict__ invstd,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ dbias, float* __restrict__ coef) {
    double s, sx;
    int c;
    if (!reduce_partials(partial, nblk, C, s, sx, c)) return;
    if (dgamma) dgamma[c] = (float)sx;
    if (dbeta) dbeta[c] = (float)s;
    const float k1 = (gamma ? gamma[c] : 1.f) * invstd[c];
    coef[c] = k1;
    coef[C + c] = train ? (float)(s / M) : 0.f;
    coef[2 * C + c] = train ? (float)(sx / M) : 0.f;
    if (dbias) dbias[c] = train ? 0.f : k1 * (float)s;
}

// RPOST (compile-time form): out = act(z) + residual - the residual branch receives dout itself, not g
template <bool RPOST = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dout,
                                                           const float* __restrict__ out,
                                                           const float* __restrict__ y,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ coef, int act, size_t total4,
                                                           int C4, float* __restrict__ dy, float* __restrict__ dres,
                                                           int dres_accumulate) {
    const int C = C4 * 4;
    const unsigned stride = gridDim.x * 256u, stride_mod = stride % (unsigned)C4;  // see scale_shift_act_kernel
    unsigned q = (blockIdx.x * 256u + threadIdx.x) % (unsigned)C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4;
         i += stride, q = q + stride_mod >= (unsigned)C4 ? q + stride_mod - C4 : q + stride_mod) {
        f32x4 g = reinterpret_cast<const f32x4*>(dout)[i];
        const f32x4 yv = reinterpret_cast<const f32x4*>(y)[i];
        if (RPOST && dres) {
            f32x4 d = g;
            if (dres_accumulate) d += reinterpret_cast<const f32x4*>(dres)[i];
            reinterpret_cast<f32x4*>(dres)[i] = d;
        }
        if (RPOST && act == ORBIT_ACT_RELU)
            g = relu_mask(g, yv * reinterpret_cast<const f32x4*>(scale)[q] + reinterpret_cast<const f32x4*>(shift)[q]);
        else if (act == ORBIT_ACT_RELU) g = relu_mask(g, reinterpret_cast<const f32x4*>(out)[i]);
        else if (act == ORBIT_ACT_SILU)
            g = silu_grad(g, yv * reinterpret_cast<const f32x4*>(scale)[q] + reinterpret_cast<const f32x4*>(shift)[q]);
        const f32x4 xh = (yv - reinterpret_cast<const f32x4*>(mean)[q]) * reinterpret_cast<const f32x4*>(invstd)[q];
        const f32x4 k1 = reinterpret_cast<const f32x4*>(coef)[q];
        const f32x4 k2 = reinterpret_cast<const f32x4*>(coef + C)[q];
        const f32x4 k3 = reinterpret_cast<const f32x4*>(coef + 2 * C)[q];
        reinterpret_cast<f32x4*>(dy)[i] = k1 * (g - k2 - xh * k3);
        if (!RPOST && dres) {
            if (dres_accumulate) g += reinterpret_cast<const f32x4*>(dres)[i];
            reinterpret_cast<f32x4*>(dres)[i] = g;
        }
    }
}

// ---- max-pool with recorded argmax (first maximum in (kh, kw) scan order, the rule of torch's CPU/GPU kernels) ----
__global__ __launch_bounds__(256) void maxpool_idx_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          uint8_t* __restrict__ idx, int B, int H, int W, int C4,
                                                          int K, int stride, int pad, int Ho, int Wo) {
    const size_t total = (size_t)B * Ho * Wo * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        // 32-bit index arithmetic (the launcher checks total < 2^32): 64-bit div / mod are ~100 instructions each
        const unsigned iu = (unsigned)i, r1 = iu / (unsigned)C4, r2 = r1 / (unsigned)Wo, bu = r2 / (unsigned)Ho;
        const int q = (int)(iu - r1 * C4), wo = (int)(r1 - r2 * Wo), ho = (int)(r2 - bu * Ho), b = (int)bu;
        f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bi[4] = {-1, -1, -1, -1};
        for (int kh = 0; kh < K; ++kh) {
            const int hi = ho * stride - pad + kh;
            if ((unsigned)hi >= (unsigned)H) continue;
            for (int kw = 0; kw < K; ++kw) {
                const int wi = wo * stride - pad + kw;
                if ((unsigned)wi >= (unsigned)W) continue;
                const f32x4 v = reinterpret_cast<const f32x4*>(x)[(((size_t)b * H + hi) * W + wi) * C4 + q];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (bi[k] < 0 || v[k] > best[k]) best[k] = v[k], bi[k] = kh * K + kw;
            }
        }
        reinterpret_cast<f32x4*>(y)[i] = best;
        reinterpret_cast<uchar4*>(idx)[i] = make_uchar4((uint8_t)bi[0], (uint8_t)bi[1], (uint8_t)bi[2], (uint8_t)bi[3]);
    }
}

// gather form: every input element sums the gradients of the windows whose recorded argmax is that element
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy,
                                                          const uint8_t* __restrict__ idx, float* __restrict__ dx,
                                                          int B, int H, int W, int C4, int K, int stride, int pad,
                                                          int Ho, int Wo) {
    const size_t total = (size_t)B * H * W * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        // 32-bit index arithmetic (the launcher checks total < 2^32): 64-bit div / mod are ~100 instructions each
        const unsigned iu = (unsigned)i, r1 = iu / (unsigned)C4, r2 = r1 / (unsigned)W, bu = r2 / (unsigned)H;
        const int q = (int)(iu - r1 * C4), w = (int)(r1 - r2 * W), h = (int)(r2 - bu * H), b = (int)bu;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        for (int kh = 0; kh < K; ++kh) {
            const int t = h + pad - kh;
            if (t < 0 || t % stride) continue;
            const int ho = t / stride;
            if (ho >= Ho) continue;
            for (int kw = 0; kw < K; ++kw) {
                const int u = w + pad - kw;
                if (u < 0 || u % stride) continue;
                const int wo = u / stride;
                if (wo >= Wo) continue;
                const size_t o = (((size_t)b * Ho + ho) * Wo + wo) * C4 + q;
                const uchar4 id = reinterpret_cast<const uchar4*>(idx)[o];
                const f32x4 d = reinterpret_cast<const f32x4*>(dy)[o];
                const int me = kh * K + kw;
                if (id.x == me) g[0] += d[0];
                if (id.y == me) g[1] += d[1];
                if (id.z == me) g[2] += d[2];
                if (id.w == me) g[3] += d[3];
            }
        }
        reinterpret_cast<f32x4*>(dx)[i] = g;
    }
}

__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B,
                                                          int HW, int C4) {
    const size_t total = (size_t)B * HW * C4;
    const float inv = 1.0f / (float)HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const unsigned iu = (unsigned)i;  // 32-bit index arithmetic (launcher: total < 2^32)
        const int q = (int)(iu % (unsigned)C4);
        const int b = (int)(iu / ((unsigned)HW * (unsigned)C4));
        reinterpret_cast<f32x4*>(dx)[i] = reinterpret_cast<const f32x4*>(dy)[(size_t)b * C4 + q] * inv;
    }
}

// dst[b][h][w][:] = src[b][h/s][w/s][:] where h, w are multiples of s inside the source grid, else 0
__global__ __launch_bounds__(256) void upsample_zero_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            int B, int H, int W, int C4, int s, int Hs, int Ws) {
    const size_t total = (size_t)B * H * W * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        // 32-bit index arithmetic (the launcher checks total < 2^32): 64-bit div / mod are ~100 instructions each
        const unsigned iu = (unsigned)i, r1 = iu / (unsigned)C4, r2 = r1 / (unsigned)W, bu = r2 / (unsigned)H;
        const int q = (int)(iu - r1 * C4), w = (int)(r1 - r2 * W), h = (int)(r2 - bu * H), b = (int)bu;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (h % s == 0 && w % s == 0 && h / s < Hs && w / s < Ws)
            v = reinterpret_cast<const f32x4*>(src)[(((size_t)b * Hs + h / s) * Ws + w / s) * C4 + q];
        reinterpret_cast<f32x4*>(dst)[i] = v;
    }
}

static int grid_for(size_t total) {
    size_t b = (total + 255) / 256;
    return (int)(b > 8192 ? 8192 : (b ? b : 1));
}

// ---- launchers (declared in common.h) -----------------------------------------------------------------------------
// finalize from [nblk][2][C] partials, whoever produced them (bn_stats_partial_kernel, a conv epilogue, a depthwise kernel).
// `partial` must have room for the compaction stage behind the nblk blocks: bn_partial_floats(nblk, C) floats in all.
size_t bn_partial_floats(size_t nblk, int C) {
    return (nblk + (nblk > (size_t)BN_COMPACT_ABOVE ? (size_t)BN_COMPACT_TO : 0)) * 2 * (size_t)C;
}
int launch_bn_stats_from_partials(float* partial, int nblk, int M, int C, const BnAffine& a, const BnFold& out, hipStream_t s) {
    ORBIT_REQUIRE(C % 4 == 0 && M > 0 && nblk > 0 && partial, "bn_stats: bad arguments");
    const float* src = partial;
    if (nblk > BN_COMPACT_ABOVE) {
        const int GS = cdiv(nblk, BN_COMPACT_TO), nout = cdiv(nblk, GS), cols4 = 2 * C / 4;
        float* out = partial + (size_t)nblk * 2 * C;
        const size_t items = (size_t)nout * cols4;
        const int rec = prof_start("bn_partial_compact", 2.0 * nblk * C, 4.0 * (nblk + nout) * 2.0 * C, s);
        bn_partial_compact_kernel<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(partial, nblk, cols4, GS, nout, out);
        prof_stop(rec, s);
        ORBIT_LAUNCH_CHECK();
        src = out, nblk = nout;
    }
    bn_stats_finalize_kernel<<<cdiv(C, BN_FIN_CH), 256, 0, s>>>(src, nblk, M, C, a.eps, a.momentum, a.gamma, a.beta, a.conv_bias,
                                                                out.mean, out.invstd, out.scale, out.shift, a.running_mean,
                                                                a.running_var);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// batch statistics of y = W x (pointwise conv, W = [C][Cin] as torch stores it) from the Gram matrix of x [P][Cin]
bool bn_gram_supported(int Cin) { return Cin == 16 || Cin == BN_GRAM_MAX_CIN; }  // (the 112x112 / 56x56 blocks; wider inputs take the conv's statistics sweep)
static int gram_blocks(int P) {  // ~one block per CU and row slice: a thread walks ~40 pixels, four at a time
    const int b = cdiv(P, 256 * 32);
    return b > 256 ? 256 : (b ? b : 1);
}
size_t bn_gram_scratch_floats(int P, int Cin) { return (size_t)gram_blocks(P) * ((size_t)Cin * Cin + Cin); }
int launch_bn_stats_from_gram(const float* x, int P, int Cin, const float* w, int C, const BnAffine& a, const BnFold& out,
                              float* scratch, hipStream_t s) {
    ORBIT_REQUIRE(x && w && out.mean && out.invstd && scratch && P > 0 && C > 0 && !a.conv_bias, "bn_stats_from_gram: bad arguments");
    ORBIT_REQUIRE(bn_gram_supported(Cin), "bn_stats_from_gram: Cin = %d not instantiated", Cin);
    const int nblk = gram_blocks(P);
    const int ppb = cdiv(cdiv(P, nblk), 256) * 256;
    const int rec = prof_start("bn_gram", 2.0 * P * Cin * Cin, 4.0 * P * Cin, s);
#define ORBIT_GRAM(CI, RS_)                                                                                                  \
    do {                                                                                                                     \
        gram_partial_kernel<CI, RS_><<<dim3(cdiv(P, ppb), CI / RS_), 256, 0, s>>>(x, P, ppb, scratch);                       \
        gram_bn_finalize_kernel<CI><<<cdiv(C, 64), 1024, 0, s>>>(scratch, cdiv(P, ppb), P, w, C, a.eps, a.momentum, a.gamma,  \
                                                                a.beta, out.mean, out.invstd, out.scale, out.shift,          \
                                                                a.running_mean, a.running_var);                              \
    } while (0)
    if (Cin == 16) ORBIT_GRAM(16, 8);
    else ORBIT_GRAM(24, 6);
#undef ORBIT_GRAM
    prof_stop(rec, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// stats[0][c] = sum_b partial[b][0][c], stats[1][c] = sum_b partial[b][1][c] (double accumulation): the raw sums behind a
// train-mode BatchNorm, for the single-operator test entries
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ partial, int nblk, int C,
                                                           float* __restrict__ stats) {
    double s, ss;
    int c;
    if (!reduce_partials(partial, nblk, C, s, ss, c)) return;
    stats[c] = (float)s, stats[C + c] = (float)ss;
}
int launch_sum_partials(const float* partial, int nblk, int C, float* stats, hipStream_t s) {
    sum_partials_kernel<<<cdiv(C, BN_FIN_CH), 256, 0, s>>>(partial, nblk, C, stats);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_bn_stats(const float* y, int M, int C, const BnAffine& a, const BnFold& out, float* partial, hipStream_t s) {
    ORBIT_REQUIRE(C % 4 == 0 && M > 0, "bn_stats: C %% 4 != 0 or empty batch");
    const ColLayout L = col_layout(C);
    const int nblk = bn_reduce_blocks(M, C);
    bn_stats_partial_kernel<<<dim3(nblk, L.ygroups), 256, 0, s>>>(y, M, C, bn_rows_per_block(M, C), L.G, L.R, partial);
    ORBIT_LAUNCH_CHECK();
    return launch_bn_stats_from_partials(partial, nblk, M, C, a, out, s);
}

// chunks per frame of the pooled apply pass: enough blocks to fill the chip at any batch size, >= 4 rows per row lane
int se_pool_chunks(int B, int HW, int C) {
    const ColLayout L = col_layout(C);
    int want = cdiv(2048, B * L.ygroups);
    const int most = cdiv(HW, 4 * L.R);
    if (want > most) want = most;
    if (want < 1) want = 1;
    return cdiv(HW, cdiv(HW, want));
}
int launch_scale_shift_act_pool(const float* y, const float* scale, const float* shift, int act, int B, int HW, int C,
                                float* out, float* pool, hipStream_t s) {
    ORBIT_REQUIRE(C % 4 == 0 && y && scale && shift && out && pool, "scale_shift_act_pool: bad arguments");
    const ColLayout L = col_layout(C);
    const int chunks = se_pool_chunks(B, HW, C);
    scale_shift_act_pool_kernel<<<dim3(chunks, L.ygroups, B), 256, 0, s>>>(y, scale, shift, act, HW, C, cdiv(HW, chunks), L.G,
                                                                            L.R, out, pool);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_scale_shift_act(const float* y, const float* scale, const float* shift, const float* residual, int act,
                           size_t M, int C, float* out, hipStream_t s, int res_post) {
    ORBIT_REQUIRE(C % 4 == 0, "scale_shift_act: C %% 4 != 0");
    ORBIT_REQUIRE(!res_post || residual, "scale_shift_act: the post-activation skip needs its residual");
    const size_t total4 = M * (size_t)(C / 4);
    if (res_post) scale_shift_act_kernel<true><<<grid_for(total4), 256, 0, s>>>(y, scale, shift, residual, act, total4, C / 4, out);
    else scale_shift_act_kernel<<<grid_for(total4), 256, 0, s>>>(y, scale, shift, residual, act, total4, C / 4, out);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_bn_backward(const float* dout, const float* out, const float* y, const BnFoldC& bn, const BnGrads& p, int train,
                       int act, int M, int C, float* dy, float* dres, int dres_accumulate, float* partial, float* coef,
                       hipStream_t s, int res_post) {
    ORBIT_REQUIRE(C % 4 == 0 && M > 0, "bn_backward: C %% 4 != 0 or empty batch");
    ORBIT_REQUIRE(act != ORBIT_ACT_SILU || (bn.scale && bn.shift), "bn_backward: SiLU needs the folded scale/shift");
    ORBIT_REQUIRE(act != ORBIT_ACT_RELU || out || res_post, "bn_backward: ReLU needs the activation output");
    ORBIT_REQUIRE(!res_post || act == ORBIT_ACT_NONE || (bn.scale && bn.shift),
                  "bn_backward: the post-activation skip needs the folded scale/shift");
    const ColLayout L = col_layout(C);
    const int nblk = bn_reduce_blocks(M, C);
    if (res_post)
        bn_bwd_partial_kernel<true><<<dim3(nblk, L.ygroups), 256, 0, s>>>(dout, out, y, bn.mean, bn.invstd, bn.scale, bn.shift, act,
                                                                          M, C, bn_rows_per_block(M, C), L.G, L.R, partial);
    else
        bn_bwd_partial_kernel<<<dim3(nblk, L.ygroups), 256, 0, s>>>(dout, out, y, bn.mean, bn.invstd, bn.scale, bn.shift, act, M, C,
                                                                    bn_rows_per_block(M, C), L.G, L.R, partial);
    ORBIT_LAUNCH_CHECK();
    bn_bwd_finalize_kernel<<<cdiv(C, BN_FIN_CH), 256, 0, s>>>(partial, nblk, M, C, train, p.gamma, bn.invstd, p.dgamma, p.dbeta,
                                                              p.dbias, coef);
    ORBIT_LAUNCH_CHECK();
    if (dy) {
        const size_t total4 = (size_t)M * (C / 4);
        if (res_post)
            bn_bwd_apply_kernel<true><<<grid_for(total4), 256, 0, s>>>(dout, out, y, bn.mean, bn.invstd, bn.scale, bn.shift, coef,
                                                                       act, total4, C / 4, dy, dres, dres_accumulate);
        else
            bn_bwd_apply_kernel<<<grid_for(total4), 256, 0, s>>>(dout, out, y, bn.mean, bn.invstd, bn.scale, bn.shift, coef, act,
                                                                 total4, C / 4, dy, dres, dres_accumulate);
        ORBIT_LAUNCH_CHECK();
    }
    return ORBIT_OK;
}

int launch_bn_backward_reduced(const float* g, const float* y, const BnFoldC& bn, const BnGrads& p, int train, int M, int C,
                               float* dy, float* partial, int nblk, float* coef, hipStream_t s) {
    ORBIT_REQUIRE(C % 4 == 0 && M > 0 && nblk > 0 && g && y && partial && coef && !p.dbias, "bn_backward_reduced: bad arguments");
    const float* src = partial;
    if (nblk > BN_COMPACT_ABOVE) {
        const int GS = cdiv(nblk, BN_COMPACT_TO), nout = cdiv(nblk, GS), cols4 = 2 * C / 4;
        float* out = partial + (size_t)nblk * 2 * C;
        const size_t items = (size_t)nout * cols4;
        const int rec = prof_start("bn_partial_compact", 2.0 * nblk * C, 4.0 * (nblk + nout) * 2.0 * C, s);
        bn_partial_compact_kernel<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(partial, nblk, cols4, GS, nout, out);
        prof_stop(rec, s);
        ORBIT_LAUNCH_CHECK();
        src = out, nblk = nout;
    }
    bn_bwd_finalize_kernel<<<cdiv(C, BN_FIN_CH), 256, 0, s>>>(src, nblk, M, C, train, p.gamma, bn.invstd, p.dgamma, p.dbeta, nullptr,
                                                              coef);
    ORBIT_LAUNCH_CHECK();
    if (dy) {
        const size_t total4 = (size_t)M * (C / 4);
        bn_bwd_apply_kernel<<<grid_for(total4), 256, 0, s>>>(g, nullptr, y, bn.mean, bn.invstd, nullptr, nullptr, coef,
                                                             ORBIT_ACT_NONE, total4, C / 4, dy, nullptr, 0);
        ORBIT_LAUNCH_CHECK();
    }
    return ORBIT_OK;
}

// dy = k1 * (g - k2 - xhat * k3) with g = (dxg * gate[b] + dpooled[b] / HW) * act'(y * scale + shift) rebuilt on the fly - the
// expression gate_bwd_apply_bn_kernel (csrc/train_mbconv.hip) summed, so the sums in coef belong to exactly this g
__global__ __launch_bounds__(256) void gate_bn_bwd_apply_kernel(const float* __restrict__ dxg, const float* __restrict__ gate,
                                                                const float* __restrict__ dpooled,
                                                                const float* __restrict__ y, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift,
                                                                const float* __restrict__ coef, int act, int HW, int C4,
                                                                size_t total4, float* __restrict__ dy) {
    const int C = C4 * 4;
    const float inv = 1.0f / (float)HW;
    const unsigned per_frame = (unsigned)HW * (unsigned)C4;  // grid = (blocks per frame, frames); total4 = per_frame here
    const unsigned b = blockIdx.y;
    const unsigned stride = gridDim.x * 256u, stride_mod = stride % (unsigned)C4;  // see scale_shift_act_kernel
    unsigned q = (blockIdx.x * 256u + threadIdx.x) % (unsigned)C4;
    const size_t base = (size_t)b * per_frame;
    for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < per_frame;
         j += stride, q = q + stride_mod >= (unsigned)C4 ? q + stride_mod - C4 : q + stride_mod) {
        const size_t i = base + j;
        f32x4 g = reinterpret_cast<const f32x4*>(dxg)[i] * reinterpret_cast<const f32x4*>(gate)[(size_t)b * C4 + q] +
                  reinterpret_cast<const f32x4*>(dpooled)[(size_t)b * C4 + q] * inv;
        const f32x4 yv = reinterpret_cast<const f32x4*>(y)[i];
        if (act == ORBIT_ACT_SILU) {
            const f32x4 z = yv * reinterpret_cast<const f32x4*>(scale)[q] + reinterpret_cast<const f32x4*>(shift)[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-z[k]));
                g[k] *= sg * (1.0f + z[k] * (1.0f - sg));
            }
        } else if (act == ORBIT_ACT_RELU) {
            const f32x4 z = yv * reinterpret_cast<const f32x4*>(scale)[q] + reinterpret_cast<const f32x4*>(shift)[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = z[k] > 0.f ? g[k] : 0.f;
        }
        const f32x4 xh = (yv - reinterpret_cast<const f32x4*>(mean)[q]) * reinterpret_cast<const f32x4*>(invstd)[q];
        const f32x4 k1 = reinterpret_cast<const f32x4*>(coef)[q];
        const f32x4 k2 = reinterpret_cast<const f32x4*>(coef + C)[q];
        const f32x4 k3 = reinterpret_cast<const f32x4*>(coef + 2 * C)[q];
        reinterpret_cast<f32x4*>(dy)[i] = k1 * (g - k2 - xh * k3);
    }
}

int launch_bn_backward_reduced_gated(const float* dxg, const float* gate, const float* dpooled, int HW, const BnTaped& t,
                                     const BnGrads& p, int train, int M, int C, float* dy, int nblk, float* coef, hipStream_t s) {
    const float* y = t.y;
    float* partial = t.partial;
    const int act = t.act;
    ORBIT_REQUIRE(C % 4 == 0 && M > 0 && HW > 0 && M % HW == 0 && nblk > 0 && dxg && gate && dpooled && y && partial && coef &&
                      !p.dbias,
                  "bn_backward_reduced_gated: bad arguments");
    ORBIT_REQUIRE(act != ORBIT_ACT_SILU || (t.bn.scale && t.bn.shift), "bn_backward_reduced_gated: SiLU needs the folded scale/shift");
    const float* src = partial;
    if (nblk > BN_COMPACT_ABOVE) {
        const int GS = cdiv(nblk, BN_COMPACT_TO), nout = cdiv(nblk, GS), cols4 = 2 * C / 4;
        float* out = partial + (size_t)nblk * 2 * C;
        const size_t items = (size_t)nout * cols4;
        const int rec = prof_start("bn_partial_compact", 2.0 * nblk * C, 4.0 * (nblk + nout) * 2.0 * C, s);
        bn_partial_compact_kernel<<<(unsigned)((items + 255) / 256), 256, 0, s>>>(partial, nblk, cols4, GS, nout, out);
        prof_stop(rec, s);
        ORBIT_LAUNCH_CHECK();
        src = out, nblk = nout;
    }
    bn_bwd_finalize_kernel<<<cdiv(C, BN_FIN_CH), 256, 0, s>>>(src, nblk, M, C, train, p.gamma, t.bn.invstd, p.dgamma, p.dbeta, nullptr,
                                                              coef);
    ORBIT_LAUNCH_CHECK();
    if (dy) {
        const size_t total4 = (size_t)M * (C / 4);
        ORBIT_REQUIRE((unsigned long long)total4 < (1ull << 32), "tensor too large for the 32-bit index arithmetic of this kernel");
        const unsigned per_frame4 = (unsigned)HW * (unsigned)(C / 4);
        const int B = M / HW;
        const int gx = std::max(1, std::min(cdiv((int)per_frame4, 256), cdiv(16384, B)));
        gate_bn_bwd_apply_kernel<<<dim3(gx, B), 256, 0, s>>>(dxg, gate, dpooled, y, t.bn.mean, t.bn.invstd, t.bn.scale, t.bn.shift,
                                                             coef, act, HW, C / 4, total4, dy);
        ORBIT_LAUNCH_CHECK();
    }
    return ORBIT_OK;
}

int launch_maxpool_idx(const float* x, float* y, uint8_t* idx, const LayerGeom& g, hipStream_t s) {
    const int B = g.B, H = g.H, W = g.W, C = g.Cin, K = g.KH, stride = g.stride, pad = g.pad_t, Ho = g.Ho, Wo = g.Wo;
    ORBIT_REQUIRE(C % 4 == 0 && K * K <= 255, "maxpool: C %% 4 != 0 or window too large");
    ORBIT_REQUIRE((unsigned long long)((size_t)B * Ho * Wo * (C / 4)) < (1ull << 32), "tensor too large for the 32-bit index arithmetic of this kernel");
    maxpool_idx_kernel<<<grid_for((size_t)B * Ho * Wo * (C / 4)), 256, 0, s>>>(x, y, idx, B, H, W, C / 4, K, stride, pad,
                                                                               Ho, Wo);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_maxpool_bwd(const float* dy, const uint8_t* idx, float* dx, const LayerGeom& g, hipStream_t s) {
    const int B = g.B, H = g.H, W = g.W, C = g.Cin, K = g.KH, stride = g.stride, pad = g.pad_t, Ho = g.Ho, Wo = g.Wo;
    ORBIT_REQUIRE(C % 4 == 0, "maxpool_backward: C %% 4 != 0");
    ORBIT_REQUIRE((unsigned long long)((size_t)B * H * W * (C / 4)) < (1ull << 32), "tensor too large for the 32-bit index arithmetic of this kernel");
    maxpool_bwd_kernel<<<grid_for((size_t)B * H * W * (C / 4)), 256, 0, s>>>(dy, idx, dx, B, H, W, C / 4, K, stride, pad,
                                                                             Ho, Wo);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_avgpool_bwd(const float* dy, float* dx, int B, int HW, int C, hipStream_t s) {
    ORBIT_REQUIRE(C % 4 == 0, "avgpool_backward: C %% 4 != 0");
    ORBIT_REQUIRE((unsigned long long)((size_t)B * HW * (C / 4)) < (1ull << 32), "tensor too large for the 32-bit index arithmetic of this kernel");
    avgpool_bwd_kernel<<<grid_for((size_t)B * HW * (C / 4)), 256, 0, s>>>(dy, dx, B, HW, C / 4);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_upsample_zero(const float* src, float* dst, int B, int H, int W, int C, int stride, int Hs, int Ws,
                         hipStream_t s) {
    ORBIT_REQUIRE(C % 4 == 0 && stride >= 1, "upsample_zero: C %% 4 != 0");
    ORBIT_REQUIRE((unsigned long long)((size_t)B * H * W * (C / 4)) < (1ull << 32), "tensor too large for the 32-bit index arithmetic of this kernel");
    upsample_zero_kernel<<<grid_for((size_t)B * H * W * (C / 4)), 256, 0, s>>>(src, dst, B, H, W, C / 4, stride, Hs, Ws);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// ---- prototype head backward: d(features) of logits = s*(q.W^T + b) or s*cos(q, w_c); q = mean of T frame rows -----
// one wave per query row; C <= 64 (dlogits of the row live in lane registers)
__global__ __launch_bounds__(256) void proto_predict_bwd_kernel(const float* __restrict__ dlogits,
                                                                const float* __restrict__ Q,
                                                                const float* __restrict__ Wt, int M, int T, int D,
                                                                int C, float logit_scale, int cosine,
                                                                float* __restrict__ dQ) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + wave;
    if (m >= M) return;
    const float invT = 1.0f / (float)T;
    const float* q = Q + (size_t)m * T * D;
    float* dq = dQ + (size_t)m * T * D;
    const float my_dl = lane < C ? dlogits[(size_t)m * C + lane] * logit_scale : 0.f;
    const int Dceil = (D + 63) & ~63;  // every lane runs every iteration: the shuffles below need the whole wave
    if (!cosine) {
        for (int d = lane; d < Dceil; d += 64) {
            float g = 0.f;
            for (int c = 0; c < C; ++c) g += __shfl(my_dl, c, 64) * (d < D ? Wt[(size_t)c * D + d] : 0.f);
            g *= invT;
            if (d < D)
                for (int t = 0; t < T; ++t) dq[(size_t)t * D + d] = g;
        }
        return;
    }
    // cosine: cos_c = q.w_c / (max(|q|, eps) max(|w_c|, eps))
    float qq = 0.f;
    for (int d = lane; d < D; d += 64) {
        float x = 0.f;
        for (int t = 0; t < T; ++t) x += q[(size_t)t * D + d];
        x *= invT;
        qq += x * x;
    }
    const float nq = sqrtf(wave_sum_xor(qq)), nqc = fmaxf(nq, 1e-8f);
    float a_c = 0.f, b_sum = 0.f;  // lane c keeps dl_c / (nq' nw'_c); b_sum = sum_c dl_c dot_c / (nq'^2 nw'_c nq)
    for (int c = 0; c < C; ++c) {
        float dot = 0.f, ww = 0.f;
        for (int d = lane; d < D; d += 64) {
            float x = 0.f;
            for (int t = 0; t < T; ++t) x += q[(size_t)t * D + d];
            x *= invT;
            const float w = Wt[(size_t)c * D + d];
            dot += x * w, ww += w * w;
        }
        dot = wave_sum_xor(dot);
        const float nwc = fmaxf(sqrtf(wave_sum_xor(ww)), 1e-8f);
        const float dl = __shfl(my_dl, c, 64);
        if (lane == c) a_c = dl / (nqc * nwc);
        if (nq > 1e-8f) b_sum += dl * dot / (nqc * nqc * nwc * nq);
    }
    for (int d = lane; d < Dceil; d += 64) {
        float x = 0.f;
        if (d < D) {
            for (int t = 0; t < T; ++t) x += q[(size_t)t * D + d];
            x *= invT;
        }
        float g = -b_sum * x;
        for (int c = 0; c < C; ++c) g += __shfl(a_c, c, 64) * (d < D ? Wt[(size_t)c * D + d] : 0.f);
        g *= invT;
        if (d < D)
            for (int t = 0; t < T; ++t) dq[(size_t)t * D + d] = g;
    }
}

// linear head parameter gradients: dW[c][d] = scale * sum_m dl[m][c] q[m][d], db[c] = scale * sum_m dl[m][c];
// thread = one feature column d, classes in chunks of 16 accumulators, rows in ascending order (deterministic)
__global__ __launch_bounds__(256) void linear_head_wgrad_kernel(const float* __restrict__ dl, const float* __restrict__ q,
                                                                int M, int D, int C, float scale,
                                                                float* __restrict__ dW, float* __restrict__ db) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    const int c0 = blockIdx.y * 16;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    float bacc = 0.f;  // thread d == 0..15 of block x == 0 also reduces the bias of class c0 + d
    for (int m = 0; m < M; ++m) {
        const float x = d < D ? q[(size_t)m * D + d] : 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (c0 + j < C) acc[j] = fmaf(dl[(size_t)m * C + c0 + j], x, acc[j]);
        if (blockIdx.x == 0 && threadIdx.x < 16 && c0 + threadIdx.x < C) bacc += dl[(size_t)m * C + c0 + threadIdx.x];
    }
    if (d < D) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (c0 + j < C) dW[(size_t)(c0 + j) * D + d] = scale * acc[j];
    }
    if (db && blockIdx.x == 0 && threadIdx.x < 16 && c0 + threadIdx.x < C) db[c0 + threadIdx.x] = scale * bacc;
}

}  // namespace orbit

using namespace orbit;

extern "C" {

int orbit_linear_head_backward(const float* dlogits, const float* features, int M, int D, int C, float logit_scale,
                               float* dweight, float* dbias, orbit_stream_t stream) {
    ORBIT_REQUIRE(dlogits && features && dweight, "linear_head_backward: null pointer");
    ORBIT_REQUIRE(M > 0 && D > 0 && C > 0, "linear_head_backward: bad sizes");
    linear_head_wgrad_kernel<<<dim3(cdiv(D, 256), cdiv(C, 16)), 256, 0, (hipStream_t)stream>>>(dlogits, features, M, D, C,
                                                                                             logit_scale, dweight, dbias);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int orbit_op_bn_train_forward(const float* y, int M, int C, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, const float* residual, int act,
                              float* out, float* save_mean, float* save_invstd, orbit_stream_t stream) {
    ORBIT_REQUIRE(y && out && save_mean && save_invstd, "op_bn_train_forward: null pointer");
    ORBIT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "op_bn_train_forward: running stats come in pairs");
    hipStream_t s = (hipStream_t)stream;
    float* tmp = nullptr;
    const size_t nfl = (size_t)bn_reduce_blocks(M, C) * 2 * C + 2 * (size_t)C;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&tmp), nfl * sizeof(float), s));
    float* scale = tmp + (size_t)bn_reduce_blocks(M, C) * 2 * C;
    const BnAffine a{gamma, beta, nullptr, running_mean, running_var, eps, momentum};
    int rc = launch_bn_stats(y, M, C, a, BnFold{save_mean, save_invstd, scale, scale + C}, tmp, s);
    if (rc == ORBIT_OK) rc = launch_scale_shift_act(y, scale, scale + C, residual, act, (size_t)M, C, out, s);
    (void)hipFreeAsync(tmp, s);
    return rc;
}

int orbit_op_bn_stats_from_gram(const float* x, int P, int Cin, const float* w, int C, float eps, float* save_mean,
                                float* save_invstd, orbit_stream_t stream) {
    ORBIT_REQUIRE(x && w && save_mean && save_invstd, "op_bn_stats_from_gram: null pointer");
    hipStream_t s = (hipStream_t)stream;
    float* tmp = nullptr;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&tmp), bn_gram_scratch_floats(P, Cin) * sizeof(float), s));
    BnAffine a;
    a.eps = eps;
    const int rc = launch_bn_stats_from_gram(x, P, Cin, w, C, a, BnFold{save_mean, save_invstd}, tmp, s);
    (void)hipFreeAsync(tmp, s);
    return rc;
}

int orbit_op_bn_backward(const float* dout, const float* out, const float* y, int M, int C, const float* gamma,
                         const float* mean, const float* invstd, int train, int act, float* dy, float* dres,
                         float* dgamma, float* dbeta, orbit_stream_t stream) {
    ORBIT_REQUIRE(dout && y && mean && invstd && dy, "op_bn_backward: null pointer");
    ORBIT_REQUIRE(act == ORBIT_ACT_NONE || out, "op_bn_backward: the activation output is needed for the ReLU mask");
    hipStream_t s = (hipStream_t)stream;
    float* tmp = nullptr;
    const size_t npart = (size_t)bn_reduce_blocks(M, C) * 2 * C;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&tmp), (npart + 3 * (size_t)C) * sizeof(float), s));
    ORBIT_REQUIRE(act != ORBIT_ACT_SILU, "op_bn_backward: SiLU is exercised through the network-level entry points");
    const int rc = launch_bn_backward(dout, out, y, BnFoldC{mean, invstd}, BnGrads{gamma, dgamma, dbeta}, train, act, M, C, dy,
                                      dres, 0, tmp, tmp + npart, s);
    (void)hipFreeAsync(tmp, s);
    return rc;
}

int orbit_op_bn_backward_ex(const float* dout, const float* out, const float* y, int M, int C, const float* gamma,
                            const float* mean, const float* invstd, const float* scale, const float* shift, int train, int act,
                            int flags, float* dy, float* dres, int dres_accumulate, float* dgamma, float* dbeta,
                            orbit_stream_t stream) {
    ORBIT_REQUIRE(dout && y && mean && invstd && dy, "op_bn_backward_ex: null pointer");
    ORBIT_REQUIRE((flags & ~ORBIT_BN_RESIDUAL_POST_ACT) == 0, "op_bn_backward_ex: unknown flags 0x%x", flags);
    ORBIT_REQUIRE(act == ORBIT_ACT_NONE || act == ORBIT_ACT_RELU || act == ORBIT_ACT_SILU, "op_bn_backward_ex: bad activation %d", act);
    ORBIT_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "op_bn_backward_ex: bad sizes M = %d, C = %d", M, C);
    const int res_post = (flags & ORBIT_BN_RESIDUAL_POST_ACT) ? 1 : 0;
    ORBIT_REQUIRE(act != ORBIT_ACT_RELU || out || res_post, "op_bn_backward_ex: the activation output is needed for the ReLU mask");
    ORBIT_REQUIRE((act != ORBIT_ACT_SILU && !(res_post && act == ORBIT_ACT_RELU)) || (scale && shift),
                  "op_bn_backward_ex: this form needs the folded scale / shift");
    hipStream_t s = (hipStream_t)stream;
    float* tmp = nullptr;
    const size_t npart = (size_t)bn_reduce_blocks(M, C) * 2 * C;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&tmp), (npart + 3 * (size_t)C) * sizeof(float), s));
    const int rc = launch_bn_backward(dout, out, y, BnFoldC{mean, invstd, scale, shift}, BnGrads{gamma, dgamma, dbeta}, train, act, M,
                                      C, dy, dres, dres_accumulate, tmp, tmp + npart, s, res_post);
    (void)hipFreeAsync(tmp, s);
    return rc;
}

int orbit_op_scale_shift_act(const float* y, const float* scale, const float* shift, const float* residual, int act, int M, int C,
                             int flags, float* out, orbit_stream_t stream) {
    ORBIT_REQUIRE(y && scale && shift && out, "op_scale_shift_act: null pointer");
    ORBIT_REQUIRE((flags & ~ORBIT_BN_RESIDUAL_POST_ACT) == 0, "op_scale_shift_act: unknown flags 0x%x", flags);
    ORBIT_REQUIRE(act == ORBIT_ACT_NONE || act == ORBIT_ACT_RELU || act == ORBIT_ACT_SILU, "op_scale_shift_act: bad activation %d", act);
    ORBIT_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "op_scale_shift_act: bad sizes M = %d, C = %d", M, C);
    return launch_scale_shift_act(y, scale, shift, residual, act, (size_t)M, C, out, (hipStream_t)stream,
                                  (flags & ORBIT_BN_RESIDUAL_POST_ACT) ? 1 : 0);
}

/* The layout rules of the per-channel reductions (host only), for the parity tests: col_layout, bn_reduce_blocks and
 * bn_rows_per_block of an [M][C] tensor. */
int orbit_op_bn_reduce_plan(int M, int C, int* G, int* R, int* ygroups, int* nblk, int* rows_per_block) {
    ORBIT_REQUIRE(G && R && ygroups && nblk && rows_per_block, "op_bn_reduce_plan: null pointer");
    ORBIT_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "op_bn_reduce_plan: bad sizes M = %d, C = %d", M, C);
    const ColLayout L = col_layout(C);
    *G = L.G, *R = L.R, *ygroups = L.ygroups, *nblk = bn_reduce_blocks(M, C), *rows_per_block = bn_rows_per_block(M, C);
    return ORBIT_OK;
}

/* ... and of the pooled apply pass (host only): se_pool_chunks and the rows of a chunk. */
int orbit_op_se_pool_chunks(int B, int HW, int C, int* chunks, int* rows_per_chunk) {
    ORBIT_REQUIRE(chunks && rows_per_chunk, "op_se_pool_chunks: null pointer");
    ORBIT_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 4 == 0, "op_se_pool_chunks: bad sizes B = %d, HW = %d, C = %d", B, HW, C);
    *chunks = se_pool_chunks(B, HW, C), *rows_per_chunk = cdiv(HW, *chunks);
    return ORBIT_OK;
}

/* The train-mode finalize from a producer's partial sums, single-operator entry for the parity tests: the caller's
 * partial[nblk][2][C] (sums of y and y^2 over M rows in all) is copied into scratch with room for the compaction stage, then
 * launch_bn_stats_from_partials runs as behind a conv epilogue. gamma / beta / conv_bias / scale+shift / running statistics nullable. */
int orbit_op_bn_stats_from_partials(const float* partial, int nblk, int M, int C, const float* gamma, const float* beta,
                                    const float* conv_bias, float eps, float momentum, float* running_mean, float* running_var,
                                    float* mean, float* invstd, float* scale, float* shift, orbit_stream_t stream) {
    ORBIT_REQUIRE(partial && mean && invstd, "op_bn_stats_from_partials: null pointer");
    ORBIT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "op_bn_stats_from_partials: running stats come in pairs");
    ORBIT_REQUIRE((scale == nullptr) == (shift == nullptr), "op_bn_stats_from_partials: scale and shift come in pairs");
    ORBIT_REQUIRE(nblk > 0 && M > 0 && C > 0 && C % 4 == 0, "op_bn_stats_from_partials: bad sizes nblk = %d, M = %d, C = %d", nblk, M, C);
    hipStream_t s = (hipStream_t)stream;
    float* tmp = nullptr;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&tmp), bn_partial_floats((size_t)nblk, C) * sizeof(float), s));
    const hipError_t e = hipMemcpyAsync(tmp, partial, (size_t)nblk * 2 * C * sizeof(float), hipMemcpyDeviceToDevice, s);
    int rc = e == hipSuccess ? ORBIT_OK : set_err(ORBIT_ERR_HIP, "%s: copying the partials failed: %s", "op_bn_stats_from_partials", hipGetErrorString(e));
    const BnAffine a{gamma, beta, conv_bias, running_mean, running_var, eps, momentum};
    if (rc == ORBIT_OK) rc = launch_bn_stats_from_partials(tmp, nblk, M, C, a, BnFold{mean, invstd, scale, shift}, s);
    (void)hipFreeAsync(tmp, s);
    return rc;
}

/* The BatchNorm backward behind a producer that already summed g and g * xhat (the depthwise and squeeze-excite backward kernels),
 * single-operator entry for the parity tests: partial[nblk][2][C] as above through launch_bn_backward_reduced. g is the gradient
 * at the BatchNorm's output (activation derivative applied); dy nullable. */
int orbit_op_bn_backward_reduced(const float* g, const float* y, const float* mean, const float* invstd, const float* gamma, int train,
                                 int M, int C, const float* partial, int nblk, float* dy, float* dgamma, float* dbeta,
                                 orbit_stream_t stream) {
    ORBIT_REQUIRE(g && y && mean && invstd && partial, "op_bn_backward_reduced: null pointer");
    ORBIT_REQUIRE(nblk > 0 && M > 0 && C > 0 && C % 4 == 0, "op_bn_backward_reduced: bad sizes nblk = %d, M = %d, C = %d", nblk, M, C);
    hipStream_t s = (hipStream_t)stream;
    float* tmp = nullptr;
    const size_t npart = bn_partial_floats((size_t)nblk, C);
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&tmp), (npart + 3 * (size_t)C) * sizeof(float), s));
    const hipError_t e = hipMemcpyAsync(tmp, partial, (size_t)nblk * 2 * C * sizeof(float), hipMemcpyDeviceToDevice, s);
    int rc = e == hipSuccess ? ORBIT_OK : set_err(ORBIT_ERR_HIP, "%s: copying the partials failed: %s", "op_bn_backward_reduced", hipGetErrorString(e));
    if (rc == ORBIT_OK)
        rc = launch_bn_backward_reduced(g, y, BnFoldC{mean, invstd}, BnGrads{gamma, dgamma, dbeta}, train, M, C, dy, tmp, nblk,
                                        tmp + npart, s);
    (void)hipFreeAsync(tmp, s);
    return rc;
}

/* out = act(scale * y + shift) for [B][HW][C] with the squeeze-excite pooling partials pool[B][chunks][C] of out from the same
 * pass (chunks as orbit_op_se_pool_chunks reports), single-operator entry for the parity tests. */
int orbit_op_scale_shift_act_pool(const float* y, const float* scale, const float* shift, int act, int B, int HW, int C, float* out,
                                  float* pool, orbit_stream_t stream) {
    ORBIT_REQUIRE(y && scale && shift && out && pool, "op_scale_shift_act_pool: null pointer");
    ORBIT_REQUIRE(act == ORBIT_ACT_NONE || act == ORBIT_ACT_RELU || act == ORBIT_ACT_SILU, "op_scale_shift_act_pool: bad activation %d", act);
    ORBIT_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 4 == 0, "op_scale_shift_act_pool: bad sizes B = %d, HW = %d, C = %d", B, HW, C);
    return launch_scale_shift_act_pool(y, scale, shift, act, B, HW, C, out, pool, (hipStream_t)stream);
}

int orbit_op_maxpool2d_train(const float* x, float* y, uint8_t* idx, int B, int H, int W, int C, int K, int stride,
                             int pad, int Ho, int Wo, orbit_stream_t stream) {
    ORBIT_REQUIRE(x && y && idx, "op_maxpool2d_train: null pointer");
    return launch_maxpool_idx(x, y, idx, LayerGeom{B, H, W, C, C, K, K, stride, pad, pad, Ho, Wo}, (hipStream_t)stream);
}

int orbit_op_maxpool2d_backward(const float* dy, const uint8_t* idx, float* dx, int B, int H, int W, int C, int K,
                                int stride, int pad, int Ho, int Wo, orbit_stream_t stream) {
    ORBIT_REQUIRE(dy && idx && dx, "op_maxpool2d_backward: null pointer");
    return launch_maxpool_bwd(dy, idx, dx, LayerGeom{B, H, W, C, C, K, K, stride, pad, pad, Ho, Wo}, (hipStream_t)stream);
}

int orbit_op_avgpool_backward(const float* dy, float* dx, int B, int HW, int C, orbit_stream_t stream) {
    ORBIT_REQUIRE(dy && dx, "op_avgpool_backward: null pointer");
    return launch_avgpool_bwd(dy, dx, B, HW, C, (hipStream_t)stream);
}

int orbit_proto_predict_backward(const float* dlogits, const float* features, const float* weight, int M, int T, int D,
                                 int C, float logit_scale, int cosine, float* dfeatures, orbit_stream_t stream) {
    ORBIT_REQUIRE(dlogits && features && weight && dfeatures, "proto_predict_backward: null pointer");
    ORBIT_REQUIRE(M > 0 && T > 0 && D > 0 && C > 0 && C <= 64, "proto_predict_backward: bad sizes (C must be <= 64)");
    proto_predict_bwd_kernel<<<cdiv(M, 4), 256, 0, (hipStream_t)stream>>>(dlogits, features, weight, M, T, D, C,
                                                                          logit_scale, cosine, dfeatures);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

}  // extern "C"
