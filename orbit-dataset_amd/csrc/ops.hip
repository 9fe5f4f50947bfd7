// HBM-bound layer kernels of the extractors (NHWC activations, channels innermost so every wave
// instruction moves 1 KiB of contiguous data): depthwise convolution (+ fused squeeze-excite pooling),
// max/avg pooling, squeeze-excite gate.
//
// Reference sites these stand in for (all run through ATen in the reference):
//   depthwise / SE / SiLU        timm tf_efficientnet_b0 blocks used by model/feature_extractors.py:39-43
//   max-pool, global avg-pool    model/set_encoders.py:101-118 and the ResNet/EfficientNet trunks
//   BatchNorm (eval) + FiLM      model/few_shot_recognisers.py:114-117,176-183 — never a kernel of its own:
//                                folded here to a per-channel (scale, shift) consumed by conv epilogues.
#include "common.h"
#include "device_util.h"
#include "se_gate.h"
#include <algorithm>

namespace orbit {

using v4f = __attribute__((ext_vector_type(4))) float;

// Input transform of the depthwise kernels (XF, DwInXf in common.h): the kernel reads the RAW output y of the producing
// convolution and applies that layer's BatchNorm + activation, act(y * scale[c] + shift[c]), as it loads - the activated tensor
// is never written. Used by the batch-statistics forward of passes that run no backward (csrc/extractor_train.hip): for those the
// separate activation pass (read y, write a) over the 6x-expanded tensor disappears. Same arithmetic as
// scale_shift_act_kernel, so the depthwise outputs are bit-identical to the two-pass form.
// BatchNorm-backward epilogue of the data-gradient use (DwBnBwd, common.h): g = dx * act'(z), z = y * scale + shift; the fast
// exp / rcp of the forward activation; returns g and adds g, g * xhat to the running sums
struct DwBnbVec {
    v4f sc, sh, mu, is;
};
__device__ __forceinline__ v4f dw_bnb(v4f dx, v4f yv, const DwBnbVec& b, int act, v4f& s0, v4f& s1) {
    const v4f z = yv * b.sc + b.sh;
    v4f g = dx;
    if (act == ORBIT_ACT_SILU) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-z[k]));
            g[k] *= sg * (1.0f + z[k] * (1.0f - sg));
        }
    } else if (act == ORBIT_ACT_RELU) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = z[k] > 0.f ? g[k] : 0.f;
    }
    s0 += g;
    s1 += g * ((yv - b.mu) * b.is);
    return g;
}
__device__ __forceinline__ v4f dw_xf(v4f v, v4f isc, v4f ish, int act) {
    v = v * isc + ish;
    if (act == ORBIT_ACT_RELU) {
        v[0] = fmaxf(v[0], 0.f), v[1] = fmaxf(v[1], 0.f), v[2] = fmaxf(v[2], 0.f), v[3] = fmaxf(v[3], 0.f);
    } else if (act == ORBIT_ACT_SILU) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] * __builtin_amdgcn_rcpf(1.0f + __expf(-v[k]));
    }
    return v;
}

__global__ __launch_bounds__(256) void dw_pack_kernel(const float* __restrict__ w, float* __restrict__ wp,
                                                      int C, int K) {
    const int total = C * K * K;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int c = i % C, tap = i / C;
        wp[i] = w[(size_t)c * K * K + tap];
    }
}

// ---- depthwise KxK + folded BN + activation + fused squeeze-excite pooling ---------------------------------
// HBM-bound (reads the 6x-expanded tensor once, writes the depthwise output once). Thread = 4 channels (float4) x
// 4 consecutive output columns of one output row: the (3*S + K) input columns a row of taps needs are loaded once
// and reused by the 4 outputs (K=5,S=1: 10 loads per output float4 instead of 25). The block's weights (its
// channel slice x K*K taps) sit in LDS. Every thread owns a FIXED channel quad, so its running sum of activated
// outputs is the squeeze-excite pooling partial: reduced across the block's column lanes in a fixed order and
// written to pool_partial[b][row_chunk][c] (deterministic; orbit se_gate sums the row chunks).
// STATS (all four depthwise kernels): instead of the squeeze-excite pooling partials [B][chunk][C], `pool_partial` receives
// the column sums AND sums of squares of the outputs, [B * chunks][2][C] - the per-block layout the train-mode BatchNorm
// finalize reads (csrc/train_ops.hip); the training forward launches these kernels without scale / shift / activation, so
// the sums are those of the raw depthwise outputs and BatchNorm needs no statistics pass of its own over y.
template <int K, int S, bool STATS = false, bool XF = false>
__global__ __launch_bounds__(256) void dwconv_se_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        float* __restrict__ y, const float* __restrict__ scale,
                                                        const float* __restrict__ shift,
                                                        float* __restrict__ pool_partial, int H, int W, int C,
                                                        int pad_t, int pad_l, int Ho, int Wo, int act, int cb4,
                                                        int rows_per_chunk, DwInXf xf = DwInXf{nullptr, nullptr, 0}) {
    constexpr int NCOL = 3 * S + K;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float4* wl = reinterpret_cast<float4*>(sm);             // [K*K][cb4]
    float4* red = wl + K * K * cb4;                         // [WL][cb4]
    const int b = blockIdx.z, chunk = blockIdx.y;
    const int c4_0 = blockIdx.x * cb4;
    const int WL = 256 / cb4;
    const int tid = threadIdx.x;
    const int lc = tid % cb4, lw = tid / cb4;
    const bool active = lw < WL;
    const int c = (c4_0 + lc) * 4;
    for (int i = tid; i < K * K * cb4; i += 256) {
        const int tap = i / cb4, cc = i % cb4;
        wl[i] = *reinterpret_cast<const float4*>(w + (size_t)tap * C + (c4_0 + cc) * 4);
    }
    __syncthreads();
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (scale) sc = *reinterpret_cast<const float4*>(scale + c);
    if (shift) sh = *reinterpret_cast<const float4*>(shift + c);
    float4 psum = make_float4(0.f, 0.f, 0.f, 0.f), psq = make_float4(0.f, 0.f, 0.f, 0.f);
    v4f isc = {1.f, 1.f, 1.f, 1.f}, ish = {0.f, 0.f, 0.f, 0.f};
    if (XF) isc = *reinterpret_cast<const v4f*>(xf.scale + c), ish = *reinterpret_cast<const v4f*>(xf.shift + c);
    const float* xb = x + (size_t)b * H * W * C + c;
    float* yb = y + (size_t)b * Ho * Wo * C + c;
    const int ho_end = min(Ho, (chunk + 1) * rows_per_chunk);
    const int WQ = (Wo + 3) >> 2;
    if (active) {
        for (int ho = chunk * rows_per_chunk; ho < ho_end; ++ho) {
            for (int wq = lw; wq < WQ; wq += WL) {
                float4 acc[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                const int wi0 = wq * 4 * S - pad_l;
#pragma unroll
                for (int kh = 0; kh < K; ++kh) {
                    const int hi = ho * S - pad_t + kh;
                    if ((unsigned)hi >= (unsigned)H) continue;  // uniform over the block's row
                    const float* xr = xb + (size_t)hi * W * C;
                    float4 col[NCOL];
#pragma unroll
                    for (int q = 0; q < NCOL; ++q) {
                        const int wi = wi0 + q;
                        col[q] = (unsigned)wi < (unsigned)W ? *reinterpret_cast<const float4*>(xr + (size_t)wi * C)
                                                            : make_float4(0.f, 0.f, 0.f, 0.f);
                        if (XF && (unsigned)wi < (unsigned)W) {
                            const v4f t = dw_xf((v4f){col[q].x, col[q].y, col[q].z, col[q].w}, isc, ish, xf.act);
                            col[q] = make_float4(t[0], t[1], t[2], t[3]);
                        }
                    }
#pragma unroll
                    for (int kw = 0; kw < K; ++kw) {
                        const float4 f = wl[(kh * K + kw) * cb4 + lc];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float4 v = col[j * S + kw];
                            acc[j].x = fmaf(v.x, f.x, acc[j].x);
                            acc[j].y = fmaf(v.y, f.y, acc[j].y);
                            acc[j].z = fmaf(v.z, f.z, acc[j].z);
                            acc[j].w = fmaf(v.w, f.w, acc[j].w);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int wo = wq * 4 + j;
                    if (wo < Wo) {
                        float4 o;
                        o.x = apply_act(acc[j].x * sc.x + sh.x, act);
                        o.y = apply_act(acc[j].y * sc.y + sh.y, act);
                        o.z = apply_act(acc[j].z * sc.z + sh.z, act);
                        o.w = apply_act(acc[j].w * sc.w + sh.w, act);
                        *reinterpret_cast<float4*>(yb + ((size_t)ho * Wo + wo) * C) = o;
                        psum.x += o.x, psum.y += o.y, psum.z += o.z, psum.w += o.w;
                        if (STATS) psq.x += o.x * o.x, psq.y += o.y * o.y, psq.z += o.z * o.z, psq.w += o.w * o.w;
                    }
                }
            }
        }
    }
    if (pool_partial == nullptr) return;
    if (active) red[lw * cb4 + lc] = psum;
    __syncthreads();
    const size_t prow = ((size_t)b * gridDim.y + chunk) * (STATS ? 2 : 1);
    if (tid < cb4) {
        float4 t = red[tid];
        for (int l = 1; l < WL; ++l) {
            const float4 u = red[l * cb4 + tid];
            t.x += u.x, t.y += u.y, t.z += u.z, t.w += u.w;
        }
        *reinterpret_cast<float4*>(pool_partial + prow * C + (c4_0 + tid) * 4) = t;
    }
    if (STATS) {
        __syncthreads();
        if (active) red[lw * cb4 + lc] = psq;
        __syncthreads();
        if (tid < cb4) {
            float4 t = red[tid];
            for (int l = 1; l < WL; ++l) {
                const float4 u = red[l * cb4 + tid];
                t.x += u.x, t.y += u.y, t.z += u.z, t.w += u.w;
            }
            *reinterpret_cast<float4*>(pool_partial + (prow + 1) * C + (c4_0 + tid) * 4) = t;
        }
    }
}

// ---- streaming depthwise, software-pipelined over the tap rows ----------------------------------------------------------
// Same mapping and outputs as dwconv_se_kernel. There the NCOL loads of a tap row are predicated (image border), which
// hipcc turns into one exec-mask branch per load and a vmcnt(0) before the row's FMAs: K exposed memory round trips per
// output group. Here every load is unconditional (column / row clamped to a valid address, the value multiplied by a
// 0/1 mask afterwards - the masks of the columns are computed once per column strip) and tap row kh+1 is requested
// before row kh is consumed, so the waits are counted and one row of loads is always in flight.
template <int K, int S, bool STATS = false, bool XF = false>
__global__ __launch_bounds__(256) void dwconv_pipe_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          float* __restrict__ y, const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          float* __restrict__ pool_partial, int H, int W, int C,
                                                          int pad_t, int pad_l, int Ho, int Wo, int act, int cb4,
                                                          int rows_per_chunk, DwInXf xf = DwInXf{nullptr, nullptr, 0}) {
    constexpr int NCOL = 3 * S + K;
    extern __shared__ __attribute__((aligned(16))) float smp[];
    v4f* wl = reinterpret_cast<v4f*>(smp);  // [K*K][cb4]
    v4f* red = wl + K * K * cb4;            // [WL][cb4]
    const int b = blockIdx.z, chunk = blockIdx.y;
    const int c4_0 = blockIdx.x * cb4;
    const int WL = 256 / cb4;
    const int tid = threadIdx.x;
    const int lc = tid % cb4, lw = tid / cb4;
    const bool active = lw < WL;
    const int c = (c4_0 + lc) * 4;
    for (int i = tid; i < K * K * cb4; i += 256) {
        const int tap = i / cb4, cc = i % cb4;
        wl[i] = *reinterpret_cast<const v4f*>(w + (size_t)tap * C + (c4_0 + cc) * 4);
    }
    __syncthreads();
    v4f sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f}, psum = {0.f, 0.f, 0.f, 0.f}, psq = {0.f, 0.f, 0.f, 0.f};
    if (scale) sc = *reinterpret_cast<const v4f*>(scale + c);
    if (shift) sh = *reinterpret_cast<const v4f*>(shift + c);
    v4f isc = {1.f, 1.f, 1.f, 1.f}, ish = {0.f, 0.f, 0.f, 0.f};
    if (XF) isc = *reinterpret_cast<const v4f*>(xf.scale + c), ish = *reinterpret_cast<const v4f*>(xf.shift + c);
    const float* xb = x + (size_t)b * H * W * C + c;
    float* yb = y + (size_t)b * Ho * Wo * C + c;
    const int ho_end = min(Ho, (chunk + 1) * rows_per_chunk);
    const int WQ = (Wo + 3) >> 2;
    if (active) {
        for (int wq = lw; wq < WQ; wq += WL) {
            const int wi0 = wq * 4 * S - pad_l;
            int coff[NCOL];
            float cm[NCOL];
#pragma unroll
            for (int q = 0; q < NCOL; ++q) {
                const bool ok = (unsigned)(wi0 + q) < (unsigned)W;
                coff[q] = ok ? (wi0 + q) * C : 0;
                cm[q] = ok ? 1.f : 0.f;
            }
            for (int ho = chunk * rows_per_chunk; ho < ho_end; ++ho) {
                const int hi0 = ho * S - pad_t;
                v4f bufA[NCOL], bufB[NCOL];
                auto load_row = [&](int kh, v4f* dst) {
                    const int hi = hi0 + kh;
                    const float* xr = xb + (size_t)((unsigned)hi < (unsigned)H ? hi : 0) * W * C;
#pragma unroll
                    for (int q = 0; q < NCOL; ++q) dst[q] = *reinterpret_cast<const v4f*>(xr + coff[q]);
                };
                v4f acc[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = (v4f){0.f, 0.f, 0.f, 0.f};
                auto consume = [&](int kh, const v4f* src) {
                    const float rm = (unsigned)(hi0 + kh) < (unsigned)H ? 1.f : 0.f;  // uniform over the block
                    v4f col[NCOL];
#pragma unroll
                    for (int q = 0; q < NCOL; ++q) col[q] = (XF ? dw_xf(src[q], isc, ish, xf.act) : src[q]) * (cm[q] * rm);
                    const v4f* wk = wl + (size_t)kh * K * cb4 + lc;
#pragma unroll
                    for (int kw = 0; kw < K; ++kw) {
                        const v4f f = wk[kw * cb4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] += col[j * S + kw] * f;
                    }
                };
                // a ROLLED loop over pairs of tap rows (two named buffers): fully unrolled, hipcc hoists the loads of all
                // K rows to the top (256 VGPRs, one wave per SIMD); this way exactly two rows are live
                load_row(0, bufA);
#pragma unroll 1
                for (int kh = 0; kh + 2 < K; kh += 2) {
                    load_row(kh + 1, bufB);
                    consume(kh, bufA);
                    load_row(kh + 2, bufA);
                    consume(kh + 1, bufB);
                }
                consume(K - 1, bufA);  // K is odd: the last row sits in bufA
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int wo = wq * 4 + j;
                    if (wo < Wo) {
                        v4f o = acc[j] * sc + sh;
                        o[0] = apply_act(o[0], act), o[1] = apply_act(o[1], act), o[2] = apply_act(o[2], act), o[3] = apply_act(o[3], act);
                        *reinterpret_cast<v4f*>(yb + ((size_t)ho * Wo + wo) * C) = o;
                        psum += o;
                        if (STATS) psq += o * o;
                    }
                }
            }
        }
    }
    if (pool_partial == nullptr) return;
    if (active) red[lw * cb4 + lc] = psum;
    __syncthreads();
    const size_t prow = ((size_t)b * gridDim.y + chunk) * (STATS ? 2 : 1);
    if (tid < cb4) {
        v4f t = red[tid];
        for (int l = 1; l < WL; ++l) t += red[l * cb4 + tid];
        *reinterpret_cast<v4f*>(pool_partial + prow * C + (c4_0 + tid) * 4) = t;
    }
    if (STATS) {
        __syncthreads();
        if (active) red[lw * cb4 + lc] = psq;
        __syncthreads();
        if (tid < cb4) {
            v4f t = red[tid];
            for (int l = 1; l < WL; ++l) t += red[l * cb4 + tid];
            *reinterpret_cast<v4f*>(pool_partial + (prow + 1) * C + (c4_0 + tid) * 4) = t;
        }
    }
}

// ---- depthwise with a vertical sliding window in registers ---------------------------------------------------------
// Same mapping and outputs as dwconv_se_kernel, but a thread walks DOWN its column strip keeping the last K input rows
// (K x NCOL quads) in registers: every output row loads only the S new input rows instead of all K, i.e. 3-5x fewer
// L1/L2 requests (the plain kernel re-reads each input ~K*NCOL/NOUT times and is L2-bandwidth-bound on the 5x5 layers).
// The ring slot of an input row is static: the row loop is unrolled over one ring period (K steps).
// WG (with BNB, the data-gradient use): the layer's filter gradient rides along (DwBnBwd::wgrad_partial) - the window holds
// dy, the layer's input at the output pixel is act(y * scale + shift), and window element (kh, j + kw) times that input is the
// (K-1-kh, K-1-kw) tap's term (the data gradient runs with flipped taps): K*K accumulators per thread, one [K*K][C] partial row
// per block.
template <int K, int S, int NOUT, bool STATS = false, bool XF = false, bool BNB = false, bool WG = false>
__global__ __launch_bounds__(256) void dwconv_win_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         float* __restrict__ y, const float* __restrict__ scale,
                                                         const float* __restrict__ shift,
                                                         float* __restrict__ pool_partial, int H, int W, int C,
                                                         int pad_t, int pad_l, int Ho, int Wo, int act, int cb4,
                                                         int rows_per_chunk, DwInXf xf = DwInXf{nullptr, nullptr, 0},
                                                         DwBnBwd bnb = DwBnBwd{}) {
    constexpr int NCOL = (NOUT - 1) * S + K;
    extern __shared__ __attribute__((aligned(16))) float smw[];
    v4f* wl = reinterpret_cast<v4f*>(smw);  // [K*K][cb4]
    v4f* red = wl + K * K * cb4;            // [WL][cb4]
    const int b = blockIdx.z, chunk = blockIdx.y;
    const int c4_0 = blockIdx.x * cb4;
    const int WL = 256 / cb4;
    const int tid = threadIdx.x;
    const int lc = tid % cb4, lw = tid / cb4;
    const bool active = lw < WL;
    const int c = (c4_0 + lc) * 4;
    for (int i = tid; i < K * K * cb4; i += 256) {
        const int tap = i / cb4, cc = i % cb4;
        wl[i] = *reinterpret_cast<const v4f*>(w + (size_t)tap * C + (c4_0 + cc) * 4);
    }
    __syncthreads();
    v4f sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f}, psum = {0.f, 0.f, 0.f, 0.f}, psq = {0.f, 0.f, 0.f, 0.f};
    if (scale) sc = *reinterpret_cast<const v4f*>(scale + c);
    if (shift) sh = *reinterpret_cast<const v4f*>(shift + c);
    v4f isc = {1.f, 1.f, 1.f, 1.f}, ish = {0.f, 0.f, 0.f, 0.f};
    if (XF) isc = *reinterpret_cast<const v4f*>(xf.scale + c), ish = *reinterpret_cast<const v4f*>(xf.shift + c);
    const float* xb = x + (size_t)b * H * W * C + c;
    float* yb = y + (size_t)b * Ho * Wo * C + c;
    DwBnbVec bv;
    const float* byb = nullptr;
    if (BNB) {
        bv.sc = *reinterpret_cast<const v4f*>(bnb.bn.scale + c), bv.sh = *reinterpret_cast<const v4f*>(bnb.bn.shift + c);
        bv.mu = *reinterpret_cast<const v4f*>(bnb.bn.mean + c), bv.is = *reinterpret_cast<const v4f*>(bnb.bn.invstd + c);
        byb = bnb.y + (size_t)b * Ho * Wo * C + c;
    }
    v4f wacc[WG ? K * K : 1];
#pragma unroll
    for (int t = 0; t < (WG ? K * K : 1); ++t) wacc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
    const int ho0 = chunk * rows_per_chunk;
    const int ho_end = min(Ho, ho0 + rows_per_chunk);
    const int WQ = (Wo + NOUT - 1) / NOUT;
    if (active) {
        for (int wq = lw; wq < WQ; wq += WL) {
            const int wi0 = wq * NOUT * S - pad_l;
            int coff[NCOL];
            float cmask[NCOL];
#pragma unroll
            for (int q = 0; q < NCOL; ++q) {
                const bool ok = (unsigned)(wi0 + q) < (unsigned)W;
                coff[q] = ok ? (wi0 + q) * C : 0;
                cmask[q] = ok ? 1.f : 0.f;
            }
            v4f win[K][NCOL];
            auto load_row = [&](int hi, v4f* dst) {
                const bool row_ok = (unsigned)hi < (unsigned)H;
                const float* xr = xb + (size_t)(row_ok ? hi : 0) * W * C;
                const float rm = row_ok ? 1.f : 0.f;
#pragma unroll
                for (int q = 0; q < NCOL; ++q) {
                    const v4f raw = *reinterpret_cast<const v4f*>(xr + coff[q]);
                    dst[q] = (XF ? dw_xf(raw, isc, ish, xf.act) : raw) * (rm * cmask[q]);
                }
            };
            const int hi_base = ho0 * S - pad_t;  // input row of ring position 0
#pragma unroll
            for (int r = 0; r < K - S; ++r) load_row(hi_base + r, win[r]);
            for (int hob = ho0; hob < ho_end; hob += K) {
                const int rel = (hob - ho0) * S;  // multiple of K: ring slots below are static
#pragma unroll
                for (int ph = 0; ph < K; ++ph) {
                    const int ho = hob + ph;
                    if (ho < ho_end) {
#pragma unroll
                        for (int s2 = 0; s2 < S; ++s2)
                            load_row(hi_base + rel + ph * S + K - S + s2, win[(ph * S + K - S + s2) % K]);
                        v4f yv[NOUT];  // BNB: the producer's raw outputs under this row's results, in flight with the row above
                        if (BNB) {
#pragma unroll
                            for (int j = 0; j < NOUT; ++j)
                                yv[j] = *reinterpret_cast<const v4f*>(byb + ((size_t)ho * Wo + min(wq * NOUT + j, Wo - 1)) * C);
                        }
                        v4f ain[WG ? NOUT : 1];  // WG: the layer's input at the NOUT pixels (0 beyond the row's end)
                        if (WG) {
#pragma unroll
                            for (int j = 0; j < NOUT; ++j) {
                                ain[j] = dw_xf(yv[j], bv.sc, bv.sh, bnb.act);
                                if (wq * NOUT + j >= Wo) ain[j] = (v4f){0.f, 0.f, 0.f, 0.f};
                            }
                        }
                        v4f acc[NOUT];
#pragma unroll
                        for (int j = 0; j < NOUT; ++j) acc[j] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int kh = 0; kh < K; ++kh) {
#pragma unroll
                            for (int kw = 0; kw < K; ++kw) {
                                const v4f f = wl[(kh * K + kw) * cb4 + lc];
#pragma unroll
                                for (int j = 0; j < NOUT; ++j) {
                                    acc[j] += win[(ph * S + kh) % K][j * S + kw] * f;
                                    if (WG) wacc[kh * K + kw] += win[(ph * S + kh) % K][j * S + kw] * ain[j];
                                }
                            }
                        }
#pragma unroll
                        for (int j = 0; j < NOUT; ++j) {
                            const int wo = wq * NOUT + j;
                            if (wo < Wo) {
                                if (BNB) {
                                    *reinterpret_cast<v4f*>(yb + ((size_t)ho * Wo + wo) * C) = dw_bnb(acc[j], yv[j], bv, bnb.act, psum, psq);
                                } else {
                                    v4f o = acc[j] * sc + sh;
                                    o[0] = apply_act(o[0], act), o[1] = apply_act(o[1], act), o[2] = apply_act(o[2], act),
                                    o[3] = apply_act(o[3], act);
                                    *reinterpret_cast<v4f*>(yb + ((size_t)ho * Wo + wo) * C) = o;
                                    psum += o;
                                    if (STATS) psq += o * o;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    if (pool_partial == nullptr) return;
    if (active) red[lw * cb4 + lc] = psum;
    __syncthreads();
    const size_t prow = ((size_t)b * gridDim.y + chunk) * (STATS ? 2 : 1);
    if (tid < cb4) {
        v4f t = red[tid];
        for (int l = 1; l < WL; ++l) t += red[l * cb4 + tid];
        *reinterpret_cast<v4f*>(pool_partial + prow * C + (c4_0 + tid) * 4) = t;
    }
    if (STATS) {
        __syncthreads();
        if (active) red[lw * cb4 + lc] = psq;
        __syncthreads();
        if (tid < cb4) {
            v4f t = red[tid];
            for (int l = 1; l < WL; ++l) t += red[l * cb4 + tid];
            *reinterpret_cast<v4f*>(pool_partial + (prow + 1) * C + (c4_0 + tid) * 4) = t;
        }
    }
    if (WG) {
        // this block's filter-gradient partial row: taps in rounds of 8 through an [8][256] buffer, column lanes added in order;
        // accumulator t belongs to tap K*K - 1 - t (flipped taps)
        v4f* wred = wl + K * K * cb4;
        constexpr int TB = 8;
        const size_t wrow = (size_t)b * gridDim.y + chunk;
#pragma unroll
        for (int t0 = 0; t0 < K * K; t0 += TB) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < TB; ++u)
                if (t0 + u < K * K) wred[u * 256 + tid] = active ? wacc[t0 + u] : (v4f){0.f, 0.f, 0.f, 0.f};
            __syncthreads();
            for (int i = tid; i < TB * cb4; i += 256) {
                const int u = i / cb4, cc = i - u * cb4;
                if (t0 + u < K * K) {
                    v4f t = wred[u * 256 + cc];
                    for (int l = 1; l < WL; ++l) t += wred[u * 256 + l * cb4 + cc];
                    *reinterpret_cast<v4f*>(bnb.wgrad_partial + (wrow * K * K + (K * K - 1 - (t0 + u))) * C + (c4_0 + cc) * 4) = t;
                }
            }
        }
    }
}

// ---- depthwise through an LDS input patch -----------------------------------------------------------------------------
// The streaming kernels above read every input K*NCOL/NOUT times from the vector L1 (10x for 5x5): on the 5x5 layers that
// L1 traffic, not HBM, is the limit (1.8-2.0 TB/s of algorithmic bytes, tools/dw_bench.py). Here a block stages the input
// patch of (row chunk) x (full width) x (cs4 channel quads) in LDS once - every input element crosses the L1 exactly
// once - and the taps are ds_read_b128 (4x the L1's bytes per clock). Pixel stride is padded by one quad so that the
// lanes of a read (same channel quad, neighbouring pixels) spread over the banks.
// Thread = channel quad x (4-column output group, row lane); outputs, pooling partials and chunking as dwconv_se_kernel.
template <int K, int S, int U, bool STATS = false, bool XF = false, bool BNB = false>
__global__ __launch_bounds__(256) void dwconv_lds_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         float* __restrict__ y, const float* __restrict__ scale,
                                                         const float* __restrict__ shift,
                                                         float* __restrict__ pool_partial, int H, int W, int C,
                                                         int pad_t, int pad_l, int Ho, int Wo, int act, int cs4,
                                                         int rows_per_chunk, int G, int IWA,
                                                         DwInXf xf = DwInXf{nullptr, nullptr, 0}, DwBnBwd bnb = DwBnBwd{}) {
    constexpr int NCOL = 3 * S + K;
    extern __shared__ __attribute__((aligned(16))) float sml[];
    const int CSP = cs4 * 4 + 4;                     // padded pixel stride (floats)
    const int b = blockIdx.z, chunk = blockIdx.y;
    const int c0 = blockIdx.x * cs4 * 4;
    const int ho0 = chunk * rows_per_chunk;
    const int TH = min(Ho, ho0 + rows_per_chunk) - ho0;
    const int IH = (TH - 1) * S + K;
    const int IHmax = (rows_per_chunk - 1) * S + K;
    float* tile = sml;                               // [IH][IWA][CSP]
    v4f* wl = reinterpret_cast<v4f*>(sml + (size_t)IHmax * IWA * CSP);  // [K*K][cs4]
    v4f* red = wl + K * K * cs4;                     // [P][cs4]
    const int tid = threadIdx.x;
    const int lc = tid % cs4, p = tid / cs4, P = 256 / cs4;
    const int c = c0 + lc * 4;
    // the block's filter taps (<= 2 quads per thread: K*K*cs4 <= 400) are requested first and written to LDS after the
    // patch loads below have been issued: one round trip for both instead of two in a row
    v4f wq[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = tid + u * 256;
        if (i < K * K * cs4) wq[u] = *reinterpret_cast<const v4f*>(w + (size_t)(i / cs4) * C + c0 + (i % cs4) * 4);
    }
    {   // stage the patch (zero outside the image: TF-SAME / symmetric padding alike). A thread walks the patch pixels
        // p, p + P, ... of its channel quad; the loads of a batch of 8 are all issued before the first LDS store (one
        // load -> store round trip per pixel would serialise 5-8 HBM latencies per block)
        const int hi0 = ho0 * S - pad_t;
        const float* xb = x + (size_t)b * H * W * C + c;
        const int n_items = IH * IWA;
        const int dr = P / IWA, dc = P % IWA;   // walk step in (row, col)
        int r = p / IWA, col = p % IWA;
        for (int i0 = p; i0 < n_items; i0 += U * P) {
            v4f v[U];
            int dst[U];
            unsigned loaded = 0;  // XF: the transform applies to pixels of the image only (the zero padding stays zero)
            v4f xsc = {1.f, 1.f, 1.f, 1.f}, xsh = {0.f, 0.f, 0.f, 0.f};
            if (XF) xsc = *reinterpret_cast<const v4f*>(xf.scale + c), xsh = *reinterpret_cast<const v4f*>(xf.shift + c);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = i0 + u * P < n_items;
                const int hi = hi0 + r, wi = col - pad_l;
                v[u] = (v4f){0.f, 0.f, 0.f, 0.f};
                dst[u] = in ? (r * IWA + col) * CSP + lc * 4 : -1;
                if (in && (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W) {
                    v[u] = *reinterpret_cast<const v4f*>(xb + ((size_t)hi * W + wi) * C);
                    loaded |= 1u << u;
                }
                r += dr, col += dc;
                if (col >= IWA) col -= IWA, ++r;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (dst[u] >= 0)
                    *reinterpret_cast<v4f*>(tile + dst[u]) = (XF && ((loaded >> u) & 1u)) ? dw_xf(v[u], xsc, xsh, xf.act) : v[u];
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
        if (tid + u * 256 < K * K * cs4) wl[tid + u * 256] = wq[u];
    __syncthreads();
    v4f sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f}, psum = {0.f, 0.f, 0.f, 0.f}, psq = {0.f, 0.f, 0.f, 0.f};
    if (scale) sc = *reinterpret_cast<const v4f*>(scale + c);
    if (shift) sh = *reinterpret_cast<const v4f*>(shift + c);
    const int RL = P / G;                            // row lanes
    const int g = p % G, rl = p / G;
    float* yb = y + (size_t)b * Ho * Wo * C + c;
    DwBnbVec bv;
    const float* byb = nullptr;
    if (BNB) {
        bv.sc = *reinterpret_cast<const v4f*>(bnb.bn.scale + c), bv.sh = *reinterpret_cast<const v4f*>(bnb.bn.shift + c);
        bv.mu = *reinterpret_cast<const v4f*>(bnb.bn.mean + c), bv.is = *reinterpret_cast<const v4f*>(bnb.bn.invstd + c);
        byb = bnb.y + (size_t)b * Ho * Wo * C + c;
    }
    if (rl < RL) {
        for (int ro = rl; ro < TH; ro += RL) {
            v4f acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = (v4f){0.f, 0.f, 0.f, 0.f};
            const float* t0 = tile + ((size_t)(ro * S) * IWA + g * 4 * S) * CSP + lc * 4;
            const v4f* wk = wl + lc;
            const int ho = ho0 + ro;
            v4f yv[4];  // BNB: the producer's raw outputs under these four results, in flight with the tap loop
            if (BNB) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    yv[j] = *reinterpret_cast<const v4f*>(byb + ((size_t)ho * Wo + min(g * 4 + j, Wo - 1)) * C);
            }
            // a real loop over the tap rows: fully unrolled, the compiler hoists all K*(NCOL + K) LDS reads (260 VGPRs,
            // one wave per SIMD); one tap row is NCOL + K reads in flight and 4*K quad FMAs
#pragma unroll 1
            for (int kh = 0; kh < K; ++kh) {
                v4f col[NCOL];
#pragma unroll
                for (int q = 0; q < NCOL; ++q) col[q] = *reinterpret_cast<const v4f*>(t0 + q * CSP);
#pragma unroll
                for (int kw = 0; kw < K; ++kw) {
                    const v4f f = wk[kw * cs4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] += col[j * S + kw] * f;
                }
                t0 += IWA * CSP;
                wk += K * cs4;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int wo = g * 4 + j;
                if (wo < Wo) {
                    if (BNB) {
                        *reinterpret_cast<v4f*>(yb + ((size_t)ho * Wo + wo) * C) = dw_bnb(acc[j], yv[j], bv, bnb.act, psum, psq);
                    } else {
                        v4f o = acc[j] * sc + sh;
                        o[0] = apply_act(o[0], act), o[1] = apply_act(o[1], act), o[2] = apply_act(o[2], act), o[3] = apply_act(o[3], act);
                        *reinterpret_cast<v4f*>(yb + ((size_t)ho * Wo + wo) * C) = o;
                        psum += o;
                        if (STATS) psq += o * o;
                    }
                }
            }
        }
    }
    if (pool_partial == nullptr) return;
    red[p * cs4 + lc] = psum;
    __syncthreads();
    const size_t prow = ((size_t)b * gridDim.y + chunk) * (STATS ? 2 : 1);
    if (tid < cs4) {
        v4f t = red[tid];
        for (int l = 1; l < P; ++l) t += red[l * cs4 + tid];
        *reinterpret_cast<v4f*>(pool_partial + prow * C + c0 + tid * 4) = t;
    }
    if (STATS) {
        __syncthreads();
        red[p * cs4 + lc] = psq;
        __syncthreads();
        if (tid < cs4) {
            v4f t = red[tid];
            for (int l = 1; l < P; ++l) t += red[l * cs4 + tid];
            *reinterpret_cast<v4f*>(pool_partial + (prow + 1) * C + c0 + tid * 4) = t;
        }
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void se_gate2_kernel(const float* __restrict__ partial, int chunks, float inv_hw,
                                                       const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2t, const float* __restrict__ b2,
                                                       float* __restrict__ gate, int C, int R,
                                                       float* __restrict__ pooled_out) {
    extern __shared__ __attribute__((aligned(16))) float sm2[];  // [C] pooled, [R] hidden
    const int b = blockIdx.x;
    se_gate_frame<NT, 4>(partial + (size_t)b * chunks * C, chunks, inv_hw, w1, b1, w2t, b2, gate + (size_t)b * C, C, R,
                         pooled_out ? pooled_out + (size_t)b * C : nullptr, sm2);
}

__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int rows,
                                                        int cols) {
    const int total = rows * cols;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int r = i / cols, c = i % cols;
        out[(size_t)c * rows + r] = in[i];
    }
}

// ---- max-pool NHWC ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                      int B, int H, int W, int C, int K, int stride, int pad,
                                                      int Ho, int Wo) {
    const int C4 = C >> 2;
    const size_t total = (size_t)B * Ho * Wo * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        // 32-bit index arithmetic (the launcher checks total < 2^32): 64-bit div / mod are ~100 instructions each
        const unsigned iu = (unsigned)i, r1 = iu / (unsigned)C4, r2 = r1 / (unsigned)Wo, bu = r2 / (unsigned)Ho;
        const int c = (int)(iu - r1 * C4) * 4, wo = (int)(r1 - r2 * Wo), ho = (int)(r2 - bu * Ho), b = (int)bu;
        const float* xb = x + (size_t)b * H * W * C + c;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int kh = 0; kh < K; ++kh) {
            const int hi = ho * stride - pad + kh;
            if ((unsigned)hi >= (unsigned)H) continue;
            for (int kw = 0; kw < K; ++kw) {
                const int wi = wo * stride - pad + kw;
                if ((unsigned)wi >= (unsigned)W) continue;
                const float4 v = *reinterpret_cast<const float4*>(xb + ((size_t)hi * W + wi) * C);
                m.x = fmaxf(m.x, v.x), m.y = fmaxf(m.y, v.y), m.z = fmaxf(m.z, v.z), m.w = fmaxf(m.w, v.w);
            }
        }
        *reinterpret_cast<float4*>(y + (((size_t)b * Ho + ho) * Wo + wo) * C + c) = m;
    }
}

// ---- global average pool NHWC [B][HW][C] -> [B][C] -----------------------------------------------
// grid (ceil(C/64), B); 256 threads = 64 channels x 4 interleaved spatial slices, combined through LDS in
// a fixed order (deterministic).
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                      int HW, int C) {
    __shared__ float part[4][64];
    const int b = blockIdx.y;
    const int cl = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    float s = 0.f;
    if (c < C) {
        const float* p = x + (size_t)b * HW * C + c;
        for (int i = slice; i < HW; i += 4) s += p[(size_t)i * C];
    }
    part[slice][cl] = s;
    __syncthreads();
    if (slice == 0 && c < C)
        y[(size_t)b * C + c] = (part[0][cl] + part[1][cl] + part[2][cl] + part[3][cl]) / (float)HW;
}

// ---- squeeze-excite gate: one block per frame ------------------------------------------------------
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ pooled,
                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      float* __restrict__ gate, int C, int R) {
    extern __shared__ float sm[];  // [C] pooled, [R] hidden
    float* sp = sm;
    float* hid = sm + C;
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) sp[c] = pooled[(size_t)b * C + c];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < R; r += 4) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s = fmaf(w1[(size_t)r * C + c], sp[c], s);
        s = wave_sum_xor(s);
        if (lane == 0) {
            s += b1[r];
            hid[r] = s / (1.0f + expf(-s));  // SiLU
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = b2[c];
        for (int r = 0; r < R; ++r) s = fmaf(w2[(size_t)c * R + r], hid[r], s);
        gate[(size_t)b * C + c] = 1.0f / (1.0f + expf(-s));
    }
}

static int grid_for(size_t total) {
    size_t b = (total + 255) / 256;
    return (int)(b > 8192 ? 8192 : (b == 0 ? 1 : b));
}

// channel quads per block: the largest divisor of C/4 that is <= 64 (keeps every thread on a fixed channel quad)
static int dw_cb4(int C) {
    const int c4 = C / 4;
    for (int d = c4 < 64 ? c4 : 64; d >= 1; --d)
        if (c4 % d == 0) return d;
    return 1;
}
static int dwconv_se_rows_per_chunk(int Ho) { return Ho >= 56 ? 8 : (Ho >= 14 ? 7 : Ho); }
int dwconv_se_chunks(int Ho) { return cdiv(Ho, dwconv_se_rows_per_chunk(Ho)); }

// The kernel form the options and the measured rules prefer for a (K, stride) layer with Ho output rows, before any fit check
// (dw_lds / dw_window / dw_pipe: 1 = auto, 0 = never, 2 = always; read here and nowhere else). train_form: the statistics
// epilogue, with the input transform applied per load. lds_fits = false: what dw_plan falls back to when the patch does not fit.
DwForm dw_form_rule(int K, int stride, int Ho, bool train_form, bool lds_fits) {
    // LDS patch, measured (tools/dw_bench.py, 200 frames): 5x5 stride 1 -39..-41 % time (28x240, 14x480, 14x672), -15 % at
    // 7x1152; 3x3 stride 1 on <= 14 rows -10..-20 %; stride 2 and the large 3x3 maps are faster through the streaming kernels.
    // Train form (tools/dw_train_bench.py): the small stride-2 map (14 -> 7 rows, 5x5) 158 -> 84 us through the LDS patch (the
    // transform once per element instead of once per tap)
    const int lds_opt = get_option("dw_lds");
    if (lds_fits && (lds_opt == 2 || (lds_opt == 1 && ((stride == 1 && (K == 5 || Ho <= 14)) || (train_form && stride == 2 && Ho < 14)))))
        return DW_LDS;
    // register window, measured in-process against the plain streaming kernel (tools/dw_bench.py): +30..45 % on 3x3 / stride 1
    // with >= 14 rows (112x32, 56x144, 14x480), slower on 5x5 (K x NCOL window -> 256 VGPRs, 1 wave/SIMD) and on stride 2
    const int win_opt = get_option("dw_window");
    if (win_opt == 2 || (win_opt == 1 && K == 3 && stride == 1 && Ho >= 14)) return DW_WINDOW;
    // software-pipelined streaming: measured +5..9 % on the large stride-2 layers (112x96 3x3, 56x144 5x5), slower on the small
    // maps (two tap rows of registers -> 2 waves per SIMD); train form: also the 28 -> 14 row layer, 102 -> 60 us
    const int pipe_opt = get_option("dw_pipe");
    if (pipe_opt == 2 || (pipe_opt == 1 && stride == 2 && Ho >= (train_form ? 14 : 28))) return DW_PIPE;
    return DW_STREAM;
}

// whether launch_dwconv_se runs a (K, stride) layer with Ho output rows through the register-window kernel (the form that can
// carry the filter gradient, DwBnBwd::wgrad_partial). A function of the rule alone, so conservative: false wherever the LDS rule
// claims the shape, even if its patch would not fit and the launch falls back to the window
bool dwconv_se_window_form(int K, int stride, int Ho) { return dw_form_rule(K, stride, Ho, false) == DW_WINDOW; }

// the form launch_dwconv_se launches and its geometry
struct DwPlan {
    DwForm form;
    int cb4, rpc;  // channel quads per block (streaming forms), output rows per chunk
    dim3 grid;     // (channel slices, row chunks, frames) of the chosen form
    size_t lds;    // its dynamic LDS bytes
    int cs4, G, IWA;  // LDS form: channel quads per block, 4-column output groups, patch width
    bool deep;        // LDS form: 12 staging loads in flight instead of 8
};
static DwPlan dw_plan(int B, int C, int K, int stride, int Ho, int Wo, bool train_form) {
    DwPlan p{};
    p.cb4 = dw_cb4(C), p.rpc = dwconv_se_rows_per_chunk(Ho);
    p.form = dw_form_rule(K, stride, Ho, train_form);
    if (p.form == DW_LDS) {
        const int c4 = C / 4;
        p.G = cdiv(Wo, 4);
        // channel quads per block (a pixel's slice stays >= 64 contiguous bytes): the widest slice (longest contiguous run per
        // pixel) whose (256 / cs4) / G row lanes cover the chunk's rows in at most two passes; else the narrowest that fits
        for (int cand : {16, 8, 4}) {
            if (c4 % cand != 0 || p.G > 256 / cand) continue;
            p.cs4 = cand;
            if (2 * ((256 / cand) / p.G) >= p.rpc) break;
        }
        p.IWA = (4 * p.G - 1) * stride + K;
        const int IHmax = (p.rpc - 1) * stride + K;
        p.lds = ((size_t)IHmax * p.IWA * (p.cs4 * 4 + 4)) * sizeof(float) + (size_t)(K * K * p.cs4 + 256) * sizeof(float4);
        if (p.cs4 != 0 && p.lds <= 64 * 1024) {
            p.grid = dim3(c4 / p.cs4, cdiv(Ho, p.rpc), B);
            // staging batch per thread: 8 loads in flight, 12 where a thread owns more than 8 patch pixels (7x7 maps with
            // 16-quad slices: one HBM round trip instead of two, +6 %; elsewhere 12 is neutral or slightly worse)
            p.deep = IHmax * p.IWA > 8 * (256 / p.cs4);
            return p;
        }
        p.form = dw_form_rule(K, stride, Ho, train_form, false);
    }
    p.grid = dim3(C / 4 / p.cb4, cdiv(Ho, p.rpc), B);
    p.lds = (size_t)(K * K * p.cb4 + (256 / p.cb4) * p.cb4) * sizeof(float4);
    return p;
}

// The data-gradient use of the launch below (DwBnBwd): the LDS patch and the register window carry the BatchNorm-backward epilogue,
// the register window also the filter gradient; both write one partial row per (row chunk, frame). The streaming forms carry
// neither. What launch_dwconv_se reports through DwBnBwd::nblk / wgrad_rows, and what the backward plan query answers.
static DwBwdForm dw_bwd_form(const DwPlan& p, int stride, bool want_wgrad) {
    DwBwdForm f;
    f.form = p.form, f.chunks = (int)p.grid.y, f.rpc = p.rpc;
    const int rows = (int)(p.grid.y * p.grid.z);
    if (stride == 1 && (p.form == DW_LDS || p.form == DW_WINDOW)) f.bn_rows = rows;
    if (stride == 1 && p.form == DW_WINDOW && want_wgrad) f.wgrad_rows = rows;
    return f;
}
DwBwdForm dwconv_se_bwd_form(const LayerGeom& g, bool want_wgrad) {
    return dw_bwd_form(dw_plan(g.B, g.Cin, g.KH, g.stride, g.Ho, g.Wo, false), g.stride, want_wgrad);
}

static int launch_dwconv_se_impl(const float* x, const float* w_khwc, float* y, const float* scale, const float* shift,
                                 float* pool_partial, const LayerGeom& g, int act, hipStream_t s, int stats, const DwInXf& xf,
                                 const DwBnBwd* bnb);

// (per-launch event record for bench.py's roofline.families: algorithmic bytes = input + output + taps, FLOP = 2 K^2 per output)
int launch_dwconv_se(const float* x, const float* w_khwc, float* y, const float* scale, const float* shift,
                     float* pool_partial, const LayerGeom& g, int act, hipStream_t s, int stats, const DwInXf& in, const DwBnBwd* bnb) {
    int rec = -1;
    if (conv_prof_enabled()) {
        const int C = g.Cin, K = g.KH;
        char name[48];
        snprintf(name, sizeof(name), "dwconv<%dx%d/%d>%s", K, K, g.stride, bnb ? ",dgrad" : stats ? ",train" : "");
        const double out = (double)g.B * g.Ho * g.Wo * C;
        rec = prof_start(name, 2.0 * out * K * K, 4.0 * ((double)g.B * g.H * g.W * C + out * (bnb ? 2.0 : 1.0) + (double)K * K * C), s,
                         act == ORBIT_ACT_SILU ? out : 0.0);
    }
    const int rc = launch_dwconv_se_impl(x, w_khwc, y, scale, shift, pool_partial, g, act, s, stats, in, bnb);
    prof_stop(rec, s);
    return rc;
}

static int launch_dwconv_se_impl(const float* x, const float* w_khwc, float* y, const float* scale, const float* shift,
                                 float* pool_partial, const LayerGeom& g, int act, hipStream_t s, int stats, const DwInXf& xf,
                                 const DwBnBwd* bnb) {
    const int B = g.B, H = g.H, W = g.W, C = g.Cin, K = g.KH, stride = g.stride, pad_t = g.pad_t, pad_l = g.pad_l, Ho = g.Ho, Wo = g.Wo;
    const float *in_scale = xf.scale, *in_shift = xf.shift;
    ORBIT_REQUIRE(x && w_khwc && y, "dwconv_se: null pointer");
    if (bnb) {
        ORBIT_REQUIRE(bnb->y && bnb->bn.mean && bnb->bn.invstd && bnb->bn.scale && bnb->bn.shift && bnb->partial && bnb->nblk,
                      "dwconv_se: incomplete BatchNorm-backward epilogue");
        ORBIT_REQUIRE(!stats && !in_scale && !scale && !shift && !pool_partial && stride == 1 && act == ORBIT_ACT_NONE,
                      "dwconv_se: the BatchNorm-backward epilogue belongs to the plain stride-1 data-gradient use");
        *bnb->nblk = 0;
    }
    ORBIT_REQUIRE(!stats || pool_partial, "dwconv_se: statistics requested without a buffer");
    ORBIT_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "dwconv_se: the input transform needs scale and shift");
    ORBIT_REQUIRE(!in_scale || stats, "dwconv_se: the input transform is instantiated for the statistics form only");
    const bool use_xf = in_scale != nullptr;
    ORBIT_REQUIRE(C % 4 == 0, "dwconv_se: C %% 4 != 0 (C=%d)", C);
    ORBIT_REQUIRE((K == 3 || K == 5) && (stride == 1 || stride == 2), "dwconv_se: K=%d stride=%d not instantiated", K,
                  stride);
    const DwPlan p = dw_plan(B, C, K, stride, Ho, Wo, stats != 0);
    const dim3 grid = p.grid;
    const size_t lds = p.lds;
    if (bnb) {
        const DwBwdForm bf = dw_bwd_form(p, stride, bnb->wgrad_partial != nullptr);
        *bnb->nblk = bf.bn_rows;
        if (bnb->wgrad_rows) *bnb->wgrad_rows = bf.wgrad_rows;
    }
    const int cb4 = p.cb4, rpc = p.rpc, cs4 = p.cs4, G = p.G, IWA = p.IWA;
    const DwInXf no_xf{nullptr, nullptr, 0};
    dw_dispatch_ks(K, stride, [&](auto kc, auto sc) {
        constexpr int KK = decltype(kc)::value, SS = decltype(sc)::value;
        switch (p.form) {
        case DW_LDS:
            if (bnb) {
                if constexpr (SS == 1)
                    dwconv_lds_kernel<KK, SS, 8, true, false, true><<<grid, 256, lds, s>>>(
                        x, w_khwc, y, nullptr, nullptr, bnb->partial, H, W, C, pad_t, pad_l, Ho, Wo, act, cs4, rpc, G, IWA, no_xf, *bnb);
            } else if (use_xf)
                dwconv_lds_kernel<KK, SS, 8, true, true><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t,
                                                                               pad_l, Ho, Wo, act, cs4, rpc, G, IWA, xf);
            else if (stats)
                dwconv_lds_kernel<KK, SS, 8, true><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l,
                                                                         Ho, Wo, act, cs4, rpc, G, IWA);
            else if (p.deep)
                dwconv_lds_kernel<KK, SS, 12><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l, Ho,
                                                                    Wo, act, cs4, rpc, G, IWA);
            else
                dwconv_lds_kernel<KK, SS, 8><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l, Ho,
                                                                   Wo, act, cs4, rpc, G, IWA);
            break;
        case DW_WINDOW: {
            constexpr int NO = KK == 3 ? 4 : (SS == 1 ? 2 : 1);  // outputs per thread: what the K x NCOL window leaves registers for
            if (bnb && bnb->wgrad_partial) {
                const size_t lds_wg = (size_t)(K * K * cb4 + 8 * 256) * sizeof(float4);
                if constexpr (SS == 1)
                    dwconv_win_kernel<KK, SS, NO, true, false, true, true><<<grid, 256, lds_wg, s>>>(
                        x, w_khwc, y, nullptr, nullptr, bnb->partial, H, W, C, pad_t, pad_l, Ho, Wo, act, cb4, rpc, no_xf, *bnb);
            } else if (bnb) {
                if constexpr (SS == 1)
                    dwconv_win_kernel<KK, SS, NO, true, false, true><<<grid, 256, lds, s>>>(
                        x, w_khwc, y, nullptr, nullptr, bnb->partial, H, W, C, pad_t, pad_l, Ho, Wo, act, cb4, rpc, no_xf, *bnb);
            } else if (use_xf)
                dwconv_win_kernel<KK, SS, NO, true, true><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t,
                                                                                 pad_l, Ho, Wo, act, cb4, rpc, xf);
            else if (stats)
                dwconv_win_kernel<KK, SS, NO, true><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l,
                                                                           Ho, Wo, act, cb4, rpc);
            else
                dwconv_win_kernel<KK, SS, NO><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l, Ho,
                                                                     Wo, act, cb4, rpc);
            break;
        }
        case DW_PIPE:
            if (use_xf)
                dwconv_pipe_kernel<KK, SS, true, true><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t,
                                                                              pad_l, Ho, Wo, act, cb4, rpc, xf);
            else if (stats)
                dwconv_pipe_kernel<KK, SS, true><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l, Ho,
                                                                        Wo, act, cb4, rpc);
            else
                dwconv_pipe_kernel<KK, SS><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l, Ho, Wo,
                                                                  act, cb4, rpc);
            break;
        case DW_STREAM:
            if (use_xf)
                dwconv_se_kernel<KK, SS, true, true><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l,
                                                                            Ho, Wo, act, cb4, rpc, xf);
            else if (stats)
                dwconv_se_kernel<KK, SS, true><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l, Ho,
                                                                      Wo, act, cb4, rpc);
            else
                dwconv_se_kernel<KK, SS><<<grid, 256, lds, s>>>(x, w_khwc, y, scale, shift, pool_partial, H, W, C, pad_t, pad_l, Ho, Wo, act,
                                                                cb4, rpc);
            break;
        }
    });
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_se_gate2(const float* partial, int chunks, int HW, const float* w1, const float* b1, const float* w2t,
                    const float* b2, float* gate, int B, int C, int R, hipStream_t s, float* pooled_out) {
    ORBIT_REQUIRE(partial && w1 && b1 && w2t && b2 && gate, "se_gate2: null pointer");
    ORBIT_REQUIRE(C % 4 == 0, "se_gate2: C %% 4 != 0 (C=%d)", C);
    // wide blocks for the wide layers: the gate of a frame is a chain of L2 latencies through ONE CU (up to 2 x 221 KB of
    // weights); 1024 threads take all 48 hidden units of the 1152-channel blocks in one round and every channel quad in one
    // pass (19-20 us -> measured below), 256 stay best for the narrow early blocks
    const size_t lds = (size_t)(((C + R + 3) & ~3) + 4 * 1024) * sizeof(float);
    const int rec = prof_start("se_gate", 4.0 * B * C * R, 4.0 * ((double)B * chunks * C + 2.0 * C * R + C + R + (double)B * C), s);
    if (C >= 1024)  // measured per 200 frames: C = 1152: 19-20 -> 14.2-14.8 us; C = 672: 11.0-11.3 -> 11.3-13.1 (worse)
        se_gate2_kernel<1024><<<B, 1024, lds, s>>>(partial, chunks, 1.0f / (float)HW, w1, b1, w2t, b2, gate, C, R, pooled_out);
    else
        se_gate2_kernel<256><<<B, 256, lds, s>>>(partial, chunks, 1.0f / (float)HW, w1, b1, w2t, b2, gate, C, R, pooled_out);
    prof_stop(rec, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_transpose(const float* in, float* out, int rows, int cols, hipStream_t s) {
    transpose_kernel<<<grid_for((size_t)rows * cols), 256, 0, s>>>(in, out, rows, cols);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int dwconv_pack_weights(const float* w, float* w_khwc, int C, int K, hipStream_t s) {
    dw_pack_kernel<<<grid_for((size_t)C * K * K), 256, 0, s>>>(w, w_khwc, C, K);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_maxpool(const float* x, float* y, const LayerGeom& g, hipStream_t s) {
    const int B = g.B, H = g.H, W = g.W, C = g.Cin, K = g.KH, stride = g.stride, pad = g.pad_t, Ho = g.Ho, Wo = g.Wo;
    ORBIT_REQUIRE(x && y, "maxpool: null pointer");
    ORBIT_REQUIRE(C % 4 == 0, "maxpool: C %% 4 != 0 (C=%d)", C);
    const size_t total = (size_t)B * Ho * Wo * (C / 4);
    ORBIT_REQUIRE(total < (1ull << 32), "maxpool: tensor too large for 32-bit index arithmetic");
    const int rec = prof_start("maxpool", 0.0, 4.0 * ((double)B * H * W * C + (double)B * Ho * Wo * C), s);
    maxpool_kernel<<<grid_for(total), 256, 0, s>>>(x, y, B, H, W, C, K, stride, pad, Ho, Wo);
    prof_stop(rec, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_avgpool(const float* x, float* y, int B, int HW, int C, hipStream_t s) {
    ORBIT_REQUIRE(x && y && B > 0 && HW > 0 && C > 0, "avgpool: bad arguments");
    dim3 grid(cdiv(C, 64), B);
    const int rec = prof_start("avgpool", (double)B * HW * C, 4.0 * ((double)B * HW * C + (double)B * C), s);
    avgpool_kernel<<<grid, 256, 0, s>>>(x, y, HW, C);
    prof_stop(rec, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int launch_se_gate(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* gate, int B, int C, int R, hipStream_t s) {
    ORBIT_REQUIRE(pooled && w1 && b1 && w2 && b2 && gate, "se_gate: null pointer");
    se_gate_kernel<<<B, 256, (size_t)(C + R) * sizeof(float), s>>>(pooled, w1, b1, w2, b2, gate, C, R);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

}  // namespace orbit

using namespace orbit;

extern "C" {

int orbit_op_dwconv2d(const float* x, const float* w, float* y, const float* scale, const float* shift, int B,
                      int H, int W, int C, int K, int stride, int pad_top, int pad_left, int Ho, int Wo,
                      int act, orbit_stream_t stream) {
    ORBIT_REQUIRE(x && w && y, "op_dwconv2d: null pointer");
    hipStream_t s = (hipStream_t)stream;
    float* wp = nullptr;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&wp), (size_t)C * K * K * sizeof(float), s));
    int rc = dwconv_pack_weights(w, wp, C, K, s);
    if (rc == ORBIT_OK)
        rc = launch_dwconv_se(x, wp, y, scale, shift, nullptr, LayerGeom{B, H, W, C, C, K, K, stride, pad_top, pad_left, Ho, Wo}, act, s);
    (void)hipFreeAsync(wp, s);
    return rc;
}

/* Training form of the depthwise op (single-operator entry for the parity tests): y = dwconv(act_in(x * in_scale + in_shift))
 * with the input transform applied on load (in_scale / in_shift nullable = none), and the per-channel sums / sums of squares
 * of y, reduced from the kernel's per-(frame, chunk) partials: stats [2][C]. The depthwise kernel variant is chosen by the
 * usual options (dw_window / dw_lds / dw_pipe). */
int orbit_op_dwconv2d_train(const float* x, const float* w, float* y, const float* in_scale, const float* in_shift,
                            int in_act, int B, int H, int W, int C, int K, int stride, int pad_top, int pad_left, int Ho,
                            int Wo, float* stats, orbit_stream_t stream) {
    ORBIT_REQUIRE(x && w && y && stats, "op_dwconv2d_train: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int nblk = B * dwconv_se_chunks(Ho);
    float* tmp = nullptr;
    const size_t wfl = (size_t)C * K * K, pfl = bn_partial_floats((size_t)nblk, C) + 4 * (size_t)C;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&tmp), (((wfl + 63) & ~(size_t)63) + pfl) * sizeof(float), s));
    float* part = tmp + ((wfl + 63) & ~(size_t)63);
    int rc = dwconv_pack_weights(w, tmp, C, K, s);
    if (rc == ORBIT_OK)
        rc = launch_dwconv_se(x, tmp, y, nullptr, nullptr, part, LayerGeom{B, H, W, C, C, K, K, stride, pad_top, pad_left, Ho, Wo},
                              ORBIT_ACT_NONE, s, 1, DwInXf{in_scale, in_shift, in_act});
    // "mean" and "invstd" outputs of the finalize carry the statistics back: mean = sum / M; from invstd the test recovers
    // the variance. Simpler for a test: finalize with M = 1 and eps = 0 is not meaningful - sum the partials directly
    if (rc == ORBIT_OK) rc = launch_sum_partials(part, nblk, C, stats, s);
    (void)hipFreeAsync(tmp, s);
    return rc;
}

/* Inference form of the depthwise op WITH its squeeze-excite pooling epilogue (single-operator entry for the parity tests): the
 * launch the plan makes for an MBConv block's depthwise layer, y = act(dw(x) * scale + shift) and partial[b][chunk][c] = the sum
 * of y over the chunk's output rows; partial is [B][chunks][C] with chunks as orbit_op_dwconv2d_plan reports them. */
int orbit_op_dwconv2d_se(const float* x, const float* w, const float* scale, const float* shift, int act, int B, int H, int W,
                         int C, int K, int stride, int pad_top, int pad_left, int Ho, int Wo, float* y, float* partial,
                         orbit_stream_t stream) {
    ORBIT_REQUIRE(x && w && y && partial, "op_dwconv2d_se: null pointer");
    ORBIT_REQUIRE(B > 0 && C > 0 && Ho > 0 && Wo > 0 && (K == 3 || K == 5), "op_dwconv2d_se: bad geometry");
    hipStream_t s = (hipStream_t)stream;
    float* wp = nullptr;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&wp), (size_t)C * K * K * sizeof(float), s));
    int rc = dwconv_pack_weights(w, wp, C, K, s);
    if (rc == ORBIT_OK)
        rc = launch_dwconv_se(x, wp, y, scale, shift, partial, LayerGeom{B, H, W, C, C, K, K, stride, pad_top, pad_left, Ho, Wo}, act, s,
                              0);
    (void)hipFreeAsync(wp, s);
    return rc;
}

/* Host only: the kernel form launch_dwconv_se runs for this layer under the current options, after the LDS-fit fallback, and
 * the row chunking of its pooling partials. *form: 0 streaming, 1 software-pipelined, 2 register window, 3 LDS patch. */
int orbit_op_dwconv2d_plan(int B, int C, int K, int stride, int Ho, int Wo, int train_form, int* form, int* chunks,
                           int* rows_per_chunk) {
    ORBIT_REQUIRE(form && chunks && rows_per_chunk, "op_dwconv2d_plan: null pointer");
    ORBIT_REQUIRE(B > 0 && C > 0 && C % 4 == 0 && Ho > 0 && Wo > 0 && (K == 3 || K == 5) && (stride == 1 || stride == 2),
                  "op_dwconv2d_plan: bad geometry");
    const DwPlan p = dw_plan(B, C, K, stride, Ho, Wo, train_form != 0);
    *form = (int)p.form, *chunks = (int)p.grid.y, *rows_per_chunk = p.rpc;
    return ORBIT_OK;
}

/* The gate kernel the plans launch (se_gate2_kernel / se_gate_frame), single-operator entry for the parity tests:
 * pooled = (sum over chunks of partial[b][chunk]) / hw, gate = sigmoid(W2 silu(W1 pooled + b1) + b2). w2 in torch layout [C][R]
 * (transposed here as the plan's packing does); pooled_out [B][C] or nullptr. */
int orbit_op_se_gate2(const float* partial, int chunks, int hw, const float* w1, const float* b1, const float* w2,
                      const float* b2, int B, int C, int R, float* gate, float* pooled_out, orbit_stream_t stream) {
    ORBIT_REQUIRE(partial && w1 && b1 && w2 && b2 && gate, "op_se_gate2: null pointer");
    ORBIT_REQUIRE(B > 0 && C > 0 && R > 0 && chunks > 0 && hw > 0, "op_se_gate2: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    float* w2t = nullptr;
    ORBIT_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&w2t), (size_t)C * R * sizeof(float), s));
    int rc = launch_transpose(w2, w2t, C, R, s);
    if (rc == ORBIT_OK) rc = launch_se_gate2(partial, chunks, hw, w1, b1, w2t, b2, gate, B, C, R, s, pooled_out);
    (void)hipFreeAsync(w2t, s);
    return rc;
}

int orbit_op_maxpool2d(const float* x, float* y, int B, int H, int W, int C, int K, int stride, int pad,
                       int Ho, int Wo, orbit_stream_t stream) {
    return launch_maxpool(x, y, LayerGeom{B, H, W, C, C, K, K, stride, pad, pad, Ho, Wo}, (hipStream_t)stream);
}

int orbit_op_avgpool(const float* x, float* y, int B, int HW, int C, orbit_stream_t stream) {
    return launch_avgpool(x, y, B, HW, C, (hipStream_t)stream);
}

int orbit_op_se_gate(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* gate, int B, int C, int R, orbit_stream_t stream) {
    return launch_se_gate(pooled, w1, b1, w2, b2, gate, B, C, R, (hipStream_t)stream);
}

}  // extern "C"
