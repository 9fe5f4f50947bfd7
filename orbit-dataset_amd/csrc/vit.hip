// Vision-transformer feature extractors (timm 0.6.12 `vit_small_patch32_224_in21k`, `vit_base_patch32_224_in21k`,
// `vit_base_patch32_224_clip_laion2b`, built with num_classes=0: reference model/feature_extractors.py:49-63), inference only by
// default; orbit_vit_train_forward / orbit_vit_backward give the gradients of the FiLM vectors (LayerNorm gamma / beta) of the
// frozen network, orbit_vit_backward_params those of every parameter as well (second half of this file).
//
// One forward, fp32 throughout (reference: timm VisionTransformer.forward_features + forward_head with global_pool='token'):
//   tokens[b][0]   = cls_token + pos_embed[0]
//   tokens[b][1+p] = patch_embed(frames)[b][p] + pos_embed[1+p]          32x32 stride-32 conv, p = 0..48 (224x224 frames)
//   (CLIP) tokens  = LayerNorm_pre(tokens)
//   12 x { x += proj(attn(LN1(x)));  x += fc2(GELU_erf(fc1(LN2(x)))) }
//   feature        = LN_final(x)[:, 0]
// Kernels:
//   vit_gemm_kernel      y = x W^T + b (+ erf-GELU | + residual) on v_mfma_f32_32x32x2_f32, 128- or 64-row tiles x 128
//                        columns x 32-deep K steps, operands staged K-major in LDS. The patch embedding is the same kernel
//                        with an implicit-GEMM A loader (rows gathered from the NCHW frames, k = c*1024 + kh*32 + kw, the
//                        OIHW order of the filter) and an epilogue that adds pos_embed and writes token rows 1..49.
//                        Every output element is the same k-ordered fma chain whatever the tile height or M: a frame's
//                        features do not depend on the batch it is in (bit for bit).
//   vit_layernorm_kernel one wave per token row, two-pass (mean, centred variance) in registers; gamma / beta from the
//                        parameter pool or from the per-task FiLM vectors (reference model/film.py:57-66).
//   vit_attention_kernel one workgroup per (frame, head): Q, K, V (50 x 64) in LDS, S = QK^T / 8, row softmax, O = PV.
//   vit_gemm_bf16_kernel the opt-in inference form of the four token GEMMs (orbit_vit_enable_bf16): bf16 operands, fp32
//                        accumulation on v_mfma_f32_32x32x16_bf16, weights from bf16 copies made by vit_pack_bf16_kernel;
//                        everything else of such a plan's forward is the fp32 kernels of this list.
// The patch-16 models of the same families (vit_s_16, vit_b_16, vit_b_16_clip: 14 x 14 patches, 197 tokens, six names in all)
// run the same forward with the geometry read from the plan: the patch GEMM's EPI_PATCH16 form (k = c*256 + kh*16 + kw, token
// rows 1..196) and vit_attention197_kernel (fp32 MFMA, K and V resident in LDS). Their plans are inference + FiLM only until
// orbit_vit_enable_backward switches on the taped forward and the FiLM gradients of the frozen network (the same reverse pass
// at 197 tokens, with vit_attention197_bwd_kernel). orbit_vit_enable_weight_backward opens orbit_vit_backward_params for such a
// plan as well: the patch filter gradient is the WX_PATCH16 form of vit_wgrad_kernel (16-float patch rows, M = 196 B, K = 768),
// vit_token_bwd_kernel sums dpos over 197 token rows, and every Linear weight gradient runs at M = 197 B.
// Other frame sizes (orbit_vit_create_sized: square, a multiple of the patch, 32..512; inference + FiLM only): the same forward
// with the position table resampled to the plan's grid once per parameter upload (vit_pos_resample_kernel, torch's bicubic), the
// patch GEMM's EPI_PATCH_RT / EPI_PATCH16_RT forms (frame side and patches per side from the arguments) and, at every token
// count but 50 and 197, vit_attention_n_kernel (the 197-token scheme with K and V streamed through LDS under a running softmax).
// A 224 plan launches what it launched before.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "bf3.h"
#include "common.h"
#include "device_util.h"
#include "param_pool.h"

using namespace orbit;

namespace {

constexpr int VIT_PATCH = 32;
constexpr int VIT_SIZE = 224;
constexpr int VIT_GRID = VIT_SIZE / VIT_PATCH;    // 7
constexpr int VIT_P = VIT_GRID * VIT_GRID;        // 49 patches
constexpr int VIT_N = VIT_P + 1;                  // 50 tokens
constexpr int VIT_KPATCH = 3 * VIT_PATCH * VIT_PATCH;  // 3072
constexpr int VIT_HD = 64;                        // head dim
constexpr int VIT_DEPTH = 12;
constexpr int VIT_MAX_B = 8192;
// the patch-16 models (196 patches + the class token): B * 197 * 4 D stays below 2^31 up to this many frames at D = 768
constexpr int VIT16_PATCH = 16;
constexpr int VIT16_GRID = VIT_SIZE / VIT16_PATCH;     // 14
constexpr int VIT16_P = VIT16_GRID * VIT16_GRID;       // 196 patches
constexpr int VIT16_N = VIT16_P + 1;                   // 197 tokens
constexpr int VIT16_KPATCH = 3 * VIT16_PATCH * VIT16_PATCH;  // 768
constexpr int VIT16_MAX_B = 2048;

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

// ---- token GEMM ------------------------------------------------------------------------------------------------------
constexpr int G_BN = 128, G_BK = 32, G_THREADS = 256;
// EPI_GELU_TAPE: EPI_GELU that also stores the pre-activation (aux); EPI_DGELU: times GELU'(u), u read through `residual`
// EPI_PATCH16: EPI_PATCH for 16 x 16 patches (its own A gather and token-row geometry)
// EPI_PATCH_RT / EPI_PATCH16_RT: the two patch forms with the frame side and the patches per side read from the arguments (the
// plans of orbit_vit_create_sized at other frame sizes than 224); the patch size, and with it the k order, stays a constant
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESIDUAL = 2, EPI_PATCH = 3, EPI_GELU_TAPE = 4, EPI_DGELU = 5, EPI_PATCH16 = 6,
       EPI_PATCH_RT = 7, EPI_PATCH16_RT = 8 };

struct GemmArgs {
    const float* x;         // [M][K] token rows, or the NCHW frames (EPI_PATCH)
    const float* w;         // [N][K] (torch Linear / OIHW conv layout)
    const float* bias;      // [N] or nullptr
    const float* residual;  // [M][N] (EPI_RESIDUAL; may alias y)
    const float* pos;       // pos_embed [50][N] (EPI_PATCH) / [197][N] (EPI_PATCH16)
    float* y;
    int M, N, K;
    float* aux = nullptr;   // [M][N] pre-activation out (EPI_GELU_TAPE)
    int side = 0, grid = 0; // frame side and patches per side (EPI_PATCH_RT / EPI_PATCH16_RT only; pos is then [grid^2 + 1][N])
};

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
// d/du of u Phi(u) = Phi(u) + u phi(u); Phi through erfc, which keeps its relative accuracy in the negative tail
__device__ __forceinline__ float gelu_erf_grad(float u) {
    return 0.5f * erfcf(-u * 0.70710678118654752f) + u * 0.39894228040143268f * expf(-0.5f * u * u);
}

// implicit-GEMM row gather of the patch embedding: element k = c*1024 + kh*32 + kw of patch m % 49 of frame m / 49 (NCHW frames)
__device__ __forceinline__ const float* patch_row_ptr(const float* frames, int m, int k) {
    const int b = m / VIT_P, p = m - b * VIT_P;
    const int ph = p / VIT_GRID, pw = p - ph * VIT_GRID;
    const int c = k >> 10, kh = (k >> 5) & 31, kw = k & 31;
    return frames + (((size_t)b * 3 + c) * VIT_SIZE + ph * VIT_PATCH + kh) * VIT_SIZE + pw * VIT_PATCH + kw;
}

// the same for 16 x 16 patches: k = c*256 + kh*16 + kw of patch m % 196 of frame m / 196. A patch row is 16 floats, so the 8
// four-float chunks of a 32-deep K step lie in two frame rows: chunks 0..3 in row kh, chunks 4..7 in row kh + 1
__device__ __forceinline__ const float* patch16_row_ptr(const float* frames, int m, int k) {
    const int b = m / VIT16_P, p = m - b * VIT16_P;
    const int ph = p / VIT16_GRID, pw = p - ph * VIT16_GRID;
    const int c = k >> 8, kh = (k >> 4) & 15, kw = k & 15;
    return frames + (((size_t)b * 3 + c) * VIT_SIZE + ph * VIT16_PATCH + kh) * VIT_SIZE + pw * VIT16_PATCH + kw;
}

// the two gathers on square frames of any side (a multiple of the patch): LG = log2(patch), k = c*patch^2 + kh*patch + kw
template <int LG>
__device__ __forceinline__ const float* patch_rt_row_ptr(const float* frames, int m, int k, int side, int grid) {
    const int np = grid * grid;
    const int b = m / np, p = m - b * np;
    const int ph = p / grid, pw = p - ph * grid;
    const int c = k >> (2 * LG), kh = (k >> LG) & ((1 << LG) - 1), kw = k & ((1 << LG) - 1);
    return frames + (((size_t)b * 3 + c) * side + (ph << LG) + kh) * side + (pw << LG) + kw;
}

// address of the 4 consecutive k of A row m (clamped into [0, M)) starting at k
template <int EPI>
__device__ __forceinline__ const float* a_row_ptr(const GemmArgs& a, int m, int k) {
    if (EPI == EPI_PATCH) return patch_row_ptr(a.x, m, k);
    if (EPI == EPI_PATCH16) return patch16_row_ptr(a.x, m, k);
    if (EPI == EPI_PATCH_RT) return patch_rt_row_ptr<5>(a.x, m, k, a.side, a.grid);
    if (EPI == EPI_PATCH16_RT) return patch_rt_row_ptr<4>(a.x, m, k, a.side, a.grid);
    return a.x + (size_t)m * a.K + k;
}

// BLOCKED (the data-gradient GEMMs): the k-ordered chain is cut every 256 k into a second accumulator set, so the rounding error
// grows with sqrt(256) + K / 256 instead of sqrt(K) - the accuracy of a cache-blocked CPU sgemm, which the gradient tests take
// as their yardstick. The forward keeps the single chain (its bit-for-bit promises are pinned to it).
template <int BM, int EPI, bool BLOCKED = false>
__global__ __launch_bounds__(G_THREADS) void vit_gemm_kernel(GemmArgs a) {
    constexpr int TI = BM / 64;          // 32-row MFMA tiles per wave (waves are 2 x 2 over the block tile)
    constexpr int AR = BM / 32;          // float4 loads of A per thread per K step
    constexpr int BR = G_BN / 32;        // ... of B
    constexpr int LDA = BM + 4, LDB = G_BN + 4;
    __shared__ float As[G_BK * LDA];
    __shared__ float Bs[G_BK * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * G_BN, m0 = blockIdx.y * BM;
    const int lc = tid & 7, lr = tid >> 3;  // loader: k chunk (4 floats) and row

    const float* ap[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        int m = m0 + lr + 32 * i;
        m = m < a.M ? m : a.M - 1;  // rows past the tail re-read the last row; their outputs are never stored
        ap[i] = a_row_ptr<EPI>(a, m, 4 * lc);
    }
    const float* bp[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) bp[i] = a.w + (size_t)(n0 + lr + 32 * i) * a.K + 4 * lc;

    floatx16 acc[TI][2];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    floatx16 tot[BLOCKED ? TI : 1][2];
    if (BLOCKED) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
    }

    float4 ra[AR], rb[BR];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            // patch rows: k0 advances (c, kh) - one frame row of 32 pixels per K step
            // (16 x 16 patches: (c, kh) with kh even - two frame rows of 16 pixels per K step, the loader's chunk picks the row)
            const float* p = EPI == EPI_PATCH ? ap[i] + ((k0 >> 10) * VIT_SIZE + ((k0 >> 5) & 31)) * VIT_SIZE
                             : EPI == EPI_PATCH16 ? ap[i] + ((k0 >> 8) * VIT_SIZE + ((k0 >> 4) & 15)) * VIT_SIZE
                             : EPI == EPI_PATCH_RT ? ap[i] + (size_t)((k0 >> 10) * a.side + ((k0 >> 5) & 31)) * a.side
                             : EPI == EPI_PATCH16_RT ? ap[i] + (size_t)((k0 >> 8) * a.side + ((k0 >> 4) & 15)) * a.side
                                                     : ap[i] + k0;
            ra[i] = *reinterpret_cast<const float4*>(p);
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) rb[i] = *reinterpret_cast<const float4*>(bp[i] + k0);
    };

    const int nk = a.K / G_BK;
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int r = lr + 32 * i;
            As[(4 * lc + 0) * LDA + r] = ra[i].x;
            As[(4 * lc + 1) * LDA + r] = ra[i].y;
            As[(4 * lc + 2) * LDA + r] = ra[i].z;
            As[(4 * lc + 3) * LDA + r] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            const int r = lr + 32 * i;
            Bs[(4 * lc + 0) * LDB + r] = rb[i].x;
            Bs[(4 * lc + 1) * LDB + r] = rb[i].y;
            Bs[(4 * lc + 2) * LDB + r] = rb[i].z;
            Bs[(4 * lc + 3) * LDB + r] = rb[i].w;
        }
        __syncthreads();
        if (kt + 1 < nk) load((kt + 1) * G_BK);  // next K step in flight during the MFMAs
        const int kh = lane >> 5, col = lane & 31;
#pragma unroll
        for (int kk = 0; kk < G_BK / 2; ++kk) {
            float af[TI], bf[2];
#pragma unroll
            for (int i = 0; i < TI; ++i) af[i] = As[(2 * kk + kh) * LDA + wm * (BM / 2) + 32 * i + col];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Bs[(2 * kk + kh) * LDB + wn * 64 + 32 * j + col];
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (BLOCKED && ((kt & 7) == 7 || kt + 1 == nk)) {
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tot[i][j][r] += acc[i][j][r], acc[i][j][r] = 0.f;
        }
    }

    // epilogue: C[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + 32 * j + (lane & 31);
            const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * (BM / 2) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row >= a.M) continue;
                float v = (BLOCKED ? tot[i][j][r] : acc[i][j][r]) + bv;
                if (EPI == EPI_PATCH_RT || EPI == EPI_PATCH16_RT) {
                    const int np = a.grid * a.grid;  // patches per frame; token rows: np + 1
                    const int b = row / np, p = row - b * np;
                    v += a.pos[(size_t)(1 + p) * a.N + col];
                    a.y[((size_t)b * (np + 1) + 1 + p) * a.N + col] = v;
                    continue;
                }
                if (EPI == EPI_PATCH || EPI == EPI_PATCH16) {
                    constexpr int NP = EPI == EPI_PATCH16 ? VIT16_P : VIT_P;  // patches per frame; token rows: NP + 1
                    const int b = row / NP, p = row - b * NP;
                    v += a.pos[(size_t)(1 + p) * a.N + col];
                    a.y[((size_t)b * (NP + 1) + 1 + p) * a.N + col] = v;
                    continue;
                }
                if (EPI == EPI_GELU_TAPE) a.aux[(size_t)row * a.N + col] = v;
                if (EPI == EPI_GELU || EPI == EPI_GELU_TAPE) v = gelu_erf(v);
                if (EPI == EPI_DGELU) v *= gelu_erf_grad(a.residual[(size_t)row * a.N + col]);
                if (EPI == EPI_RESIDUAL) v += a.residual[(size_t)row * a.N + col];
                a.y[(size_t)row * a.N + col] = v;
            }
        }
}

// tile_rows: 0 = the rule below, 64 / 128 = that instantiation (the single-operator entry points; the forward passes 0)
int check_tile_rows(int tile_rows) {
    ORBIT_REQUIRE(tile_rows == 0 || tile_rows == 64 || tile_rows == 128, "vit gemm: tile_rows must be 0, 64 or 128, got %d", tile_rows);
    return ORBIT_OK;
}
template <int EPI, bool BLOCKED = false>
int launch_gemm(const GemmArgs& a, const char* what, hipStream_t s, int tile_rows = 0) {
    if (a.N % G_BN || a.K % G_BK || a.M <= 0) return set_err(ORBIT_ERR_ARG, "vit gemm: unsupported shape M=%d N=%d K=%d", a.M, a.N, a.K);
    if (int rc = check_tile_rows(tile_rows)) return rc;
    // tile height: 128 rows unless that leaves fewer than two tiles per CU (the D x D and 4D x D layers at ~10k rows)
    const int n_tiles = a.N / G_BN;
    const bool tall = tile_rows ? tile_rows == 128 : (long)cdiv(a.M, 128) * n_tiles >= 512;
    const double flops = 2.0 * a.M * a.N * a.K;
    const double bytes = 4.0 * ((double)a.M * a.K + (double)a.N * a.K + (double)a.M * a.N * (EPI == EPI_RESIDUAL || EPI == EPI_GELU_TAPE || EPI == EPI_DGELU ? 2 : 1));
    char name[48];
    snprintf(name, sizeof(name), "vit_%s<%d>", what, tall ? 128 : 64);
    const int pi = prof_start(name, flops, bytes, s);
    if (tall)
        vit_gemm_kernel<128, EPI, BLOCKED><<<dim3(n_tiles, cdiv(a.M, 128)), G_THREADS, 0, s>>>(a);
    else
        vit_gemm_kernel<64, EPI, BLOCKED><<<dim3(n_tiles, cdiv(a.M, 64)), G_THREADS, 0, s>>>(a);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// ---- bf16 token GEMM (opt-in: orbit_vit_enable_bf16) -----------------------------------------------------------------
// y = x W^T + b (+ erf-GELU | + residual) on v_mfma_f32_32x32x16_bf16: the outer shape of vit_gemm_kernel (BM x 128 block tile,
// 256 threads, 2 x 2 waves, the same tail rule and epilogues), 64-deep K steps. x is the fp32 token rows, rounded to bf16 (RNE,
// v_cvt_pk_bf16_f32) on the way into LDS; w is a bf16 copy of the weight [N][K] (vit_pack_bf16_kernel). LDS rows are
// K-contiguous, 64 bf16 + 16 bytes of padding (GB_ROWB = 144 bytes: 9 r mod 16 is a bijection, so the sixteen rows of a
// ds_read_b128 lane group fall on sixteen different 16-byte slots), and a lane's fragment is one 16-byte read:
// lane l holds row l & 31, k = 16 ks + 8 (l >> 5) + j.
// Numerics: every operand is rounded to bf16 once (RNE); products of two bf16 are exact in the matrix unit. Each 64-deep K step
// is summed by four chained MFMAs that start from ZERO, and that partial sum is added to the running fp32 sum with one RNE add
// per step, in ascending k (the unit aligns its addends to the largest exponent and drops low bits without rounding - fed the
// running sum as C it would lose up to an ulp of the SUM per instruction, always toward zero; see the conv_bf3 row of DESIGN.md
// §5). The epilogue is fp32. Deterministic; a row's bits depend neither on M nor on the tile height (every row sees the same
// steps in the same order). Nothing is promised about subnormal inputs.
constexpr int GB_BK = 64, GB_ROWB = 2 * GB_BK + 16;

struct GemmBf16Args {
    const float* x;           // [M][K] fp32 token rows
    const unsigned short* w;  // [N][K] bf16
    const float* bias;        // [N] or nullptr
    const float* residual;    // [M][N] (EPI_RESIDUAL; may alias y)
    float* y;
    int M, N, K;
};

template <int BM, int EPI>
__global__ __launch_bounds__(G_THREADS) void vit_gemm_bf16_kernel(GemmBf16Args a) {
    constexpr int TI = BM / 64;   // 32-row MFMA tiles per wave (waves are 2 x 2 over the block tile)
    constexpr int AR = BM / 32;   // 32-byte loads of A per thread per K step (8 fp32 -> 8 bf16)
    constexpr int BR = G_BN / 32; // 16-byte loads of B
    constexpr int KS = GB_BK / 16;
    __shared__ __attribute__((aligned(16))) char smem[(BM + G_BN) * GB_ROWB];
    char* As = smem;
    char* Bs = smem + BM * GB_ROWB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * G_BN, m0 = blockIdx.y * BM;
    const int lc = tid & 7, lr = tid >> 3;  // loader: k chunk (8 elements) and row

    const float* ap[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        int m = m0 + lr + 32 * i;
        m = m < a.M ? m : a.M - 1;  // rows past the tail re-read the last row; their outputs are never stored
        ap[i] = a.x + (size_t)m * a.K + 8 * lc;
    }
    const unsigned short* bp[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) bp[i] = a.w + (size_t)(n0 + lr + 32 * i) * a.K + 8 * lc;

    floatx16 acc[TI][2];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    floatx4 ra0[AR], ra1[AR];
    uintx4 rb[BR];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            ra0[i] = *reinterpret_cast<const floatx4*>(ap[i] + k0);
            ra1[i] = *reinterpret_cast<const floatx4*>(ap[i] + k0 + 4);
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) rb[i] = *reinterpret_cast<const uintx4*>(bp[i] + k0);
    };

    // fragment addresses: row l & 31 of the wave's tiles, 16 bytes at k = 8 (l >> 5) of each 16-deep k-step
    const int fr = lane & 31, fh = lane >> 5;
    const char* afp = As + (wm * (BM / 2) + fr) * GB_ROWB + 16 * fh;
    const char* bfp = Bs + (wn * 64 + fr) * GB_ROWB + 16 * fh;

    const int nk = a.K / GB_BK;
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const uintx4 p = {pk_bf16(ra0[i][0], ra0[i][1]), pk_bf16(ra0[i][2], ra0[i][3]), pk_bf16(ra1[i][0], ra1[i][1]),
                              pk_bf16(ra1[i][2], ra1[i][3])};
            *reinterpret_cast<uintx4*>(As + (lr + 32 * i) * GB_ROWB + 16 * lc) = p;
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) *reinterpret_cast<uintx4*>(Bs + (lr + 32 * i) * GB_ROWB + 16 * lc) = rb[i];
        __syncthreads();
        if (kt + 1 < nk) load((kt + 1) * GB_BK);  // next K step in flight during the MFMAs
        // EVERY fragment of the K step is in registers before its first MFMA, and none is written again before the step's last
        // MFMA result has been read (the adds below): an issued bf16 MFMA that waits behind another stream's matrix work has been
        // seen to pick up operands that a later LDS return overwrote (csrc/conv_bf3.hip, compute_tile)
        bf16x8 af[KS][TI], bf[KS][2];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int i = 0; i < TI; ++i) af[ks][i] = *reinterpret_cast<const bf16x8*>(afp + 32 * i * GB_ROWB + 32 * ks);
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[ks][j] = *reinterpret_cast<const bf16x8*>(bfp + 32 * j * GB_ROWB + 32 * ks);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                floatx16 t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks][i], bf[ks][j], t, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += t[r];
            }
        __builtin_amdgcn_sched_barrier(0);
    }

    // epilogue: C[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) - the map of the fp32 32x32x2 form
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + 32 * j + (lane & 31);
            const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * (BM / 2) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row >= a.M) continue;
                float v = acc[i][j][r] + bv;
                if (EPI == EPI_GELU) v = gelu_erf(v);
                if (EPI == EPI_RESIDUAL) v += a.residual[(size_t)row * a.N + col];
                a.y[(size_t)row * a.N + col] = v;
            }
        }
}

// the tile rule and the tile_rows override of launch_gemm; profiler rows vit_<what>_bf16<64|128>
template <int EPI>
int launch_gemm_bf16(const GemmBf16Args& a, const char* what, hipStream_t s, int tile_rows = 0) {
    if (a.N % G_BN || a.K % GB_BK || a.M <= 0)
        return set_err(ORBIT_ERR_ARG, "vit bf16 gemm: unsupported shape M=%d N=%d K=%d (N %% %d and K %% %d must be 0)", a.M, a.N, a.K,
                       G_BN, GB_BK);
    if (int rc = check_tile_rows(tile_rows)) return rc;
    const int n_tiles = a.N / G_BN;
    const bool tall = tile_rows ? tile_rows == 128 : (long)cdiv(a.M, 128) * n_tiles >= 512;
    const double flops = 2.0 * a.M * a.N * a.K;
    const double bytes = 4.0 * a.M * a.K + 2.0 * a.N * a.K + 4.0 * a.M * a.N * (EPI == EPI_RESIDUAL ? 2 : 1);
    char name[56];
    snprintf(name, sizeof(name), "vit_%s_bf16<%d>", what, tall ? 128 : 64);
    const int pi = prof_start(name, flops, bytes, s);
    if (tall)
        vit_gemm_bf16_kernel<128, EPI><<<dim3(n_tiles, cdiv(a.M, 128)), G_THREADS, 0, s>>>(a);
    else
        vit_gemm_bf16_kernel<64, EPI><<<dim3(n_tiles, cdiv(a.M, 64)), G_THREADS, 0, s>>>(a);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// fp32 -> bf16 (RNE), 8 elements per thread; the tail and unaligned buffers go element by element
__global__ __launch_bounds__(256) void vit_pack_bf16_kernel(const float* __restrict__ w, unsigned short* __restrict__ out,
                                                            size_t numel, int vec_ok) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= numel) return;
    if (vec_ok && i + 8 <= numel) {
        const float4 lo = *reinterpret_cast<const float4*>(w + i), hi = *reinterpret_cast<const float4*>(w + i + 4);
        const uint4 p = {pk_bf16(lo.x, lo.y), pk_bf16(lo.z, lo.w), pk_bf16(hi.x, hi.y), pk_bf16(hi.z, hi.w)};
        *reinterpret_cast<uint4*>(out + i) = p;
        return;
    }
    for (size_t j = i; j < numel && j < i + 8; ++j) out[j] = (unsigned short)(pk_bf16(w[j], 0.f) & 0xffffu);
}

int launch_pack_bf16(const float* w, unsigned short* out, size_t numel, hipStream_t s) {
    const int vec_ok = (((uintptr_t)w | (uintptr_t)out) & 15) == 0;
    const size_t blocks = (numel + 2047) / 2048;  // 256 threads x 8 elements
    const int pi = prof_start("vit_pack_bf16", 0.0, 6.0 * numel, s);
    vit_pack_bf16_kernel<<<(unsigned)blocks, 256, 0, s>>>(w, out, numel, vec_ok);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// ---- class token row -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vit_cls_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                                      float* __restrict__ tokens, int B, int D, int N) {
    const size_t n = (size_t)B * D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int b = (int)(i / D), d = (int)(i - (size_t)b * D);
        tokens[(size_t)b * N * D + d] = cls[d] + pos[d];
    }
}

// N: token rows per frame (row 0 of each frame is written)
int launch_cls_token(const float* cls, const float* pos, float* tokens, int B, int D, int N, hipStream_t s) {
    const int pi = prof_start("vit_cls_token", 0.0, 4.0 * B * D, s);
    vit_cls_kernel<<<cdiv(B * D, 256) < 1024 ? cdiv(B * D, 256) : 1024, 256, 0, s>>>(cls, pos, tokens, B, D, N);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// ---- position table at another grid -----------------------------------------------------------------------------------
// pos [1 + g*g][D] -> out [1 + G*G][D]: row 0 copied, rows 1.. the g x g table resampled to G x G as torch's
// F.interpolate(mode="bicubic", align_corners=False) does it (aten UpSampleBicubic2d): source coordinate (i + 0.5) * (g / G) - 0.5
// with the ratio rounded to fp32 first, cubic convolution with A = -0.75 on t = coordinate - floor, four taps per axis clamped to
// [0, g - 1], the four rows interpolated along x and then those four along y. One thread per output element, fp32.
__device__ __forceinline__ void bicubic_coeffs(float t, float (&c)[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x3 = (1.f - t) + 1.f, x2 = 1.f - t;
    c[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    c[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    c[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    c[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

__global__ __launch_bounds__(256) void vit_pos_resample_kernel(const float* __restrict__ pos, float* __restrict__ out, int g, int G,
                                                               int D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (G * G + 1) * D) return;
    const int row = i / D, d = i - row * D;
    if (row == 0) {
        out[i] = pos[i];
        return;
    }
    const int oy = (row - 1) / G, ox = (row - 1) - oy * G;
    const float ratio = (float)g / (float)G;
    const float fy = ratio * (oy + 0.5f) - 0.5f, fx = ratio * (ox + 0.5f) - 0.5f;
    const float iyf = floorf(fy), ixf = floorf(fx);
    const int iy = (int)iyf, ix = (int)ixf;
    float cy[4], cx[4];
    bicubic_coeffs(fy - iyf, cy);
    bicubic_coeffs(fx - ixf, cx);
    float v = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int y = min(max(iy - 1 + a, 0), g - 1);
        float r = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int x = min(max(ix - 1 + b, 0), g - 1);
            r += pos[(size_t)(1 + y * g + x) * D + d] * cx[b];
        }
        v += r * cy[a];
    }
    out[i] = v;
}

int launch_pos_resample(const float* pos, float* out, int g, int G, int D, hipStream_t s) {
    const int n = (G * G + 1) * D;
    const int pi = prof_start("vit_pos_resample", 40.0 * n, 4.0 * (n + (g * g + 1) * D), s);
    vit_pos_resample_kernel<<<cdiv(n, 256), 256, 0, s>>>(pos, out, g, G, D);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// ---- LayerNorm -------------------------------------------------------------------------------------------------------
template <int NPL>  // D / 64 values per lane
__global__ __launch_bounds__(256) void vit_layernorm_kernel(const float* x, size_t x_stride, float* y, size_t y_stride,
                                                            int rows, const float* __restrict__ g,
                                                            const float* __restrict__ b, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    constexpr int D = NPL * 64;
    const float* xr = x + (size_t)row * x_stride;
    float v[NPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) v[i] = xr[lane + 64 * i], s += v[i];
    // a division, not * (1.f / D): the compiler contracts that product into the subtraction below (fma(-sum, 1/D, v)), which
    // subtracts the UNROUNDED sum * fl(1/D) - for a constant row c that leaves v = -c * 2^-25 instead of 0, and at variance 0 the
    // 1/sqrt(eps) = 1000 behind it turns that into 1e-4 * gamma (tests/test_gpu_vit_ops.py, constant rows must give beta)
    const float mean = wave_sum_xor(s) / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) v[i] -= mean, q += v[i] * v[i];
    const float rstd = 1.f / sqrtf(wave_sum_xor(q) * (1.f / D) + eps);
    float* yr = y + (size_t)row * y_stride;  // (may alias x: every lane has read its values)
#pragma unroll
    for (int i = 0; i < NPL; ++i) yr[lane + 64 * i] = v[i] * rstd * g[lane + 64 * i] + b[lane + 64 * i];
}

int launch_layernorm(const float* x, size_t xs, float* y, size_t ys, int rows, int D, const float* g, const float* b,
                     float eps, hipStream_t s) {
    const int pi = prof_start("vit_layernorm", 8.0 * rows * D, 4.0 * 2 * rows * D, s);
    const dim3 grid(cdiv(rows, 4));
    if (D == 384)
        vit_layernorm_kernel<6><<<grid, 256, 0, s>>>(x, xs, y, ys, rows, g, b, eps);
    else if (D == 768)
        vit_layernorm_kernel<12><<<grid, 256, 0, s>>>(x, xs, y, ys, rows, g, b, eps);
    else
        return set_err(ORBIT_ERR_ARG, "vit layernorm: unsupported width %d", D);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// ---- attention -------------------------------------------------------------------------------------------------------
// qkv [B*50][3D] (timm: qkv.reshape(B, N, 3, heads, 64)) -> out [B*50][D], columns h*64..h*64+63
__global__ __launch_bounds__(256) void vit_attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int D,
                                                            int heads) {
    constexpr int LDK = VIT_HD + 1, LDS_ = 52;
    __shared__ float q[VIT_N * VIT_HD], k[VIT_N * LDK], v[VIT_N * VIT_HD], sc[VIT_N * LDS_];
    const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x;
    const float* base = qkv + (size_t)b * VIT_N * 3 * D + h * VIT_HD;
    for (int i = tid; i < VIT_N * VIT_HD; i += 256) {
        const int t = i >> 6, d = i & 63;
        const float* r = base + (size_t)t * 3 * D + d;
        q[i] = r[0];
        k[t * LDK + d] = r[D];
        v[i] = r[2 * D];
    }
    __syncthreads();
    for (int i = tid; i < VIT_N * VIT_N; i += 256) {
        const int r = i / VIT_N, c = i - r * VIT_N;
        float acc = 0.f;
#pragma unroll 16
        for (int d = 0; d < VIT_HD; ++d) acc = fmaf(q[r * VIT_HD + d], k[c * LDK + d], acc);
        sc[r * LDS_ + c] = acc * 0.125f;  // head_dim ** -0.5
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < VIT_N; r += 4) {
        const float val = lane < VIT_N ? sc[r * LDS_ + lane] : -INFINITY;
        const float m = wave_max_xor(val);
        const float e = lane < VIT_N ? expf(val - m) : 0.f;
        const float sum = wave_sum_xor(e);
        if (lane < VIT_N) sc[r * LDS_ + lane] = e / sum;
    }
    __syncthreads();
    for (int i = tid; i < VIT_N * VIT_HD; i += 256) {
        const int r = i >> 6, d = i & 63;
        float acc = 0.f;
#pragma unroll 10
        for (int c = 0; c < VIT_N; ++c) acc = fmaf(sc[r * LDS_ + c], v[c * VIT_HD + d], acc);
        out[((size_t)b * VIT_N + r) * D + h * VIT_HD + d] = acc;
    }
}

// The same for the 197 tokens of the patch-16 models, on v_mfma_f32_32x32x2_f32. One workgroup of 7 waves per (frame, head):
// K [224][65] and V [224][72] (rows 197..223 zero) resident in 122 752 bytes of LDS, each wave owns 32 queries. A wave computes
// the TRANSPOSED scores S^T = K (Q/8)^T - A operand K out of LDS, B operand its queries out of registers - so that the MFMA's
// C layout leaves every lane with one query's column: 7 tiles x 16 registers = 112 keys in the lane, the other 112 in lane ^ 32.
// The softmax is then a reduction inside the lane plus one exchange, and P^T is already the B operand of O^T = V^T P^T (A operand
// V out of LDS): P never goes through LDS. Keys 197..223 are set to -inf before the maximum; queries past 196 re-read query 196
// and are never stored. k order inside a score: step kk adds d = kk and d = 32 + kk; inside an output: the keys of a lane half in
// (tile, register) order - fixed, and independent of the other workgroups of the launch.
constexpr int A16_WAVES = 7;
constexpr int A16_NPAD = 32 * A16_WAVES;  // 224
constexpr int A16_LDK = VIT_HD + 1;       // odd row stride: the 32 keys of an A fragment hit 32 banks, the two d halves the other 32
constexpr int A16_LDV = VIT_HD + 8;       // rows 4 apart (the two lane halves of a PV step) land 32 banks apart; float4 rows
constexpr size_t A16_LDS_BYTES = (size_t)A16_NPAD * (A16_LDK + A16_LDV) * sizeof(float);
static_assert(A16_NPAD >= VIT16_N && A16_NPAD - VIT16_N < 32, "the last key tile must hold a valid key");
static_assert((A16_NPAD * A16_LDK) % 4 == 0 && A16_LDV % 4 == 0, "V rows are written as float4");

__global__ __launch_bounds__(64 * A16_WAVES) void vit_attention197_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                          int D, int heads) {
    extern __shared__ __attribute__((aligned(16))) float a16_sm[];
    float* ks = a16_sm;
    float* vs = a16_sm + A16_NPAD * A16_LDK;
    const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const float* base = qkv + (size_t)b * VIT16_N * 3 * D + h * VIT_HD;
    for (int i = tid; i < A16_NPAD * (VIT_HD / 4); i += 64 * A16_WAVES) {
        const int t = i >> 4, c = (i & 15) * 4;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (t < VIT16_N) {
            const float* r = base + (size_t)t * 3 * D + c;
            kv = *reinterpret_cast<const float4*>(r + D);
            vv = *reinterpret_cast<const float4*>(r + 2 * D);
        }
        float* kd = ks + t * A16_LDK + c;
        kd[0] = kv.x, kd[1] = kv.y, kd[2] = kv.z, kd[3] = kv.w;
        *reinterpret_cast<float4*>(vs + t * A16_LDV + c) = vv;
    }
    // this lane's query, d = 32 half .. 32 half + 31, times head_dim ** -0.5 (a power of two: exact)
    const int query = 32 * wave + col;
    float qf[32];
    {
        const float* qp = base + (size_t)(query < VIT16_N ? query : VIT16_N - 1) * 3 * D + 32 * half;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 q4 = *reinterpret_cast<const float4*>(qp + 4 * i);
            qf[4 * i + 0] = q4.x * 0.125f, qf[4 * i + 1] = q4.y * 0.125f, qf[4 * i + 2] = q4.z * 0.125f, qf[4 * i + 3] = q4.w * 0.125f;
        }
    }
    __syncthreads();

    // S^T tile t: rows = keys 32 t + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's query
    floatx16 sc[A16_WAVES];
#pragma unroll
    for (int t = 0; t < A16_WAVES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[t][r] = 0.f;
    const float* ka = ks + col * A16_LDK + 32 * half;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk)
#pragma unroll
        for (int t = 0; t < A16_WAVES; ++t)
            sc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[32 * t * A16_LDK + kk], qf[kk], sc[t], 0, 0, 0);

    // softmax over the keys of this lane's query: the padded keys leave the maximum and the sum
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < A16_WAVES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (t == A16_WAVES - 1 && 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half >= VIT16_N) sc[t][r] = -INFINITY;
            m = fmaxf(m, sc[t][r]);
        }
    m = fmaxf(m, __shfl_xor(m, 32));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < A16_WAVES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[t][r] = expf(sc[t][r] - m), sum += sc[t][r];
    sum += __shfl_xor(sum, 32);

    // O^T tile dt: rows = d 32 dt + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's query
    floatx16 ov[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) ov[dt][r] = 0.f;
    const float* va = vs + 4 * half * A16_LDV + col;
#pragma unroll
    for (int t = 0; t < A16_WAVES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (32 * t + 8 * (r >> 2) >= VIT16_N) continue;  // (both halves' keys are padding: P = 0 and V = 0)
            const float* vr = va + (32 * t + (r & 3) + 8 * (r >> 2)) * A16_LDV;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) ov[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32 * dt], sc[t][r], ov[dt], 0, 0, 0);
        }
    if (query >= VIT16_N) return;
    float* op = out + ((size_t)b * VIT16_N + query) * D + h * VIT_HD + 4 * half;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(op + 32 * dt + 8 * g) = make_float4(ov[dt][4 * g + 0] / sum, ov[dt][4 * g + 1] / sum,
                                                                           ov[dt][4 * g + 2] / sum, ov[dt][4 * g + 3] / sum);
}

// Any token count N >= 1 (the plans of orbit_vit_create_sized): the scheme of vit_attention197_kernel made streaming. One
// workgroup of 4 waves per (frame, head, block of 128 queries); a wave owns 32 queries and keeps, per lane, its query (32 of the
// 64 d, pre-scaled), one 32-key tile of S^T, the running maximum and (half-)sum and the two O^T accumulators - nothing grows with
// N. K and V pass through LDS in tiles of 32 keys, [32][65] + [32][72] floats = 17 536 bytes, the row strides of the 197 kernel;
// the next tile is read from memory into registers while the MFMAs of the current one run. Per tile: S^T = K (Q/8)^T, keys past
// N - 1 to -inf (their K and V rows are staged as zeros), m' = max(m, tile maximum), the sum and the accumulators times
// exp(m - m'), P^T = exp(S^T - m') straight into O^T += V^T P^T. Tiles go in ascending order, so tile 0 holds key 0: m' is finite
// from the first step on, exp(-inf - m') = 0 wipes the (zero) initial state and (-inf) - (-inf) never occurs. Queries past N - 1
// re-read query N - 1 and are never stored; a wave with no valid query only helps staging. The order of every sum is fixed by N
// alone: a row's bits do not depend on B, on the query's place in its block or on the other workgroups.
constexpr int AN_WAVES = 4;
constexpr int AN_QB = 32 * AN_WAVES;  // queries per workgroup
constexpr int AN_KT = 32;             // keys per tile
static_assert(AN_KT * (VIT_HD / 4) == 2 * 64 * AN_WAVES, "two float4 of K and of V per thread and tile");

__global__ __launch_bounds__(64 * AN_WAVES) void vit_attention_n_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                        int N, int D, int heads, int qblocks) {
    __shared__ __attribute__((aligned(16))) float ks[AN_KT * A16_LDK];
    __shared__ __attribute__((aligned(16))) float vs[AN_KT * A16_LDV];
    const int qb = blockIdx.x % qblocks, bh = blockIdx.x / qblocks, b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const float* base = qkv + (size_t)b * N * 3 * D + h * VIT_HD;
    const int q0 = AN_QB * qb + 32 * wave;  // this wave's first query
    const bool active = q0 < N;             // (wave-uniform)
    const int query = q0 + col;
    float qf[32];
    {
        const float* qp = base + (size_t)(query < N ? query : N - 1) * 3 * D + 32 * half;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 q4 = *reinterpret_cast<const float4*>(qp + 4 * i);
            qf[4 * i + 0] = q4.x * 0.125f, qf[4 * i + 1] = q4.y * 0.125f, qf[4 * i + 2] = q4.z * 0.125f, qf[4 * i + 3] = q4.w * 0.125f;
        }
    }
    // staging: thread -> (key tid >> 4 and 16 + (tid >> 4), four d at 4 (tid & 15))
    const int sk = tid >> 4, sc4 = (tid & 15) * 4;
    float4 rk[2], rv[2];
    auto fetch = [&](int t) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int key = AN_KT * t + sk + 16 * i;
            rk[i] = rv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (key < N) {
                const float* r = base + (size_t)key * 3 * D + sc4;
                rk[i] = *reinterpret_cast<const float4*>(r + D);
                rv[i] = *reinterpret_cast<const float4*>(r + 2 * D);
            }
        }
    };

    float m = -INFINITY, sum = 0.f;  // running maximum (both lane halves agree) and this lane half's share of the sum
    floatx16 ov[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) ov[dt][r] = 0.f;
    const float* ka = ks + col * A16_LDK + 32 * half;
    const float* va = vs + 4 * half * A16_LDV + col;

    const int nt = (N + AN_KT - 1) / AN_KT;
    fetch(0);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();  // the previous tile has been read by every wave
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float* kd = ks + (sk + 16 * i) * A16_LDK + sc4;
            kd[0] = rk[i].x, kd[1] = rk[i].y, kd[2] = rk[i].z, kd[3] = rk[i].w;
            *reinterpret_cast<float4*>(vs + (sk + 16 * i) * A16_LDV + sc4) = rv[i];
        }
        __syncthreads();
        if (t + 1 < nt) fetch(t + 1);
        if (!active) continue;
        // S^T tile: rows = keys 32 t + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's query
        floatx16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[kk], qf[kk], sc, 0, 0, 0);
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (AN_KT * t + (r & 3) + 8 * (r >> 2) + 4 * half >= N) sc[r] = -INFINITY;
            mt = fmaxf(mt, sc[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);
        const float scale = expf(m - mn);  // tile 0: exp(-inf) = 0 on a zero state
        m = mn;
        float ts = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = expf(sc[r] - mn), ts += sc[r];
        sum = sum * scale + ts;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ov[dt][r] *= scale;
        // O^T tile dt: rows = d 32 dt + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's query
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* vr = va + ((r & 3) + 8 * (r >> 2)) * A16_LDV;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) ov[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32 * dt], sc[r], ov[dt], 0, 0, 0);
        }
    }
    if (!active || query >= N) return;
    sum += __shfl_xor(sum, 32);
    float* op = out + ((size_t)b * N + query) * D + h * VIT_HD + 4 * half;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(op + 32 * dt + 8 * g) = make_float4(ov[dt][4 * g + 0] / sum, ov[dt][4 * g + 1] / sum,
                                                                           ov[dt][4 * g + 2] / sum, ov[dt][4 * g + 3] / sum);
}

int launch_attention_n(const float* qkv, float* out, int B, int N, int D, int heads, hipStream_t s) {
    const int qblocks = cdiv(N, AN_QB);
    const int pi = prof_start("vit_attention_n", 4.0 * B * heads * (double)N * N * VIT_HD, 4.0 * 4 * (double)B * N * D, s);
    vit_attention_n_kernel<<<B * heads * qblocks, 64 * AN_WAVES, 0, s>>>(qkv, out, N, D, heads, qblocks);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// N: tokens per frame: 50 (the LDS-resident VALU kernel), 197 (the MFMA kernel) or anything else (the streaming MFMA kernel);
// but for 50, qkv and out are 16-byte aligned
int launch_attention(const float* qkv, float* out, int B, int N, int D, int heads, hipStream_t s) {
    if (N < 1) return set_err(ORBIT_ERR_ARG, "vit attention: %d tokens", N);
    if (N != VIT_N && N != VIT16_N) return launch_attention_n(qkv, out, B, N, D, heads, s);
    static bool attr_set = false;  // > 64 KiB of dynamic LDS needs the opt-in once
    if (N == VIT16_N && !attr_set) {
        ORBIT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(vit_attention197_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)A16_LDS_BYTES));
        attr_set = true;
    }
    const int pi = prof_start(N == VIT_N ? "vit_attention" : "vit_attention197", 4.0 * B * heads * N * N * VIT_HD,
                              4.0 * 4 * (double)B * N * D, s);
    if (N == VIT_N)
        vit_attention_kernel<<<B * heads, 256, 0, s>>>(qkv, out, D, heads);
    else
        vit_attention197_kernel<<<B * heads, 64 * A16_WAVES, A16_LDS_BYTES, s>>>(qkv, out, D, heads);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// ---- backward kernels (frozen network: data gradients and the per-slot LayerNorm dgamma / dbeta) -----------------------
// in [R][C] -> out [C][R] with the library's transpose (csrc/ops.hip): the K-contiguous copy of a Linear weight that the
// data-gradient GEMM reads. Runs once per parameter upload, not per step.
int vit_transpose(const float* in, float* out, int R, int C, hipStream_t s) {
    const int pi = prof_start("vit_transpose", 0.0, 8.0 * R * C, s);
    const int rc = launch_transpose(in, out, R, C, s);
    prof_stop(pi, s);
    return rc;
}

// qkv [B*50][3D], dout [B*50][D] (gradient of the attention output) -> dqkv [B*50][3D] (the [B][50][3][heads][64] layout of
// qkv). One workgroup per (frame, head) as the forward; S and P are recomputed by a copy of the forward's code (keep the two in step), then
//   dV = P^T dO,  dP = dO V^T,  dS = P o (dP - rowsum(dP o P)) (in place over P),  dQ = dS K / 8,  dK = dS^T Q / 8.
// LDS: Q, dO 50 x 64, K, V 50 x 65, P 50 x 52 floats = 62 016 bytes with alignment: two workgroups (8 waves) per CU of 160 KB - the same
// two-per-SIMD occupancy the 256-thread forward reaches with its 46 KB; the kernel is LDS-latency bound either way.
__global__ __launch_bounds__(256) void vit_attention_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                float* __restrict__ dqkv, int D, int heads) {
    constexpr int LDK = VIT_HD + 1, LDS_ = 52;
    __shared__ float q[VIT_N * VIT_HD], k[VIT_N * LDK], v[VIT_N * LDK], go[VIT_N * VIT_HD], sc[VIT_N * LDS_];
    const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x;
    const float* base = qkv + (size_t)b * VIT_N * 3 * D + h * VIT_HD;
    float* dbase = dqkv + (size_t)b * VIT_N * 3 * D + h * VIT_HD;
    for (int i = tid; i < VIT_N * VIT_HD; i += 256) {
        const int t = i >> 6, d = i & 63;
        const float* r = base + (size_t)t * 3 * D + d;
        q[i] = r[0];
        k[t * LDK + d] = r[D];
        v[t * LDK + d] = r[2 * D];
        go[i] = dout[((size_t)b * VIT_N + t) * D + h * VIT_HD + d];
    }
    __syncthreads();
    for (int i = tid; i < VIT_N * VIT_N; i += 256) {
        const int r = i / VIT_N, c = i - r * VIT_N;
        float acc = 0.f;
#pragma unroll 16
        for (int d = 0; d < VIT_HD; ++d) acc = fmaf(q[r * VIT_HD + d], k[c * LDK + d], acc);
        sc[r * LDS_ + c] = acc * 0.125f;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < VIT_N; r += 4) {
        const float val = lane < VIT_N ? sc[r * LDS_ + lane] : -INFINITY;
        const float m = wave_max_xor(val);
        const float e = lane < VIT_N ? expf(val - m) : 0.f;
        const float sum = wave_sum_xor(e);
        if (lane < VIT_N) sc[r * LDS_ + lane] = e / sum;
    }
    __syncthreads();
    for (int i = tid; i < VIT_N * VIT_HD; i += 256) {  // dV[c][d] = sum_r P[r][c] dO[r][d]
        const int c = i >> 6, d = i & 63;
        float acc = 0.f;
#pragma unroll 10
        for (int r = 0; r < VIT_N; ++r) acc = fmaf(sc[r * LDS_ + c], go[r * VIT_HD + d], acc);
        dbase[(size_t)c * 3 * D + 2 * D + d] = acc;
    }
    __syncthreads();
    for (int r = wave; r < VIT_N; r += 4) {  // row r of dS over row r of P; lane = key
        float dp = 0.f;
        if (lane < VIT_N) {
#pragma unroll 16
            for (int d = 0; d < VIT_HD; ++d) dp = fmaf(go[r * VIT_HD + d], v[lane * LDK + d], dp);
        }
        const float p = lane < VIT_N ? sc[r * LDS_ + lane] : 0.f;
        const float t = wave_sum_xor(dp * p);
        if (lane < VIT_N) sc[r * LDS_ + lane] = p * (dp - t);
    }
    __syncthreads();
    for (int i = tid; i < VIT_N * VIT_HD; i += 256) {
        const int r = i >> 6, d = i & 63;  // (r is the query row of dQ and the key row of dK)
        float aq = 0.f, ak = 0.f;
#pragma unroll 10
        for (int c = 0; c < VIT_N; ++c) {
            aq = fmaf(sc[r * LDS_ + c], k[c * LDK + d], aq);
            ak = fmaf(sc[c * LDS_ + r], q[c * VIT_HD + d], ak);
        }
        dbase[(size_t)r * 3 * D + d] = aq * 0.125f;
        dbase[(size_t)r * 3 * D + D + d] = ak * 0.125f;
    }
}

// The same for the 197 tokens of the patch-16 models, on v_mfma_f32_32x32x2_f32 as vit_attention197_kernel, whose tile layout
// (A16_NPAD = 224 padded tokens, 7 waves, lane = (column, k half)) it shares. Q, K, V and dO of a head are 4 x 197 x 64 floats and
// do not fit LDS together, so one workgroup per (frame, head) runs two phases over two [224][65] LDS matrices (rows 197..223
// zero; the odd stride serves both the row-major A fragments - 32 rows, 32 banks - and the transposed ones):
//   A  LDS = K, V. A wave owns 32 queries, its lane one query's column: S^T = K (Q/8)^T (ab16_score_tile), 7 tiles held, softmax in
//      the lane plus one exchange, P^T in place. dP^T = V dO^T is streamed tile by tile, twice: once for delta = sum_k P dP, once
//      for dS^T = P^T o (dP^T - delta), which is at once the B operand of dQ^T += K^T dS^T. The statistics of every query go
//      to a small LDS array (m, l and delta); dQ = dQ^T / 8 is stored.
//   B  every wave takes its 32 keys' K / 8 and V rows out of LDS into registers, then LDS = Q, dO. A lane owns one key's column:
//      S = Q (K/8)^T (the same products in the same order as phase A: the same bits), P from the saved m and l, dP = dO V^T,
//      dS; dV^T += dO^T P and dK^T += Q^T dS over the 7 query tiles; dK = dK^T / 8 and dV are stored.
// No wave adds into another's output and no sum depends on another workgroup: fixed order, no atomics. Padding: keys 197..223
// get S = -inf in phase A and P = 0 by a select in phase B (their columns are never stored); queries 197..223 are never stored
// in phase A and enter phase B as Q = dO = 0 rows with l = inf, so P = dS = 0 exactly: they add nothing to dK or dV.
constexpr int AB16_LD = VIT_HD + 1;
constexpr int AB16_MAT = A16_NPAD * AB16_LD;  // floats of one padded matrix
constexpr size_t AB16_LDS_BYTES = (size_t)(2 * AB16_MAT + 3 * A16_NPAD) * sizeof(float);  // 119 168

// rows 0..196 of two [197][64] global matrices (row strides in floats) into the two LDS matrices, rows 197..223 zero
__device__ __forceinline__ void ab16_stage(float* m0, float* m1, const float* g0, size_t s0, const float* g1, size_t s1, int tid) {
    for (int i = tid; i < A16_NPAD * (VIT_HD / 4); i += 64 * A16_WAVES) {
        const int t = i >> 4, c = (i & 15) * 4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (t < VIT16_N) {
            a = *reinterpret_cast<const float4*>(g0 + (size_t)t * s0 + c);
            b = *reinterpret_cast<const float4*>(g1 + (size_t)t * s1 + c);
        }
        float* d0 = m0 + t * AB16_LD + c;
        float* d1 = m1 + t * AB16_LD + c;
        d0[0] = a.x, d0[1] = a.y, d0[2] = a.z, d0[3] = a.w;
        d1[0] = b.x, d1[1] = b.y, d1[2] = b.z, d1[3] = b.w;
    }
}

// the 16 registers of a tile in chains of 4, and 7 tile sums: fixed orders
__device__ __forceinline__ float ab16_sum16(const floatx16& x) {
    const float a = ((x[0] + x[1]) + x[2]) + x[3], b = ((x[4] + x[5]) + x[6]) + x[7];
    const float c = ((x[8] + x[9]) + x[10]) + x[11], d = ((x[12] + x[13]) + x[14]) + x[15];
    return (a + b) + (c + d);
}
__device__ __forceinline__ float ab16_sum7(const float* t) { return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + t[6]); }

// float offset of tile t's first row, kept out of the compiler's sight: folded into every LDS address of an unrolled tile loop
// it costs one base register per pair of reads (the two-address read's offsets are 8 bits), which spills; as a value the reads
// of a tile share one base and their offsets fit the instruction
__device__ __forceinline__ int ab16_tile_offset(int t) {
    int o = 32 * t * AB16_LD;
    asm volatile("" : "+v"(o));
    return o;
}

// One 32 x 32 score tile, A fragments a[kk] out of LDS times b[kk], as four chains of 8 steps (16 products each) added pairwise.
// A logit reaches exp() with the rounding errors of its chain at the logit's own size (up to 15 in a peaked row), and a single
// 64-product chain - fine for the forward's outputs - puts dK of a dominant key past what a blocked fp32 evaluation gives.
// Both phases call this with the operands' roles swapped: the same products in the same order, the same bits.
__device__ __forceinline__ floatx16 ab16_score_tile(const float* a, const float (&b)[32]) {
    floatx16 part[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) part[c][r] = 0.f;
#pragma unroll
        for (int kk = 8 * c; kk < 8 * c + 8; ++kk) part[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], part[c], 0, 0, 0);
    }
    floatx16 out;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = (part[0][r] + part[1][r]) + (part[2][r] + part[3][r]);
    return out;
}

__global__ __launch_bounds__(64 * A16_WAVES) void vit_attention197_bwd_kernel(const float* __restrict__ qkv,
                                                                              const float* __restrict__ dout,
                                                                              float* __restrict__ dqkv, int D, int heads) {
    extern __shared__ __attribute__((aligned(16))) float ab16_sm[];
    float* m0s = ab16_sm;             // K, then Q
    float* m1s = ab16_sm + AB16_MAT;  // V, then dO
    float* st_m = ab16_sm + 2 * AB16_MAT;
    float* st_l = st_m + A16_NPAD;
    float* st_dl = st_l + A16_NPAD;
    const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const size_t row0 = (size_t)b * VIT16_N;
    const float* base = qkv + row0 * 3 * D + h * VIT_HD;
    const float* dob = dout + row0 * D + h * VIT_HD;
    float* dbase = dqkv + row0 * 3 * D + h * VIT_HD;
    const int own = 32 * wave + col;  // this lane's query (phase A) and key (phase B)
    const bool valid = own < VIT16_N;
    const int ownc = valid ? own : VIT16_N - 1;  // (padded lanes re-read token 196; nothing of theirs is stored)

    // ---- phase A ----
    ab16_stage(m0s, m1s, base + D, (size_t)3 * D, base + 2 * D, (size_t)3 * D, tid);
    {
        float qf[32];  // this lane's query, d = 32 half .. 32 half + 31, times head_dim ** -0.5 (a power of two: exact)
        {
            const float* qp = base + (size_t)ownc * 3 * D + 32 * half;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 q4 = *reinterpret_cast<const float4*>(qp + 4 * i);
                qf[4 * i + 0] = q4.x * 0.125f, qf[4 * i + 1] = q4.y * 0.125f, qf[4 * i + 2] = q4.z * 0.125f, qf[4 * i + 3] = q4.w * 0.125f;
            }
        }
        __syncthreads();
        // S^T tile t: rows = keys 32 t + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's query
        floatx16 sc[A16_WAVES];
        const float* ka = m0s + col * AB16_LD + 32 * half;
#pragma unroll
        for (int t = 0; t < A16_WAVES; ++t) sc[t] = ab16_score_tile(ka + ab16_tile_offset(t), qf);
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < A16_WAVES; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (t == A16_WAVES - 1 && 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half >= VIT16_N) sc[t][r] = -INFINITY;
                m = fmaxf(m, sc[t][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 32));
        // the denominator and delta below are summed in short chains (4 registers, 4 of those, 7 tiles, 2 halves), not in one
        // 112-term chain: where one key dominates, dS = P (dP - delta) cancels and carries their rounding errors at full size
        float tsum[A16_WAVES];
#pragma unroll
        for (int t = 0; t < A16_WAVES; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[t][r] = expf(sc[t][r] - m);
            tsum[t] = ab16_sum16(sc[t]);
        }
        float sum = ab16_sum7(tsum);
        sum += __shfl_xor(sum, 32);
#pragma unroll
        for (int t = 0; t < A16_WAVES; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[t][r] /= sum;  // P^T (a division: one rounding, as the fp32 reference)

        float dof[32];  // this lane's dO row, d = 32 half .. 32 half + 31
        {
            const float* op = dob + (size_t)ownc * D + 32 * half;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 o4 = *reinterpret_cast<const float4*>(op + 4 * i);
                dof[4 * i + 0] = o4.x, dof[4 * i + 1] = o4.y, dof[4 * i + 2] = o4.z, dof[4 * i + 3] = o4.w;
            }
        }
        // delta = sum over the keys of P dP, dP^T tile t = V[keys of t] dO^T: in (tile, register) order, then the other half
        const float* va = m1s + col * AB16_LD + 32 * half;
#pragma unroll
        for (int t = 0; t < A16_WAVES; ++t) {
            const int to = ab16_tile_offset(t);
            floatx16 dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(va[to + kk], dof[kk], dp, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[r] *= sc[t][r];
            tsum[t] = ab16_sum16(dp);
        }
        float delta = ab16_sum7(tsum);
        delta += __shfl_xor(delta, 32);
        // (a padded query: l = inf, so that phase B gets P = exp(0 - 0) / inf = 0 for it)
        if (half == 0) st_m[own] = valid ? m : 0.f, st_l[own] = valid ? sum : INFINITY, st_dl[own] = valid ? delta : 0.f;

        // dQ^T tile dt: rows = d 32 dt + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's query
        floatx16 dq[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
        const float* kt = m0s + 4 * half * AB16_LD + col;
#pragma unroll
        for (int t = 0; t < A16_WAVES; ++t) {
            const int to = ab16_tile_offset(t);
            floatx16 dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(va[to + kk], dof[kk], dp, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (32 * t + 8 * (r >> 2) >= VIT16_N) continue;  // (both halves' keys are padding: dS = 0 and K = 0)
                const float ds = sc[t][r] * (dp[r] - delta);
                const float* kr = kt + to + ((r & 3) + 8 * (r >> 2)) * AB16_LD;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[32 * dt], ds, dq[dt], 0, 0, 0);
            }
        }
        if (valid) {
            float* qo = dbase + (size_t)own * 3 * D + 4 * half;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<float4*>(qo + 32 * dt + 8 * g) =
                        make_float4(dq[dt][4 * g + 0] * 0.125f, dq[dt][4 * g + 1] * 0.125f, dq[dt][4 * g + 2] * 0.125f,
                                    dq[dt][4 * g + 3] * 0.125f);
        }
    }

    // ---- phase B ----
    float kf[32], vf[32];  // this lane's key: K / 8 and V, d = 32 half .. 32 half + 31 (rows 197..223: zero)
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        kf[kk] = m0s[own * AB16_LD + 32 * half + kk] * 0.125f;
        vf[kk] = m1s[own * AB16_LD + 32 * half + kk];
    }
    __syncthreads();  // every wave has its keys and is done with K and V
    ab16_stage(m0s, m1s, base, (size_t)3 * D, dob, (size_t)D, tid);
    __syncthreads();
    // dV^T / dK^T tile dt: rows = d 32 dt + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's key
    floatx16 dv[2], dk[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[dt][r] = 0.f, dk[dt][r] = 0.f;
    const float* qa = m0s + col * AB16_LD + 32 * half;
    const float* oa = m1s + col * AB16_LD + 32 * half;
    const float* qt = m0s + 4 * half * AB16_LD + col;
    const float* ot = m1s + 4 * half * AB16_LD + col;
#pragma unroll 1
    for (int t = 0; t < A16_WAVES; ++t) {
        // S and dP tile t: rows = queries 32 t + (r & 3) + 8 (r >> 2) + 4 half, column = this lane's key
        const floatx16 sq = ab16_score_tile(qa + 32 * t * AB16_LD, kf);
        floatx16 dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(oa[32 * t * AB16_LD + kk], vf[kk], dp, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = 32 * t + (r & 3) + 8 * (r >> 2);
            const int q = qr + 4 * half;
            float p = expf(sq[r] - st_m[q]) / st_l[q];
            p = valid ? p : 0.f;
            const float ds = p * (dp[r] - st_dl[q]);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ot[qr * AB16_LD + 32 * dt], p, dv[dt], 0, 0, 0);
                dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(qt[qr * AB16_LD + 32 * dt], ds, dk[dt], 0, 0, 0);
            }
        }
    }
    if (!valid) return;
    float* ko = dbase + (size_t)own * 3 * D + D + 4 * half;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            *reinterpret_cast<float4*>(ko + 32 * dt + 8 * g) =
                make_float4(dk[dt][4 * g + 0] * 0.125f, dk[dt][4 * g + 1] * 0.125f, dk[dt][4 * g + 2] * 0.125f, dk[dt][4 * g + 3] * 0.125f);
            *reinterpret_cast<float4*>(ko + D + 32 * dt + 8 * g) =
                make_float4(dv[dt][4 * g + 0], dv[dt][4 * g + 1], dv[dt][4 * g + 2], dv[dt][4 * g + 3]);
        }
}

// N: tokens per frame, 50 (the LDS-resident VALU kernel) or 197 (the MFMA kernel; qkv, dout and dqkv 16-byte aligned)
int launch_attention_bwd(const float* qkv, const float* dout, float* dqkv, int B, int N, int D, int heads, hipStream_t s) {
    if (N != VIT_N && N != VIT16_N) return set_err(ORBIT_ERR_ARG, "vit attention backward: %d tokens (50 or 197)", N);
    static bool attr_set = false;  // > 64 KiB of dynamic LDS needs the opt-in once
    if (N == VIT16_N && !attr_set) {
        ORBIT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(vit_attention197_bwd_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)AB16_LDS_BYTES));
        attr_set = true;
    }
    const int pi = prof_start(N == VIT_N ? "vit_attention_bwd" : "vit_attention197_bwd", 10.0 * B * heads * N * N * VIT_HD,
                              4.0 * 7 * (double)B * N * D, s);
    if (N == VIT_N)
        vit_attention_bwd_kernel<<<B * heads, 256, 0, s>>>(qkv, dout, dqkv, D, heads);
    else
        vit_attention197_bwd_kernel<<<B * heads, 64 * A16_WAVES, AB16_LDS_BYTES, s>>>(qkv, dout, dqkv, D, heads);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// LayerNorm backward, one wave per row with the row in registers, 64 rows per block (16 per wave, interleaved). mean / rstd
// are recomputed by a copy of the forward's code that must be kept in step with it (mean by division, see vit_layernorm_kernel).
//   xhat = (x - mean) rstd,  g = dy o gamma,  dx = rstd (g - mean(g) - xhat mean(g o xhat))  [+ dres]
// dx == nullptr: no data gradient (block 0's norm1). dres may alias dx. With dx_stride > D (the final norm: token 0 of every
// frame carries a gradient, the other 49 tokens none) only the D floats of each row are written: the caller zeroes the stream.
// Per-channel sums of dy and dy o xhat over the block's rows go to partial[block][2][D] (waves added in wave order);
// vit_layernorm_bwd_finalize_kernel adds the blocks in block order.
constexpr int LNB_ROWS = 64;
template <int NPL>
__global__ __launch_bounds__(256) void vit_layernorm_bwd_kernel(const float* x, size_t x_stride, const float* dy,
                                                                size_t dy_stride, const float* __restrict__ g, float eps,
                                                                const float* dres, float* dx, size_t dx_stride, int rows,
                                                                float* __restrict__ partial) {
    constexpr int D = NPL * 64;
    __shared__ float red[3][2][D];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float gam[NPL], sb[NPL], sg[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) gam[i] = g[lane + 64 * i], sb[i] = 0.f, sg[i] = 0.f;
    for (int j = 0; j < LNB_ROWS / 4; ++j) {
        const int row = blockIdx.x * LNB_ROWS + 4 * j + wave;
        if (row >= rows) break;  // (wave-uniform)
        const float* xr = x + (size_t)row * x_stride;
        const float* dyr = dy + (size_t)row * dy_stride;
        float v[NPL], d[NPL];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) v[i] = xr[lane + 64 * i], d[i] = dyr[lane + 64 * i], s += v[i];
        const float mean = wave_sum_xor(s) / D;
        float qq = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) v[i] -= mean, qq += v[i] * v[i];
        const float rstd = 1.f / sqrtf(wave_sum_xor(qq) * (1.f / D) + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            v[i] *= rstd;  // xhat
            sb[i] += d[i];
            sg[i] += d[i] * v[i];
            d[i] *= gam[i];  // g
            s1 += d[i];
            s2 += d[i] * v[i];
        }
        if (!dx) continue;
        const float m1 = wave_sum_xor(s1) / D, m2 = wave_sum_xor(s2) / D;
        float* dxr = dx + (size_t)row * dx_stride;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            float o = rstd * (d[i] - m1 - v[i] * m2);
            if (dres) o += dres[(size_t)row * dx_stride + lane + 64 * i];
            dxr[lane + 64 * i] = o;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < NPL; ++i) red[wave - 1][0][lane + 64 * i] = sb[i], red[wave - 1][1][lane + 64 * i] = sg[i];
    }
    __syncthreads();
    if (wave == 0) {
        float* pr = partial + (size_t)blockIdx.x * 2 * D;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
            const int c = lane + 64 * i;
            pr[c] = ((sb[i] + red[0][0][c]) + red[1][0][c]) + red[2][0][c];
            pr[D + c] = ((sg[i] + red[0][1][c]) + red[1][1][c]) + red[2][1][c];
        }
    }
}

__global__ __launch_bounds__(256) void vit_layernorm_bwd_finalize_kernel(const float* __restrict__ partial, int nblocks, int D,
                                                                         float* __restrict__ dbeta, float* __restrict__ dgamma) {
    const int i = blockIdx.x * 256 + threadIdx.x;  // [2][D]: dbeta then dgamma
    if (i >= 2 * D) return;
    float acc = 0.f;
    for (int b = 0; b < nblocks; ++b) acc += partial[(size_t)b * 2 * D + i];
    if (i < D) dbeta[i] = acc;
    else dgamma[i - D] = acc;
}

// zeroes of a gradient stream that the final norm's backward then writes token 0 of every frame into
int zero_gradient_stream(float* dx, size_t floats, hipStream_t s) {
    const int pi = prof_start("vit_grad_stream_zero", 0.0, 4.0 * floats, s);
    const hipError_t e = hipMemsetAsync(dx, 0, floats * sizeof(float), s);
    prof_stop(pi, s);
    ORBIT_HIP_CHECK(e);
    return ORBIT_OK;
}

size_t layernorm_bwd_partial_floats(int rows, int D) { return (size_t)cdiv(rows, LNB_ROWS) * 2 * D; }

int launch_layernorm_bwd(const float* x, size_t xs, const float* dy, size_t dys, const float* g, float eps, const float* dres,
                         float* dx, size_t dxs, int rows, int D, float* partial, float* dgamma, float* dbeta, hipStream_t s) {
    if (D != 384 && D != 768) return set_err(ORBIT_ERR_ARG, "vit layernorm backward: unsupported width %d", D);
    const int nblocks = cdiv(rows, LNB_ROWS);
    int pi = prof_start("vit_layernorm_bwd", 16.0 * rows * D, 4.0 * (dx ? 3 : 2) * rows * D, s);
    if (D == 384)
        vit_layernorm_bwd_kernel<6><<<nblocks, 256, 0, s>>>(x, xs, dy, dys, g, eps, dres, dx, dxs, rows, partial);
    else
        vit_layernorm_bwd_kernel<12><<<nblocks, 256, 0, s>>>(x, xs, dy, dys, g, eps, dres, dx, dxs, rows, partial);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    pi = prof_start("vit_layernorm_bwd_finalize", 2.0 * nblocks * D, 8.0 * nblocks * D, s);
    vit_layernorm_bwd_finalize_kernel<<<cdiv(2 * D, 256), 256, 0, s>>>(partial, nblocks, D, dbeta, dgamma);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}


// ---- weight gradients (orbit_vit_backward_params) ----------------------------------------------------------------------
// dW [N][K] = dY^T X, dY [M][N] and X [M][K] row-major: the reduction runs over the token rows, the slow dimension of both
// operands, so a 32-row step of either is float4 loads along n / k that land in LDS already reduction-major ([m][n], [m][k]) -
// the layout the MFMA fragment reads of vit_gemm_kernel want, without its transposing scatter. One block owns a 128 (n) x 128 (k)
// tile of dW and one of `splits` contiguous ranges of 32-row steps (the output is small and M is long: 27 tiles for the ViT-S
// qkv layer); it writes its partial tile to the workspace and vit_wgrad_reduce_kernel adds the partials in split order. The
// split count is wgrad_splits(M, N, K), nothing else: results are bitwise reproducible. Inside a split the chain is cut every
// 256 rows as in the BLOCKED data-gradient GEMMs. Rows past M are never loaded and enter the sums as exact zeros (they would be
// summed here, not merely left unstored as in the forward). Columns past K (K a multiple of 32, not of 128) likewise.
//   WX_GELU   X = GELU_erf(u), applied to the loaded registers (fc2: only the pre-activation is on the tape)
//   WX_PATCH  X = the patches gathered from the NCHW frames (patch_row_ptr), dY row m = token 1 + m % 49 of frame m / 49
//   WX_PATCH16  the same for 16 x 16 patches (patch16_row_ptr, k = c*256 + kh*16 + kw, K = 768, M = 196 B), dY row m = token
//             1 + m % 196 of frame m / 196 of the [B][197][D] stream. A float4 chunk of four consecutive k lies inside one
//             16-float patch row, 16-byte aligned (kw = 0, 4, 8, 12; patch columns start at multiples of 64 bytes). A loader's
//             32 chunks (128 k) cover eight frame rows of one channel with 64 contiguous bytes each, where patch-32 covers four
//             rows of 128 bytes: a wave's load (rows m, m + 1 x 32 chunks) is 16 runs of 64 bytes instead of 8 of 128. The
//             wave's two rows are an even m and m + 1, and 14 and 196 are even, so they are always the patches pw, pw + 1 (pw
//             even) of one patch row: the two 64-byte runs of a frame row are the halves of one 128-byte line (frames at least
//             128-byte aligned, as torch allocates them). The wave therefore still touches 8 whole lines per load and no frame
//             byte is fetched twice; the difference to patch-32 is that a line is covered by lanes l..l+3 and l+32..l+35
//             instead of eight consecutive lanes: four dwordx4 lanes per contiguous run instead of eight.
// The bias gradient db [n] = sum_m dY [m][n] is folded into the blocks of k-tile 0, which sum the dY tile they hold in LDS (32
// rows into a fresh sum per step, steps and 256-row chunks as the accumulators): dY is not read a second time.
constexpr int W_BT = 128;
enum { WX_PLAIN = 0, WX_GELU = 1, WX_PATCH = 2, WX_PATCH16 = 3 };

struct WgradArgs {
    const float* dy;
    const float* x;
    float* dw;  // [N][K], or with splits > 1 the partial tiles [splits][N][K]
    float* db;  // nullptr, [N], or with splits > 1 [splits][N]
    int M, N, K, splits;
};

// doubles while the grid stays within 512 blocks (two 256-thread blocks per CU) and every split keeps at least four 32-row steps:
// the split count changes at M = 225, 481, 993, 2017, 4065, ... and nowhere else
int wgrad_splits(int M, int N, int K) {
    const long tiles = (long)(N / W_BT) * cdiv(K, W_BT);
    const int steps = cdiv(M, G_BK);
    int s = 1;
    while (2 * s * tiles <= 512 && 8 * s <= steps) s *= 2;
    return s;
}
size_t wgrad_ws_floats(int M, int N, int K) {
    const int s = wgrad_splits(M, N, K);
    return s > 1 ? (size_t)s * ((size_t)N * K + N) : 0;
}

template <int XM>
__global__ __launch_bounds__(G_THREADS, 2) void vit_wgrad_kernel(WgradArgs a) {
    constexpr int LD = W_BT + 4;
    __shared__ __attribute__((aligned(16))) float As[G_BK * LD];  // dY tile [m][n]
    __shared__ __attribute__((aligned(16))) float Bs[G_BK * LD];  // X tile [m][k]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int k0 = blockIdx.x * W_BT, n0 = blockIdx.y * W_BT, sp = blockIdx.z;
    const int steps = (a.M + G_BK - 1) / G_BK;
    const int s_begin = (int)((long)sp * steps / a.splits), s_end = (int)((long)(sp + 1) * steps / a.splits);
    const int lc = tid & 31, lr = tid >> 5;  // loader: float4 chunk along n / k, and row (lr + 8 i)
    const bool k_in = k0 + 4 * lc < a.K;
    const bool bias_block = a.db != nullptr && blockIdx.x == 0;

    floatx16 acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f, tot[i][j][r] = 0.f;
    float bacc = 0.f, btot = 0.f;

    float4 ra[4], rb[4];
    auto load = [&](int st) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = st * G_BK + lr + 8 * i;
            ra[i] = rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m >= a.M) continue;
            const size_t dyrow = XM == WX_PATCH     ? (size_t)(m / VIT_P) * VIT_N + 1 + m % VIT_P
                                 : XM == WX_PATCH16 ? (size_t)(m / VIT16_P) * VIT16_N + 1 + m % VIT16_P
                                                    : (size_t)m;
            ra[i] = *reinterpret_cast<const float4*>(a.dy + dyrow * a.N + n0 + 4 * lc);
            if (!k_in) continue;
            const float* xp = XM == WX_PATCH     ? patch_row_ptr(a.x, m, k0 + 4 * lc)
                              : XM == WX_PATCH16 ? patch16_row_ptr(a.x, m, k0 + 4 * lc)
                                                 : a.x + (size_t)m * a.K + k0 + 4 * lc;
            rb[i] = *reinterpret_cast<const float4*>(xp);
            if (XM == WX_GELU) rb[i] = make_float4(gelu_erf(rb[i].x), gelu_erf(rb[i].y), gelu_erf(rb[i].z), gelu_erf(rb[i].w));
        }
    };

    if (s_begin < s_end) load(s_begin);
    for (int st = s_begin; st < s_end; ++st) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<float4*>(&As[(lr + 8 * i) * LD + 4 * lc]) = ra[i];
            *reinterpret_cast<float4*>(&Bs[(lr + 8 * i) * LD + 4 * lc]) = rb[i];
        }
        __syncthreads();
        if (st + 1 < s_end) load(st + 1);  // next step in flight during the MFMAs
        const int kh = lane >> 5, col = lane & 31;
#pragma unroll
        for (int kk = 0; kk < G_BK / 2; ++kk) {
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = As[(2 * kk + kh) * LD + wm * 64 + 32 * i + col];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Bs[(2 * kk + kh) * LD + wn * 64 + 32 * j + col];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (bias_block && tid < W_BT) {  // (waves 0 and 1: wave-uniform)
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < G_BK; ++r) s += As[r * LD + tid];
            bacc += s;
        }
        if (((st - s_begin) & 7) == 7 || st + 1 == s_end) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tot[i][j][r] += acc[i][j][r], acc[i][j][r] = 0.f;
            btot += bacc, bacc = 0.f;
        }
    }

    // dW[n][k]: C row = n, C col = k (the lanes of a store run along k)
    float* out = a.dw + (a.splits > 1 ? (size_t)sp * a.N * a.K : 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = k0 + wn * 64 + 32 * j + (lane & 31);
            if (col >= a.K) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = n0 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                out[(size_t)row * a.K + col] = tot[i][j][r];
            }
        }
    if (bias_block && tid < W_BT) a.db[(a.splits > 1 ? (size_t)sp * a.N : 0) + n0 + tid] = btot;
}

// part: [splits][nk] then (db) [splits][n]; the splits are added in split order, four consecutive floats per thread
__global__ __launch_bounds__(256) void vit_wgrad_reduce_kernel(const float* __restrict__ part, int splits, size_t nk, size_t n,
                                                               float* __restrict__ dw, float* __restrict__ db) {
    const size_t e = 4 * ((size_t)blockIdx.x * 256 + threadIdx.x);
    if (e >= nk + (db ? n : 0)) return;
    const bool w = e < nk;
    const float* src = w ? part + e : part + splits * nk + (e - nk);
    const size_t stride = w ? nk : n;
    float4 acc = *reinterpret_cast<const float4*>(src);
    for (int s = 1; s < splits; ++s) {
        const float4 v = *reinterpret_cast<const float4*>(src + s * stride);
        acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
    }
    *reinterpret_cast<float4*>(w ? dw + e : db + (e - nk)) = acc;
}

// ws: wgrad_ws_floats(M, N, K) floats, 16-byte aligned (unused when the rule gives one split)
template <int XM>
int launch_wgrad(const float* dy, const float* x, float* dw, float* db, int M, int N, int K, float* ws, const char* what,
                 hipStream_t s) {
    if (N % W_BT || K % G_BK || M <= 0) return set_err(ORBIT_ERR_ARG, "vit wgrad: unsupported shape M=%d N=%d K=%d", M, N, K);
    const int splits = wgrad_splits(M, N, K);
    const size_t nk = (size_t)N * K;
    WgradArgs a{dy, x, dw, db, M, N, K, splits};
    if (splits > 1) a.dw = ws, a.db = db ? ws + splits * nk : nullptr;
    char name[48];
    snprintf(name, sizeof(name), "vit_%s<%d>", what, splits);
    int pi = prof_start(name, 2.0 * M * N * K + (db ? (double)M * N : 0.0),
                        4.0 * ((double)M * N + (double)M * K + (double)splits * (nk + (db ? N : 0))), s);
    vit_wgrad_kernel<XM><<<dim3(cdiv(K, W_BT), N / W_BT, splits), G_THREADS, 0, s>>>(a);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    if (splits == 1) return ORBIT_OK;
    const size_t total = nk + (db ? N : 0);
    pi = prof_start("vit_wgrad_reduce", (double)(splits - 1) * total, 4.0 * (splits + 1) * total, s);
    vit_wgrad_reduce_kernel<<<(unsigned)((total / 4 + 255) / 256), 256, 0, s>>>(ws, splits, nk, N, dw, db);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

// gradient stream dx0 [B][N][D] (N = 50 or 197 tokens) entering the token assembly -> dpos [N][D] = sum_b dx0[b] (frames in
// ascending order, a fresh sum every 64 frames), dcls [D] = its row 0. (The patch bias gradient, the sum of rows 1..N-1, is the
// folded bias of the patch weight-gradient GEMM, which holds exactly those rows in LDS.)
__global__ __launch_bounds__(256) void vit_token_bwd_kernel(const float* __restrict__ dx0, int B, int N, int D,
                                                            float* __restrict__ dpos, float* __restrict__ dcls) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)N * D;
    if (i >= N * D) return;
    float tot = 0.f;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b1 = b0 + 64 < B ? b0 + 64 : B;
        float acc = 0.f;
#pragma unroll 4
        for (int b = b0; b < b1; ++b) acc += dx0[b * stride + i];
        tot += acc;
    }
    dpos[i] = tot;
    if (i < D) dcls[i] = tot;
}

// frames, dx0 -> d patch weight [D][3072] / [D][768], d patch bias [D] (or nullptr: CLIP), d pos_embed [50][D] / [197][D],
// d cls_token [D]; patch = 32 or 16 (validated by the callers)
int launch_patch_embed_bwd(const float* frames, const float* dx0, float* dw, float* db, float* dpos, float* dcls, int B, int D,
                           int patch, float* ws, hipStream_t s) {
    const bool p16 = patch == VIT16_PATCH;
    const int N = p16 ? VIT16_N : VIT_N;
    if (int rc = p16 ? launch_wgrad<WX_PATCH16>(dx0, frames, dw, db, B * VIT16_P, D, VIT16_KPATCH, ws, "wgrad_patch16_embed", s)
                     : launch_wgrad<WX_PATCH>(dx0, frames, dw, db, B * VIT_P, D, VIT_KPATCH, ws, "wgrad_patch_embed", s))
        return rc;
    const int pi = prof_start("vit_token_bwd", (double)B * N * D, 4.0 * (B + 1) * N * D, s);
    vit_token_bwd_kernel<<<cdiv(N * D, 256), 256, 0, s>>>(dx0, B, N, D, dpos, dcls);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

}  // namespace

// ---- plan ------------------------------------------------------------------------------------------------------------
constexpr size_t VIT_ABSENT = SIZE_MAX;
struct VitBlock {  // pool offsets (floats) of a block's twelve tensors, in state_dict order
    size_t norm1_w, norm1_b, qkv_w, qkv_b, proj_w, proj_b, norm2_w, norm2_b, fc1_w, fc1_b, fc2_w, fc2_b;
};
struct orbit_vit {
    std::string name;
    int D = 0, heads = 0, mlp = 0;
    float eps = 1e-6f;
    bool clip = false;  // pre_norm: no patch-embedding bias, norm_pre after the position add
    // geometry: patch size (32 or 16), patches per side and per frame, tokens per frame, K of the patch GEMM, largest batch.
    // The patch-16 plans are forward only (no tape, no backward) until orbit_vit_enable_backward; weight gradients only after
    // orbit_vit_enable_weight_backward
    int patch = VIT_PATCH, grid = VIT_GRID, P = VIT_P, N = VIT_N, kpatch = VIT_KPATCH, max_b = VIT_MAX_B;
    // frame side: 224 unless the plan came from orbit_vit_create_sized. Any other side is inference + FiLM only for good (the
    // attention backward and the patch filter gradient are 50 / 197-token kernels), and its forward adds the resampled table
    int side = VIT_SIZE;
    bool sized() const { return side != VIT_SIZE; }
    bool backward_enabled = false, weight_backward_enabled = false;
    bool forward_only() const { return sized() || (patch != VIT_PATCH && !backward_enabled); }
    bool weight_grads() const { return patch == VIT_PATCH || weight_backward_enabled; }
    ParamPool pool{64};  // the parameters by state_dict key (csrc/param_pool.h); 256-byte aligned tensors (float4 loads)
    // where the forward and the backward find each tensor: pool offsets, fixed by orbit_vit_create
    size_t cls = 0, pos = 0, patch_w = 0, patch_b = VIT_ABSENT, pre_w = VIT_ABSENT, pre_b = VIT_ABSENT, norm_w = 0, norm_b = 0;
    VitBlock blk[VIT_DEPTH];
    std::vector<std::string> film_names;  // FiLM slots (LayerNorm module names), D channels each
    bool finalized = false;
    double macs = 0;
    // K-contiguous transposed copies of the qkv / proj / fc1 / fc2 weights (vit_wt) for the data-gradient GEMMs: made by the
    // first orbit_vit_backward after a parameter upload, never by inference
    float* d_wt = nullptr;
    bool wt_valid = false;
    // orbit_vit_enable_bf16: qkv / proj / fc1 / fc2 run on vit_gemm_bf16_kernel from bf16 copies of their weights (the layout of
    // vit_wt, 2 bytes per element): made by the first bf16 forward after a parameter upload, never on a plan without the flag
    bool bf16_enabled = false;
    unsigned short* d_wbf = nullptr;
    bool wbf_valid = false;
    // the position table resampled to this plan's grid, [P + 1][D] (vit_pos_resample_kernel): made by the first forward after a
    // parameter upload, never on a plan whose grid is the checkpoint's (side 224)
    float* d_pos_rs = nullptr;
    bool pos_rs_valid = false;
    void invalidate() { finalized = false, wt_valid = false, wbf_valid = false, pos_rs_valid = false; }

    const float* p(size_t off) const { return off == VIT_ABSENT ? nullptr : pool.d_pool + off; }
};

namespace {

// one buffer layout for both directions: the token stream (forward) or the gradient stream (backward) [M][D], a D-wide and a
// 4D-wide scratch, and for the backward the LayerNorm partial sums behind them
struct VitWs {
    size_t x, h, big, partial, total;
};
VitWs vit_ws(const orbit_vit* v, int B, bool backward) {
    const size_t M = (size_t)B * v->N;
    VitWs L;
    L.x = 0;
    L.h = align_up(M * v->D * sizeof(float), 256);
    L.big = L.h + align_up(M * v->D * sizeof(float), 256);
    L.partial = L.big + align_up(M * v->mlp * sizeof(float), 256);
    L.total = L.partial + (backward ? align_up(layernorm_bwd_partial_floats((int)M, v->D) * sizeof(float), 256) : 0);
    return L;
}

// orbit_vit_backward_params: the frozen backward's buffers, one more D-wide buffer (the recomputed X operand of a weight
// gradient: h is busy holding dh) and the partial tiles of the largest split weight-gradient GEMM
struct VitWsParams {
    size_t x, h, h2, big, partial, wgrad, total;
};
VitWsParams vit_ws_params(const orbit_vit* v, int B) {
    const int M = B * v->N, D = v->D;
    const size_t md = align_up((size_t)M * D * sizeof(float), 256);
    size_t wg = wgrad_ws_floats(B * v->P, D, v->kpatch);
    const int shapes[4][2] = {{D, 4 * D}, {4 * D, D}, {D, D}, {3 * D, D}};  // (N, K) of fc2, fc1, proj, qkv
    for (const auto& nk : shapes) wg = std::max(wg, wgrad_ws_floats(M, nk[0], nk[1]));
    VitWsParams L;
    L.x = 0, L.h = md, L.h2 = 2 * md, L.big = 3 * md;
    L.partial = L.big + align_up((size_t)M * v->mlp * sizeof(float), 256);
    L.wgrad = L.partial + align_up(layernorm_bwd_partial_floats(M, D) * sizeof(float), 256);
    L.total = L.wgrad + align_up(wg * sizeof(float), 256);
    return L;
}

// tape of a taped forward: per block the input x [M][D], qkv [M][3D], the post-attention stream x_mid [M][D] and the fc1
// pre-activation u [M][4D] (9 M D floats), then the stream entering the final norm [M][D]. LayerNorm statistics are recomputed.
struct VitTape {
    size_t x, qkv, mid, u, block, last, total;  // byte offsets inside a block, block stride, the final stream, size
};
VitTape vit_tape(const orbit_vit* v, int B) {
    const size_t md = align_up((size_t)B * v->N * v->D * sizeof(float), 256);
    VitTape T;
    T.x = 0, T.qkv = md, T.mid = 4 * md, T.u = 5 * md, T.block = 9 * md;
    T.last = VIT_DEPTH * T.block;
    T.total = T.last + md;
    return T;
}

// the transposed weights of one block inside d_wt: qkv^T [D][3D], proj^T [D][D], fc1^T [D][4D], fc2^T [4D][D] (float offsets)
struct VitWt {
    size_t qkv, proj, fc1, fc2, block;
};
VitWt vit_wt(const orbit_vit* v) {
    const size_t DD = (size_t)v->D * v->D;
    return {0, 3 * DD, 4 * DD, 8 * DD, 12 * DD};
}

// what the three whole-network entry points refuse alike (their own null pointers are checked before, with the same text)
int vit_check_call(const char* who, const orbit_vit* v, int B, const float* film_gamma, const float* film_beta) {
    ORBIT_REQUIRE(v, "%s: null pointer", who);
    ORBIT_REQUIRE(B > 0 && B <= v->max_b, "%s: batch of %d frames (1..%d)", who, B, v->max_b);
    if (!v->finalized) return set_err(ORBIT_ERR_STATE, "%s: call orbit_vit_finalize first", who);
    ORBIT_REQUIRE((film_gamma == nullptr) == (film_beta == nullptr), "%s: film_gamma and film_beta must be given together", who);
    return ORBIT_OK;
}
// a plan of orbit_vit_create_sized at another frame size has no training path at all
int vit_check_frame_size(const char* who, const orbit_vit* v) {
    ORBIT_REQUIRE(!v->sized(), "%s: %s is a %dx%d plan (orbit_vit_create_sized): frame size %d is inference + FiLM only, the "
                  "training paths run on %dx%d frames", who, v->name.c_str(), v->side, v->side, v->side, VIT_SIZE, VIT_SIZE);
    return ORBIT_OK;
}
// the training entry points on a forward-only plan: refused by name, before any launch or allocation
int vit_check_trainable(const char* who, const orbit_vit* v) {
    ORBIT_REQUIRE(v, "%s: null pointer", who);
    if (int rc = vit_check_frame_size(who, v)) return rc;
    ORBIT_REQUIRE(!v->bf16_enabled, "%s: %s is a bf16 inference plan (orbit_vit_enable_bf16): the training paths are fp32 only", who,
                  v->name.c_str());
    ORBIT_REQUIRE(!v->forward_only(), "%s: %s is an inference-only plan (no tape and no backward for the patch-%d models)", who,
                  v->name.c_str(), v->patch);
    return ORBIT_OK;
}
int vit_check_buffer(const char* who, const char* what, const void* ptr, size_t bytes, size_t need) {
    ORBIT_REQUIRE(bytes >= need, "%s: %s too small (%zu < %zu bytes)", who, what, bytes, need);
    ORBIT_REQUIRE(((uintptr_t)ptr & 255) == 0, "%s: %s must be 256-byte aligned", who, what);
    return ORBIT_OK;
}

// any_size false: orbit_vit_create (224 x 224, or its refusal); true: orbit_vit_create_sized (square, a multiple of the patch,
// 32..512). At 224 x 224 the two build the same plan.
constexpr int VIT_SIZED_MIN = 32, VIT_SIZED_MAX = 512;
int vit_create_impl(const char* who, const char* name, int H, int W, bool any_size, orbit_vit_t** out) {
    ORBIT_REQUIRE(name && out, "%s: null pointer", who);
    std::string n(name);
    int D, heads;
    bool clip = false, p16 = false;
    if (n == "vit_s_32") D = 384, heads = 6;
    else if (n == "vit_b_32") D = 768, heads = 12;
    else if (n == "vit_b_32_clip") D = 768, heads = 12, clip = true;
    else if (n == "vit_s_16") D = 384, heads = 6, p16 = true;
    else if (n == "vit_b_16") D = 768, heads = 12, p16 = true;
    else if (n == "vit_b_16_clip") D = 768, heads = 12, clip = true, p16 = true;
    else return set_err(ORBIT_ERR_ARG, "Invalid feature_extractor_name: %s (transformer extractors: vit_s_32, vit_b_32, "
                        "vit_b_32_clip, vit_s_16, vit_b_16, vit_b_16_clip)", name);
    const int patch = p16 ? VIT16_PATCH : VIT_PATCH;
    if (!any_size) {
        ORBIT_REQUIRE(H == VIT_SIZE && W == VIT_SIZE, "vit_create: %s runs on %dx%d frames only (fixed position table), got %dx%d",
                      name, VIT_SIZE, VIT_SIZE, H, W);
    } else {
        ORBIT_REQUIRE(H == W, "%s: %s runs on square frames only, got %dx%d", who, name, H, W);
        ORBIT_REQUIRE(H >= VIT_SIZED_MIN, "%s: frame size %d is below %d", who, H, VIT_SIZED_MIN);
        ORBIT_REQUIRE(H <= VIT_SIZED_MAX, "%s: frame size %d is above %d", who, H, VIT_SIZED_MAX);
        ORBIT_REQUIRE(H % patch == 0, "%s: frame size %d is not a multiple of %s's patch size %d (nearest: %d and %d)", who, H, name,
                      patch, H / patch * patch, (H / patch + 1) * patch);
    }
    orbit_vit* v = new orbit_vit();
    v->name = n, v->pool.owner = n, v->D = D, v->heads = heads, v->mlp = 4 * D, v->clip = clip, v->eps = clip ? 1e-5f : 1e-6f;
    if (p16) {
        v->patch = VIT16_PATCH, v->grid = VIT_SIZE / v->patch, v->P = v->grid * v->grid, v->N = v->P + 1;
        v->kpatch = 3 * v->patch * v->patch, v->max_b = VIT16_MAX_B;
    }
    auto add = [&](const std::string& key, size_t numel) { return v->pool.off(v->pool.add(key, numel)); };
    // timm 0.6.12 VisionTransformer state_dict order
    v->cls = add("cls_token", D);
    v->pos = add("pos_embed", (size_t)v->N * D);  // (the checkpoint's shape at any frame size)
    if (H != VIT_SIZE) {
        // another frame size: the same parameters, the geometry of S / patch patches per side, and as many frames as keep the
        // token rows within what the caps at 224 already allow (workspace sizes stay in that range)
        v->side = H, v->grid = H / patch, v->P = v->grid * v->grid, v->N = v->P + 1;
        v->max_b = VIT_MAX_B * VIT_N / v->N;
    }
    v->patch_w = add("patch_embed.proj.weight", (size_t)D * v->kpatch);
    if (!clip) v->patch_b = add("patch_embed.proj.bias", D);
    if (clip) v->pre_w = add("norm_pre.weight", D), v->pre_b = add("norm_pre.bias", D);
    for (int i = 0; i < VIT_DEPTH; ++i) {
        const std::string b = "blocks." + std::to_string(i);
        VitBlock& k = v->blk[i];
        k.norm1_w = add(b + ".norm1.weight", D), k.norm1_b = add(b + ".norm1.bias", D);
        k.qkv_w = add(b + ".attn.qkv.weight", (size_t)3 * D * D), k.qkv_b = add(b + ".attn.qkv.bias", 3 * D);
        k.proj_w = add(b + ".attn.proj.weight", (size_t)D * D), k.proj_b = add(b + ".attn.proj.bias", D);
        k.norm2_w = add(b + ".norm2.weight", D), k.norm2_b = add(b + ".norm2.bias", D);
        k.fc1_w = add(b + ".mlp.fc1.weight", (size_t)4 * D * D), k.fc1_b = add(b + ".mlp.fc1.bias", 4 * D);
        k.fc2_w = add(b + ".mlp.fc2.weight", (size_t)4 * D * D), k.fc2_b = add(b + ".mlp.fc2.bias", D);
        v->film_names.push_back(b + ".norm1");
        v->film_names.push_back(b + ".norm2");
    }
    v->norm_w = add("norm.weight", D), v->norm_b = add("norm.bias", D);
    v->film_names.push_back("norm");
    const double Dd = D;
    v->macs = (double)v->P * v->kpatch * Dd + VIT_DEPTH * (v->N * 12.0 * Dd * Dd + 2.0 * v->N * v->N * Dd);
    *out = v;
    return ORBIT_OK;
}

}  // namespace

extern "C" {

int orbit_vit_create(const char* name, int H, int W, orbit_vit_t** out) {
    return vit_create_impl("vit_create", name, H, W, false, out);
}

int orbit_vit_create_sized(const char* name, int H, int W, orbit_vit_t** out) {
    return vit_create_impl("vit_create_sized", name, H, W, true, out);
}

void orbit_vit_destroy(orbit_vit_t* v) {
    if (!v) return;
    v->pool.free_device();
    (void)hipFree(v->d_wt);
    (void)hipFree(v->d_wbf);
    (void)hipFree(v->d_pos_rs);
    delete v;
}

int orbit_vit_num_params(const orbit_vit_t* v) { return v ? v->pool.size() : 0; }
const char* orbit_vit_param_name(const orbit_vit_t* v, int i) { return v ? v->pool.name(i) : nullptr; }
size_t orbit_vit_param_numel(const orbit_vit_t* v, int i) { return v ? v->pool.numel(i) : 0; }

// every upload invalidates the finalized state, the transposed weights of the backward, the bf16 copies and the resampled table
int orbit_vit_load(orbit_vit_t* v, const char* key, const float* data, size_t numel) {
    ORBIT_REQUIRE(v && key && data, "vit_load: null pointer");
    if (int rc = v->pool.load("vit_load", key, data, numel)) return rc;
    v->invalidate();
    return ORBIT_OK;
}

int orbit_vit_load_async(orbit_vit_t* v, const char* key, const float* device_data, size_t numel, orbit_stream_t stream) {
    ORBIT_REQUIRE(v && key && device_data, "vit_load_async: null pointer");
    if (int rc = v->pool.load_async("vit_load_async", key, device_data, numel, (hipStream_t)stream)) return rc;
    v->invalidate();
    return ORBIT_OK;
}

int orbit_vit_load_all_async(orbit_vit_t* v, const float* const* device_ptrs, int n, orbit_stream_t stream) {
    ORBIT_REQUIRE(v && device_ptrs, "vit_load_all_async: null pointer");
    if (int rc = v->pool.load_all_async("vit_load_all_async", device_ptrs, n, 32, (hipStream_t)stream)) return rc;
    v->invalidate();
    return ORBIT_OK;
}

int orbit_vit_finalize(orbit_vit_t* v, orbit_stream_t stream) {
    (void)stream;  // the kernels read the torch layouts as loaded: nothing to repack
    ORBIT_REQUIRE(v, "vit_finalize: null pointer");
    const char* missing = nullptr;
    ORBIT_REQUIRE(v->pool.all_loaded(&missing), "vit_finalize: parameter '%s' was never loaded", missing);
    v->finalized = true;
    return ORBIT_OK;
}

int orbit_vit_output_size(const orbit_vit_t* v) { return v ? v->D : 0; }
int orbit_vit_film_slots(const orbit_vit_t* v) { return v ? (int)v->film_names.size() : 0; }
int orbit_vit_film_slot_channels(const orbit_vit_t* v, int slot) {
    return (v && slot >= 0 && slot < (int)v->film_names.size()) ? v->D : 0;
}
const char* orbit_vit_film_slot_name(const orbit_vit_t* v, int slot) {
    return (v && slot >= 0 && slot < (int)v->film_names.size()) ? v->film_names[slot].c_str() : nullptr;
}
int orbit_vit_film_size(const orbit_vit_t* v) { return v ? (int)v->film_names.size() * v->D : 0; }
size_t orbit_vit_workspace_bytes(const orbit_vit_t* v, int B) {
    if (!v || B <= 0 || B > v->max_b) return 0;
    return vit_ws(v, B, false).total;
}
double orbit_vit_macs_per_frame(const orbit_vit_t* v) { return v ? v->macs : 0.0; }

}  // extern "C"

namespace {

// the forward. tape == nullptr: inference, the stream is updated in place inside the workspace. With a tape the same kernels in
// the same order write what the backward reads straight into it (each residual GEMM reads one tape slot and writes the next),
// and fc1 stores its pre-activation beside GELU(u) (EPI_GELU_TAPE): the features are bitwise those of the inference forward.
// (re)build the bf16 weight copies on `s` if a parameter upload invalidated them
int vit_ensure_wbf(orbit_vit_t* v, hipStream_t s) {
    const VitWt W = vit_wt(v);
    const size_t DD = (size_t)v->D * v->D;
    if (!v->d_wbf) ORBIT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&v->d_wbf), VIT_DEPTH * W.block * sizeof(unsigned short)));
    if (v->wbf_valid) return ORBIT_OK;
    int rc;
    for (int i = 0; i < VIT_DEPTH; ++i) {
        const VitBlock& k = v->blk[i];
        unsigned short* wb = v->d_wbf + i * W.block;
        if ((rc = launch_pack_bf16(v->p(k.qkv_w), wb + W.qkv, 3 * DD, s))) return rc;
        if ((rc = launch_pack_bf16(v->p(k.proj_w), wb + W.proj, DD, s))) return rc;
        if ((rc = launch_pack_bf16(v->p(k.fc1_w), wb + W.fc1, 4 * DD, s))) return rc;
        if ((rc = launch_pack_bf16(v->p(k.fc2_w), wb + W.fc2, 4 * DD, s))) return rc;
    }
    v->wbf_valid = true;
    return ORBIT_OK;
}

// (re)build the resampled position table on `s` if a parameter upload invalidated it (plans at another grid than the checkpoint's)
int vit_ensure_pos(orbit_vit_t* v, hipStream_t s) {
    if (!v->sized()) return ORBIT_OK;
    if (!v->d_pos_rs) ORBIT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&v->d_pos_rs), (size_t)v->N * v->D * sizeof(float)));
    if (v->pos_rs_valid) return ORBIT_OK;
    if (int rc = launch_pos_resample(v->p(v->pos), v->d_pos_rs, VIT_SIZE / v->patch, v->grid, v->D, s)) return rc;
    v->pos_rs_valid = true;
    return ORBIT_OK;
}

// With bf16 (a plan under orbit_vit_enable_bf16, tape == nullptr) the four token GEMMs of every block run on vit_gemm_bf16_kernel;
// everything else, the residual stream included, is the fp32 kernels in the same buffers.
int vit_forward_impl(orbit_vit_t* v, const float* frames, int B, const float* film_gamma, const float* film_beta, float* feats,
                     void* workspace, char* tape, hipStream_t s) {
    const bool bf16 = v->bf16_enabled;
    if (bf16 && tape) return set_err(ORBIT_ERR_ARG, "vit_forward: a bf16 plan (orbit_vit_enable_bf16) has no taped forward");
    const VitWt W = vit_wt(v);
    if (bf16)
        if (int rc = vit_ensure_wbf(v, s)) return rc;
    if (v->sized() && tape) return set_err(ORBIT_ERR_ARG, "vit_forward: a %dx%d plan has no taped forward", v->side, v->side);
    if (int rc = vit_ensure_pos(v, s)) return rc;
    const float* pos = v->sized() ? v->d_pos_rs : v->p(v->pos);  // [N][D]
    const VitWs L = vit_ws(v, B, false);
    const VitTape T = vit_tape(v, B);
    const int D = v->D, N = v->N, M = B * N;
    char* ws = static_cast<char*>(workspace);
    auto slot = [&](int i, size_t off) { return reinterpret_cast<float*>(tape + (i < VIT_DEPTH ? i * T.block + off : T.last)); };
    float* x = tape ? slot(0, T.x) : reinterpret_cast<float*>(ws + L.x);
    float* h = reinterpret_cast<float*>(ws + L.h);
    float* big = reinterpret_cast<float*>(ws + L.big);
    // LayerNorm of FiLM slot `slot`: the per-task vectors when given, else the module's own weight / bias
    auto ln_params = [&](size_t w, size_t b, int slot, const float** g, const float** be) {
        if (film_gamma) *g = film_gamma + (size_t)slot * D, *be = film_beta + (size_t)slot * D;
        else *g = v->p(w), *be = v->p(b);
    };
    int rc;
    {   // tokens: patch embedding (+ bias) + pos_embed into rows 1..N-1, cls_token + pos_embed[0] into row 0
        GemmArgs a{frames, v->p(v->patch_w), v->p(v->patch_b), nullptr, pos, x, B * v->P, D, v->kpatch};
        if (v->sized()) {  // (a 224 plan keeps its compile-time geometry)
            a.side = v->side, a.grid = v->grid;
            rc = v->patch == VIT16_PATCH ? launch_gemm<EPI_PATCH16_RT>(a, "patch_embed_sized", s)
                                         : launch_gemm<EPI_PATCH_RT>(a, "patch_embed_sized", s);
        } else {
            rc = v->patch == VIT16_PATCH ? launch_gemm<EPI_PATCH16>(a, "patch_embed", s) : launch_gemm<EPI_PATCH>(a, "patch_embed", s);
        }
        if (rc) return rc;
        if ((rc = launch_cls_token(v->p(v->cls), pos, x, B, D, N, s))) return rc;
        if (v->clip && (rc = launch_layernorm(x, D, x, D, M, D, v->p(v->pre_w), v->p(v->pre_b), v->eps, s))) return rc;
    }
    for (int i = 0; i < VIT_DEPTH; ++i) {
        const VitBlock& k = v->blk[i];
        float* qkvb = tape ? slot(i, T.qkv) : big;
        float* xmid = tape ? slot(i, T.mid) : x;
        float* xout = tape ? slot(i + 1, T.x) : x;
        const float *g, *be;
        ln_params(k.norm1_w, k.norm1_b, 2 * i, &g, &be);
        if ((rc = launch_layernorm(x, D, h, D, M, D, g, be, v->eps, s))) return rc;
        if (bf16) {
            const unsigned short* wb = v->d_wbf + i * W.block;
            if ((rc = launch_gemm_bf16<EPI_BIAS>({h, wb + W.qkv, v->p(k.qkv_b), nullptr, big, M, 3 * D, D}, "qkv", s))) return rc;
            if ((rc = launch_attention(big, h, B, N, D, v->heads, s))) return rc;
            if ((rc = launch_gemm_bf16<EPI_RESIDUAL>({h, wb + W.proj, v->p(k.proj_b), x, x, M, D, D}, "proj", s))) return rc;
            ln_params(k.norm2_w, k.norm2_b, 2 * i + 1, &g, &be);
            if ((rc = launch_layernorm(x, D, h, D, M, D, g, be, v->eps, s))) return rc;
            if ((rc = launch_gemm_bf16<EPI_GELU>({h, wb + W.fc1, v->p(k.fc1_b), nullptr, big, M, 4 * D, D}, "fc1", s))) return rc;
            if ((rc = launch_gemm_bf16<EPI_RESIDUAL>({big, wb + W.fc2, v->p(k.fc2_b), x, x, M, D, 4 * D}, "fc2", s))) return rc;
            continue;
        }
        GemmArgs qkv{h, v->p(k.qkv_w), v->p(k.qkv_b), nullptr, nullptr, qkvb, M, 3 * D, D};
        if ((rc = launch_gemm<EPI_BIAS>(qkv, "qkv", s))) return rc;
        if ((rc = launch_attention(qkvb, h, B, N, D, v->heads, s))) return rc;
        GemmArgs proj{h, v->p(k.proj_w), v->p(k.proj_b), x, nullptr, xmid, M, D, D};
        if ((rc = launch_gemm<EPI_RESIDUAL>(proj, "proj", s))) return rc;
        ln_params(k.norm2_w, k.norm2_b, 2 * i + 1, &g, &be);
        if ((rc = launch_layernorm(xmid, D, h, D, M, D, g, be, v->eps, s))) return rc;
        GemmArgs fc1{h, v->p(k.fc1_w), v->p(k.fc1_b), nullptr, nullptr, big, M, 4 * D, D};
        if (tape) {
            fc1.aux = slot(i, T.u);
            if ((rc = launch_gemm<EPI_GELU_TAPE>(fc1, "fc1", s))) return rc;
        } else if ((rc = launch_gemm<EPI_GELU>(fc1, "fc1", s))) {
            return rc;
        }
        GemmArgs fc2{big, v->p(k.fc2_w), v->p(k.fc2_b), xmid, nullptr, xout, M, D, 4 * D};
        if ((rc = launch_gemm<EPI_RESIDUAL>(fc2, "fc2", s))) return rc;
        x = xout;
    }
    const float *g, *be;
    ln_params(v->norm_w, v->norm_b, 2 * VIT_DEPTH, &g, &be);
    // final LayerNorm on the class token of every frame, straight into the caller's feature rows
    return launch_layernorm(x, (size_t)N * D, feats, D, B, D, g, be, v->eps, s);
}

// (re)build the transposed weights on `s` if a parameter upload invalidated them
int vit_ensure_wt(orbit_vit_t* v, hipStream_t s) {
    const VitWt W = vit_wt(v);
    const int D = v->D;
    if (!v->d_wt) ORBIT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&v->d_wt), VIT_DEPTH * W.block * sizeof(float)));
    if (v->wt_valid) return ORBIT_OK;
    int rc;
    for (int i = 0; i < VIT_DEPTH; ++i) {
        const VitBlock& k = v->blk[i];
        float* wt = v->d_wt + i * W.block;
        if ((rc = vit_transpose(v->p(k.qkv_w), wt + W.qkv, 3 * D, D, s))) return rc;
        if ((rc = vit_transpose(v->p(k.proj_w), wt + W.proj, D, D, s))) return rc;
        if ((rc = vit_transpose(v->p(k.fc1_w), wt + W.fc1, 4 * D, D, s))) return rc;
        if ((rc = vit_transpose(v->p(k.fc2_w), wt + W.fc2, D, 4 * D, s))) return rc;
    }
    v->wt_valid = true;
    return ORBIT_OK;
}

// the buffers of a reverse pass inside the caller's workspace; h2 and wgrad only with parameter gradients
struct VitBwdBuffers {
    float *dx, *h, *h2, *big, *partial, *wgrad;
};

// The reverse pass. pg == nullptr: the FiLM gradients of the frozen network (orbit_vit_backward). With pg, the flat parameter
// gradient buffer (pool offsets), the same kernels in the same order compute the same dgamma / dbeta, and between them every
// Linear layer's weight / bias gradient is taken from its dY and its X operand - on the tape (fc2: GELU of the pre-activation,
// on load) or recomputed into h2 by the forward's kernel (LN2(x_mid) for fc1, attention(qkv) for proj, LN1(x) for qkv); block
// 0's norm1 then hands its data gradient on to (CLIP) norm_pre and the token assembly.
int vit_backward_impl(orbit_vit_t* v, const float* frames, int B, const float* film_gamma, const float* film_beta,
                      const float* dfeats, const char* tp, float* pg, float* dgamma, float* dbeta, const VitBwdBuffers& b,
                      hipStream_t s) {
    int rc;
    if ((rc = vit_ensure_wt(v, s))) return rc;
    const VitWt W = vit_wt(v);
    const VitTape T = vit_tape(v, B);
    const int D = v->D, N = v->N, M = B * N;  // (M * 4 D < 2^31 up to max_b frames; every index below is size_t)
    float *dx = b.dx, *h = b.h, *h2 = b.h2, *big = b.big, *partial = b.partial;
    auto slot = [&](int i, size_t off) { return reinterpret_cast<const float*>(tp + i * T.block + off); };
    auto gamma_of = [&](size_t w, int sl) { return film_gamma ? film_gamma + (size_t)sl * D : v->p(w); };
    auto beta_of = [&](size_t w, int sl) { return film_beta ? film_beta + (size_t)sl * D : v->p(w); };
    // final norm: token 0 of every frame from dfeats; the other token rows of the gradient stream are exactly zero
    const int last = 2 * VIT_DEPTH;
    if ((rc = zero_gradient_stream(dx, (size_t)M * D, s))) return rc;
    if ((rc = launch_layernorm_bwd(reinterpret_cast<const float*>(tp + T.last), (size_t)N * D, dfeats, D, gamma_of(v->norm_w, last),
                                   v->eps, nullptr, dx, (size_t)N * D, B, D, partial, dgamma + (size_t)last * D,
                                   dbeta + (size_t)last * D, s)))
        return rc;
    for (int i = VIT_DEPTH - 1; i >= 0; --i) {
        const VitBlock& k = v->blk[i];
        const float* wt = v->d_wt + i * W.block;  // (vit_ensure_wt)
        // x_out = x_mid + fc2(GELU(u)):  du = (dx W2) o GELU'(u),  dh = du W1,  dx += LN2'(dh)
        if (pg && (rc = launch_wgrad<WX_GELU>(dx, slot(i, T.u), pg + k.fc2_w, pg + k.fc2_b, M, D, 4 * D, b.wgrad, "wgrad_fc2", s)))
            return rc;
        GemmArgs dfc2{dx, wt + W.fc2, nullptr, slot(i, T.u), nullptr, big, M, 4 * D, D};
        if ((rc = launch_gemm<EPI_DGELU, true>(dfc2, "dgrad_fc2", s))) return rc;
        int sl = 2 * i + 1;
        if (pg) {
            if ((rc = launch_layernorm(slot(i, T.mid), D, h2, D, M, D, gamma_of(k.norm2_w, sl), beta_of(k.norm2_b, sl), v->eps, s)))
                return rc;
            if ((rc = launch_wgrad<WX_PLAIN>(big, h2, pg + k.fc1_w, pg + k.fc1_b, M, 4 * D, D, b.wgrad, "wgrad_fc1", s))) return rc;
        }
        GemmArgs dfc1{big, wt + W.fc1, nullptr, nullptr, nullptr, h, M, D, 4 * D};
        if ((rc = launch_gemm<EPI_BIAS, true>(dfc1, "dgrad_fc1", s))) return rc;
        if ((rc = launch_layernorm_bwd(slot(i, T.mid), D, h, D, gamma_of(k.norm2_w, sl), v->eps, dx, dx, D, M, D, partial,
                                       dgamma + (size_t)sl * D, dbeta + (size_t)sl * D, s)))
            return rc;
        // x_mid = x + proj(attn(qkv)):  dO = dx Wp,  dqkv = attn'(dO),  dh = dqkv Wqkv,  dx += LN1'(dh)
        if (pg) {
            if ((rc = launch_attention(slot(i, T.qkv), h2, B, N, D, v->heads, s))) return rc;
            if ((rc = launch_wgrad<WX_PLAIN>(dx, h2, pg + k.proj_w, pg + k.proj_b, M, D, D, b.wgrad, "wgrad_proj", s))) return rc;
        }
        GemmArgs dproj{dx, wt + W.proj, nullptr, nullptr, nullptr, h, M, D, D};
        if ((rc = launch_gemm<EPI_BIAS, true>(dproj, "dgrad_proj", s))) return rc;
        if ((rc = launch_attention_bwd(slot(i, T.qkv), h, big, B, N, D, v->heads, s))) return rc;
        sl = 2 * i;
        if (pg) {
            if ((rc = launch_layernorm(slot(i, T.x), D, h2, D, M, D, gamma_of(k.norm1_w, sl), beta_of(k.norm1_b, sl), v->eps, s)))
                return rc;
            if ((rc = launch_wgrad<WX_PLAIN>(big, h2, pg + k.qkv_w, pg + k.qkv_b, M, 3 * D, D, b.wgrad, "wgrad_qkv", s))) return rc;
        }
        GemmArgs dqkv{big, wt + W.qkv, nullptr, nullptr, nullptr, h, M, D, 3 * D};
        if ((rc = launch_gemm<EPI_BIAS, true>(dqkv, "dgrad_qkv", s))) return rc;
        // (block 0 of the frozen network: nothing upstream of its norm1 takes a gradient)
        if ((rc = launch_layernorm_bwd(slot(i, T.x), D, h, D, gamma_of(k.norm1_w, sl), v->eps, dx, i > 0 || pg ? dx : nullptr, D, M,
                                       D, partial, dgamma + (size_t)sl * D, dbeta + (size_t)sl * D, s)))
            return rc;
    }
    if (!pg) return ORBIT_OK;
    const float* dx0 = dx;
    if (v->clip) {
        // norm_pre ran in place: its input tokens are rebuilt from the frames (patch GEMM + class-token row) into h2
        GemmArgs a{frames, v->p(v->patch_w), v->p(v->patch_b), nullptr, v->p(v->pos), h2, B * v->P, D, v->kpatch};
        if ((rc = v->patch == VIT16_PATCH ? launch_gemm<EPI_PATCH16>(a, "patch_embed", s) : launch_gemm<EPI_PATCH>(a, "patch_embed", s)))
            return rc;
        if ((rc = launch_cls_token(v->p(v->cls), v->p(v->pos), h2, B, D, N, s))) return rc;
        if ((rc = launch_layernorm_bwd(h2, D, dx, D, v->p(v->pre_w), v->eps, nullptr, h, D, M, D, partial, pg + v->pre_w,
                                       pg + v->pre_b, s)))
            return rc;
        dx0 = h;
    }
    return launch_patch_embed_bwd(frames, dx0, pg + v->patch_w, v->patch_b == VIT_ABSENT ? nullptr : pg + v->patch_b, pg + v->pos,
                                  pg + v->cls, B, D, v->patch, b.wgrad, s);
}

}  // namespace

extern "C" {

int orbit_vit_forward(orbit_vit_t* v, const float* frames, int B, const float* film_gamma, const float* film_beta,
                      float* feats, void* workspace, size_t workspace_bytes, orbit_stream_t stream) {
    const char* who = "vit_forward";
    ORBIT_REQUIRE(frames && feats && workspace, "%s: null pointer", who);
    if (int rc = vit_check_call(who, v, B, film_gamma, film_beta)) return rc;
    if (int rc = vit_check_buffer(who, "workspace", workspace, workspace_bytes, vit_ws(v, B, false).total)) return rc;
    ORBIT_REQUIRE(((uintptr_t)frames & 15) == 0, "%s: frames must be 16-byte aligned", who);
    return vit_forward_impl(v, frames, B, film_gamma, film_beta, feats, workspace, nullptr, (hipStream_t)stream);
}

// ---- FiLM gradients of the frozen network ----------------------------------------------------------------------------
// opt-in bf16 token GEMMs (inference only): a flag on this plan, nothing is allocated here
int orbit_vit_enable_bf16(orbit_vit_t* v) {
    ORBIT_REQUIRE(v, "vit_enable_bf16: null pointer");
    ORBIT_REQUIRE(!v->backward_enabled && !v->weight_backward_enabled, "vit_enable_bf16: %s has orbit_vit_enable_backward / "
                  "orbit_vit_enable_weight_backward set; bf16 is an inference mode (the training paths are fp32 only)", v->name.c_str());
    v->bf16_enabled = true;
    return ORBIT_OK;
}
int orbit_vit_bf16_enabled(const orbit_vit_t* v) { return v && v->bf16_enabled ? 1 : 0; }

int orbit_vit_enable_backward(orbit_vit_t* v) {
    ORBIT_REQUIRE(v, "vit_enable_backward: null pointer");
    if (int rc = vit_check_frame_size("vit_enable_backward", v)) return rc;
    ORBIT_REQUIRE(!v->bf16_enabled, "vit_enable_backward: %s is a bf16 inference plan (orbit_vit_enable_bf16)", v->name.c_str());
    v->backward_enabled = true;  // (read by forward_only() of the patch-16 plans only)
    return ORBIT_OK;
}
// weight gradients of a patch-16 plan (orbit_vit_backward_params); a patch-32 plan has them already
int orbit_vit_enable_weight_backward(orbit_vit_t* v) {
    ORBIT_REQUIRE(v, "vit_enable_weight_backward: null pointer");
    if (int rc = vit_check_frame_size("vit_enable_weight_backward", v)) return rc;
    ORBIT_REQUIRE(!v->bf16_enabled, "vit_enable_weight_backward: %s is a bf16 inference plan (orbit_vit_enable_bf16)",
                  v->name.c_str());
    v->weight_backward_enabled = true;  // (a patch-32 plan has the gradients anyway: remembered for orbit_vit_enable_bf16's refusal)
    if (v->patch == VIT_PATCH) return ORBIT_OK;
    v->backward_enabled = true;
    return ORBIT_OK;
}
size_t orbit_vit_tape_bytes(const orbit_vit_t* v, int B) {
    if (!v || v->forward_only() || B <= 0 || B > v->max_b) return 0;
    return vit_tape(v, B).total;
}
size_t orbit_vit_backward_workspace_bytes(const orbit_vit_t* v, int B) {
    if (!v || v->forward_only() || B <= 0 || B > v->max_b) return 0;
    return vit_ws(v, B, true).total;
}

int orbit_vit_train_forward(orbit_vit_t* v, const float* frames, int B, const float* film_gamma, const float* film_beta,
                            float* feats, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes,
                            orbit_stream_t stream) {
    const char* who = "vit_train_forward";
    ORBIT_REQUIRE(frames && feats && tape && workspace, "%s: null pointer", who);
    if (int rc = vit_check_trainable(who, v)) return rc;  // (before the state checks: a refusal needs no loaded plan)
    if (int rc = vit_check_call(who, v, B, film_gamma, film_beta)) return rc;
    if (int rc = vit_check_buffer(who, "workspace", workspace, workspace_bytes, vit_ws(v, B, false).total)) return rc;
    if (int rc = vit_check_buffer(who, "tape", tape, tape_bytes, vit_tape(v, B).total)) return rc;
    ORBIT_REQUIRE(((uintptr_t)frames & 15) == 0, "%s: frames must be 16-byte aligned", who);
    return vit_forward_impl(v, frames, B, film_gamma, film_beta, feats, workspace, static_cast<char*>(tape), (hipStream_t)stream);
}

int orbit_vit_backward(orbit_vit_t* v, int B, const float* film_gamma, const float* film_beta, const float* dfeats,
                       const void* tape, size_t tape_bytes, float* dgamma, float* dbeta, void* workspace,
                       size_t workspace_bytes, orbit_stream_t stream) {
    const char* who = "vit_backward";
    ORBIT_REQUIRE(dfeats && tape && dgamma && dbeta && workspace, "%s: null pointer", who);
    if (int rc = vit_check_trainable(who, v)) return rc;  // (before the state checks: a refusal needs no loaded plan)
    if (int rc = vit_check_call(who, v, B, film_gamma, film_beta)) return rc;
    const VitWs L = vit_ws(v, B, true);
    if (int rc = vit_check_buffer(who, "workspace", workspace, workspace_bytes, L.total)) return rc;
    if (int rc = vit_check_buffer(who, "tape", tape, tape_bytes, vit_tape(v, B).total)) return rc;
    ORBIT_REQUIRE((((uintptr_t)dfeats | (uintptr_t)dgamma | (uintptr_t)dbeta | (uintptr_t)film_gamma) & 3) == 0,
                  "%s: dfeats, dgamma, dbeta and film_gamma must be 4-byte aligned", who);
    char* ws = static_cast<char*>(workspace);
    const VitBwdBuffers b{reinterpret_cast<float*>(ws + L.x), reinterpret_cast<float*>(ws + L.h), nullptr,
                          reinterpret_cast<float*>(ws + L.big), reinterpret_cast<float*>(ws + L.partial), nullptr};
    return vit_backward_impl(v, nullptr, B, film_gamma, film_beta, dfeats, static_cast<const char*>(tape), nullptr, dgamma, dbeta,
                             b, (hipStream_t)stream);
}

// ---- gradients of every parameter --------------------------------------------------------------------------------------
size_t orbit_vit_grad_floats(const orbit_vit_t* v) { return v ? v->pool.pool_floats : 0; }
size_t orbit_vit_param_offset(const orbit_vit_t* v, int i) { return (v && i >= 0 && i < v->pool.size()) ? v->pool.off(i) : 0; }
size_t orbit_vit_backward_params_workspace_bytes(const orbit_vit_t* v, int B) {
    if (!v || v->forward_only() || !v->weight_grads() || B <= 0 || B > v->max_b) return 0;
    return vit_ws_params(v, B).total;
}

int orbit_vit_backward_params(orbit_vit_t* v, const float* frames, int B, const float* film_gamma, const float* film_beta,
                              const float* dfeats, const void* tape, size_t tape_bytes, float* param_grads, float* dgamma,
                              float* dbeta, void* workspace, size_t workspace_bytes, orbit_stream_t stream) {
    const char* who = "vit_backward_params";
    ORBIT_REQUIRE(frames && dfeats && tape && param_grads && dgamma && dbeta && workspace, "%s: null pointer", who);
    if (int rc = vit_check_trainable(who, v)) return rc;  // (before the state checks: a refusal needs no loaded plan)
    ORBIT_REQUIRE(v->weight_grads(), "%s: %s gives FiLM gradients through the frozen network only (weight gradients are not "
                  "built for the patch-%d models)", who, v->name.c_str(), v->patch);
    if (int rc = vit_check_call(who, v, B, film_gamma, film_beta)) return rc;
    const VitWsParams L = vit_ws_params(v, B);
    if (int rc = vit_check_buffer(who, "workspace", workspace, workspace_bytes, L.total)) return rc;
    if (int rc = vit_check_buffer(who, "tape", tape, tape_bytes, vit_tape(v, B).total)) return rc;
    ORBIT_REQUIRE(((uintptr_t)frames & 15) == 0, "%s: frames must be 16-byte aligned", who);
    ORBIT_REQUIRE(((uintptr_t)param_grads & 255) == 0, "%s: param_grads must be 256-byte aligned", who);
    ORBIT_REQUIRE((((uintptr_t)dfeats | (uintptr_t)dgamma | (uintptr_t)dbeta | (uintptr_t)film_gamma | (uintptr_t)film_beta) & 3) == 0,
                  "%s: dfeats, dgamma, dbeta and the film vectors must be 4-byte aligned", who);
    char* ws = static_cast<char*>(workspace);
    const VitBwdBuffers b{reinterpret_cast<float*>(ws + L.x), reinterpret_cast<float*>(ws + L.h), reinterpret_cast<float*>(ws + L.h2),
                          reinterpret_cast<float*>(ws + L.big), reinterpret_cast<float*>(ws + L.partial),
                          reinterpret_cast<float*>(ws + L.wgrad)};
    return vit_backward_impl(v, frames, B, film_gamma, film_beta, dfeats, static_cast<const char*>(tape), param_grads, dgamma,
                             dbeta, b, (hipStream_t)stream);
}

// ---- single operators (parity tests) ---------------------------------------------------------------------------------
// (tile_rows is validated by launch_gemm, before it launches)
int orbit_op_vit_linear(const float* x, const float* w, const float* bias, const float* residual, float* y, int M, int N,
                        int K, int epilogue, int tile_rows, orbit_stream_t stream) {
    ORBIT_REQUIRE(x && w && y, "op_vit_linear: null pointer");
    ORBIT_REQUIRE(M > 0 && M <= VIT_MAX_B * VIT_N && N > 0 && K > 0, "op_vit_linear: bad shape M=%d N=%d K=%d", M, N, K);
    ORBIT_REQUIRE(N % G_BN == 0 && K % G_BK == 0, "op_vit_linear: N must be a multiple of %d and K of %d, got N=%d K=%d", G_BN,
                  G_BK, N, K);
    ORBIT_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_GELU || epilogue == EPI_RESIDUAL,
                  "op_vit_linear: epilogue must be 0 (bias), 1 (erf-GELU) or 2 (residual), got %d", epilogue);
    ORBIT_REQUIRE((epilogue == EPI_RESIDUAL) == (residual != nullptr), "op_vit_linear: residual goes with epilogue 2 only");
    ORBIT_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0, "op_vit_linear: x and w must be 16-byte aligned");
    ORBIT_REQUIRE(((uintptr_t)y & 3) == 0 && ((uintptr_t)bias & 3) == 0 && ((uintptr_t)residual & 3) == 0,
                  "op_vit_linear: y, bias and residual must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const GemmArgs a{x, w, bias, residual, nullptr, y, M, N, K};
    if (epilogue == EPI_GELU) return launch_gemm<EPI_GELU>(a, "op_linear_gelu", s, tile_rows);
    if (epilogue == EPI_RESIDUAL) return launch_gemm<EPI_RESIDUAL>(a, "op_linear_residual", s, tile_rows);
    return launch_gemm<EPI_BIAS>(a, "op_linear", s, tile_rows);
}

int orbit_op_vit_pack_bf16(const float* w, uint16_t* out, size_t numel, orbit_stream_t stream) {
    ORBIT_REQUIRE(w && out, "op_vit_pack_bf16: null pointer");
    ORBIT_REQUIRE(numel > 0 && numel < ((size_t)1 << 40), "op_vit_pack_bf16: bad numel %zu", numel);
    ORBIT_REQUIRE(((uintptr_t)w & 3) == 0 && ((uintptr_t)out & 1) == 0, "op_vit_pack_bf16: w must be 4-byte and out 2-byte aligned");
    return launch_pack_bf16(w, out, numel, (hipStream_t)stream);
}

// the conventions of orbit_op_vit_linear; w_bf16 is [N][K] bf16 (orbit_op_vit_pack_bf16), K a multiple of 64
int orbit_op_vit_linear_bf16(const float* x, const uint16_t* w_bf16, const float* bias, const float* residual, float* y, int M,
                             int N, int K, int epilogue, int tile_rows, orbit_stream_t stream) {
    ORBIT_REQUIRE(x && w_bf16 && y, "op_vit_linear_bf16: null pointer");
    ORBIT_REQUIRE(M > 0 && M <= VIT_MAX_B * VIT_N && N > 0 && K > 0, "op_vit_linear_bf16: bad shape M=%d N=%d K=%d", M, N, K);
    ORBIT_REQUIRE(N % G_BN == 0 && K % GB_BK == 0, "op_vit_linear_bf16: N must be a multiple of %d and K of %d, got M=%d N=%d K=%d",
                  G_BN, GB_BK, M, N, K);
    ORBIT_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_GELU || epilogue == EPI_RESIDUAL,
                  "op_vit_linear_bf16: epilogue must be 0 (bias), 1 (erf-GELU) or 2 (residual), got %d", epilogue);
    ORBIT_REQUIRE((epilogue == EPI_RESIDUAL) == (residual != nullptr), "op_vit_linear_bf16: residual goes with epilogue 2 only");
    ORBIT_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w_bf16 & 15) == 0, "op_vit_linear_bf16: x and w_bf16 must be 16-byte aligned");
    ORBIT_REQUIRE(((uintptr_t)y & 3) == 0 && ((uintptr_t)bias & 3) == 0 && ((uintptr_t)residual & 3) == 0,
                  "op_vit_linear_bf16: y, bias and residual must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const GemmBf16Args a{x, w_bf16, bias, residual, y, M, N, K};
    if (epilogue == EPI_GELU) return launch_gemm_bf16<EPI_GELU>(a, "op_linear_gelu", s, tile_rows);
    if (epilogue == EPI_RESIDUAL) return launch_gemm_bf16<EPI_RESIDUAL>(a, "op_linear_residual", s, tile_rows);
    return launch_gemm_bf16<EPI_BIAS>(a, "op_linear", s, tile_rows);
}

// patch: 32 (7 x 7 patches, 50 token rows per frame) or 16 (14 x 14, 197)
int orbit_op_vit_patch_embed_p(const float* frames, const float* w, const float* bias_or_null, const float* pos_embed,
                               const float* cls_token, float* tokens, int B, int D, int patch, int tile_rows,
                               orbit_stream_t stream) {
    ORBIT_REQUIRE(frames && w && pos_embed && cls_token && tokens, "op_vit_patch_embed: null pointer");
    ORBIT_REQUIRE(patch == VIT_PATCH || patch == VIT16_PATCH, "op_vit_patch_embed: patch size %d (32 or 16)", patch);
    const bool p16 = patch == VIT16_PATCH;
    const int max_b = p16 ? VIT16_MAX_B : VIT_MAX_B;
    ORBIT_REQUIRE(B > 0 && B <= max_b, "op_vit_patch_embed: batch of %d frames (1..%d)", B, max_b);
    ORBIT_REQUIRE(D == 384 || D == 768, "op_vit_patch_embed: unsupported width %d (384 or 768)", D);
    ORBIT_REQUIRE(((uintptr_t)frames & 15) == 0 && ((uintptr_t)w & 15) == 0,
                  "op_vit_patch_embed: frames and w must be 16-byte aligned");
    ORBIT_REQUIRE(((uintptr_t)tokens & 3) == 0 && ((uintptr_t)bias_or_null & 3) == 0 && ((uintptr_t)pos_embed & 3) == 0 &&
                      ((uintptr_t)cls_token & 3) == 0,
                  "op_vit_patch_embed: tokens, bias, pos_embed and cls_token must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const GemmArgs a{frames, w, bias_or_null, nullptr, pos_embed, tokens, B * (p16 ? VIT16_P : VIT_P), D, p16 ? VIT16_KPATCH : VIT_KPATCH};
    if (int rc = p16 ? launch_gemm<EPI_PATCH16>(a, "op_patch_embed", s, tile_rows) : launch_gemm<EPI_PATCH>(a, "op_patch_embed", s, tile_rows))
        return rc;
    return launch_cls_token(cls_token, pos_embed, tokens, B, D, p16 ? VIT16_N : VIT_N, s);
}

int orbit_op_vit_patch_embed(const float* frames, const float* w, const float* bias_or_null, const float* pos_embed,
                             const float* cls_token, float* tokens, int B, int D, int tile_rows, orbit_stream_t stream) {
    return orbit_op_vit_patch_embed_p(frames, w, bias_or_null, pos_embed, cls_token, tokens, B, D, VIT_PATCH, tile_rows, stream);
}

// the patch embedding on square frames of side S (a multiple of the patch, 32..512): pos_embed is the table AT that grid,
// [(S / patch)^2 + 1][D] (orbit_op_vit_pos_resample makes it); always the runtime-geometry form of the GEMM, at S = 224 too
int orbit_op_vit_patch_embed_sized(const float* frames, const float* w, const float* bias_or_null, const float* pos_embed,
                                   const float* cls_token, float* tokens, int B, int D, int patch, int S, int tile_rows,
                                   orbit_stream_t stream) {
    const char* who = "op_vit_patch_embed_sized";
    ORBIT_REQUIRE(frames && w && pos_embed && cls_token && tokens, "%s: null pointer", who);
    ORBIT_REQUIRE(patch == VIT_PATCH || patch == VIT16_PATCH, "%s: patch size %d (32 or 16)", who, patch);
    ORBIT_REQUIRE(S >= VIT_SIZED_MIN && S <= VIT_SIZED_MAX && S % patch == 0,
                  "%s: frame size %d (a multiple of the patch size %d in %d..%d)", who, S, patch, VIT_SIZED_MIN, VIT_SIZED_MAX);
    const int grid = S / patch, np = grid * grid, max_b = VIT_MAX_B * VIT_N / (np + 1);
    ORBIT_REQUIRE(B > 0 && B <= max_b, "%s: batch of %d frames (1..%d)", who, B, max_b);
    ORBIT_REQUIRE(D == 384 || D == 768, "%s: unsupported width %d (384 or 768)", who, D);
    ORBIT_REQUIRE(((uintptr_t)frames & 15) == 0 && ((uintptr_t)w & 15) == 0, "%s: frames and w must be 16-byte aligned", who);
    ORBIT_REQUIRE(((uintptr_t)tokens & 3) == 0 && ((uintptr_t)bias_or_null & 3) == 0 && ((uintptr_t)pos_embed & 3) == 0 &&
                      ((uintptr_t)cls_token & 3) == 0,
                  "%s: tokens, bias, pos_embed and cls_token must be 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    GemmArgs a{frames, w, bias_or_null, nullptr, pos_embed, tokens, B * np, D, 3 * patch * patch};
    a.side = S, a.grid = grid;
    if (int rc = patch == VIT16_PATCH ? launch_gemm<EPI_PATCH16_RT>(a, "op_patch_embed_sized", s, tile_rows)
                                      : launch_gemm<EPI_PATCH_RT>(a, "op_patch_embed_sized", s, tile_rows))
        return rc;
    return launch_cls_token(cls_token, pos_embed, tokens, B, D, np + 1, s);
}

// pos [g*g + 1][D] (g = 7 or 14: the checkpoint's table) -> out [G*G + 1][D], 1 <= G <= 32
int orbit_op_vit_pos_resample(const float* pos, float* out, int g, int G, int D, orbit_stream_t stream) {
    ORBIT_REQUIRE(pos && out, "op_vit_pos_resample: null pointer");
    ORBIT_REQUIRE(g == VIT_GRID || g == VIT16_GRID, "op_vit_pos_resample: source grid %d (7 or 14)", g);
    ORBIT_REQUIRE(G >= 1 && G <= VIT_SIZED_MAX / VIT16_PATCH, "op_vit_pos_resample: target grid %d (1..%d)", G,
                  VIT_SIZED_MAX / VIT16_PATCH);
    ORBIT_REQUIRE(D == 384 || D == 768, "op_vit_pos_resample: unsupported width %d (384 or 768)", D);
    ORBIT_REQUIRE((((uintptr_t)pos | (uintptr_t)out) & 3) == 0, "op_vit_pos_resample: pointers must be 4-byte aligned");
    ORBIT_REQUIRE(pos != out, "op_vit_pos_resample: out must not alias pos");
    return launch_pos_resample(pos, out, g, G, D, (hipStream_t)stream);
}

int orbit_op_vit_layernorm(const float* x, size_t x_stride, float* y, size_t y_stride, int rows, int D, const float* gamma,
                           const float* beta, float eps, orbit_stream_t stream) {
    ORBIT_REQUIRE(x && y && gamma && beta, "op_vit_layernorm: null pointer");
    ORBIT_REQUIRE(D == 384 || D == 768, "op_vit_layernorm: unsupported width %d (384 or 768)", D);
    ORBIT_REQUIRE(rows > 0 && rows <= VIT_MAX_B * VIT_N, "op_vit_layernorm: %d rows (1..%d)", rows, VIT_MAX_B * VIT_N);
    ORBIT_REQUIRE(x_stride >= (size_t)D && y_stride >= (size_t)D, "op_vit_layernorm: row strides must be at least D");
    ORBIT_REQUIRE(eps >= 0.f, "op_vit_layernorm: negative eps");
    ORBIT_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 3) == 0,
                  "op_vit_layernorm: pointers must be 4-byte aligned");
    return launch_layernorm(x, x_stride, y, y_stride, rows, D, gamma, beta, eps, (hipStream_t)stream);
}

// tokens: 50 or 197 per frame (the 197-token kernel reads qkv and writes out as float4: 16-byte aligned)
int orbit_op_vit_attention_tokens(const float* qkv, float* out, int B, int tokens, int D, int heads, orbit_stream_t stream) {
    ORBIT_REQUIRE(qkv && out, "op_vit_attention: null pointer");
    ORBIT_REQUIRE(tokens == VIT_N || tokens == VIT16_N, "op_vit_attention: %d tokens per frame (50 or 197)", tokens);
    ORBIT_REQUIRE(D == 384 || D == 768, "op_vit_attention: unsupported width %d (384 or 768)", D);
    ORBIT_REQUIRE(heads * VIT_HD == D, "op_vit_attention: %d heads of %d do not make D=%d", heads, VIT_HD, D);
    const int max_b = tokens == VIT16_N ? VIT16_MAX_B : VIT_MAX_B;
    ORBIT_REQUIRE(B > 0 && B <= max_b, "op_vit_attention: batch of %d frames (1..%d)", B, max_b);
    const uintptr_t mask = tokens == VIT16_N ? 15 : 3;
    ORBIT_REQUIRE((((uintptr_t)qkv | (uintptr_t)out) & mask) == 0, "op_vit_attention: pointers must be %d-byte aligned",
                  (int)mask + 1);
    return launch_attention(qkv, out, B, tokens, D, heads, (hipStream_t)stream);
}

// any token count on vit_attention_n_kernel (50 and 197 too): B * tokens at most 8192 * 50 rows
int orbit_op_vit_attention_n(const float* qkv, float* out, int B, int tokens, int D, int heads, orbit_stream_t stream) {
    ORBIT_REQUIRE(qkv && out, "op_vit_attention_n: null pointer");
    ORBIT_REQUIRE(tokens >= 1 && tokens <= VIT_MAX_B * VIT_N, "op_vit_attention_n: %d tokens per frame (1..%d)", tokens,
                  VIT_MAX_B * VIT_N);
    ORBIT_REQUIRE(D == 384 || D == 768, "op_vit_attention_n: unsupported width %d (384 or 768)", D);
    ORBIT_REQUIRE(heads * VIT_HD == D, "op_vit_attention_n: %d heads of %d do not make D=%d", heads, VIT_HD, D);
    const int max_b = VIT_MAX_B * VIT_N / tokens;
    ORBIT_REQUIRE(B > 0 && B <= max_b, "op_vit_attention_n: batch of %d frames (1..%d)", B, max_b);
    ORBIT_REQUIRE((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "op_vit_attention_n: pointers must be 16-byte aligned");
    return launch_attention_n(qkv, out, B, tokens, D, heads, (hipStream_t)stream);
}

int orbit_op_vit_attention(const float* qkv, float* out, int B, int D, int heads, orbit_stream_t stream) {
    return orbit_op_vit_attention_tokens(qkv, out, B, VIT_N, D, heads, stream);
}

int orbit_op_vit_linear_dgrad(const float* dy, const float* w, float* wt_scratch, const float* u, const float* residual,
                              float* dx, int M, int N, int K, int tile_rows, orbit_stream_t stream) {
    ORBIT_REQUIRE(dy && w && wt_scratch && dx, "op_vit_linear_dgrad: null pointer");
    ORBIT_REQUIRE(M > 0 && M <= VIT_MAX_B * VIT_N && N > 0 && K > 0, "op_vit_linear_dgrad: bad shape M=%d N=%d K=%d", M, N, K);
    ORBIT_REQUIRE(K % G_BN == 0 && N % G_BK == 0,
                  "op_vit_linear_dgrad: K (the Linear's in_features) must be a multiple of %d and N of %d, got N=%d K=%d", G_BN,
                  G_BK, N, K);
    ORBIT_REQUIRE(!(u && residual), "op_vit_linear_dgrad: either u (times GELU') or residual (accumulate), not both");
    if (int rc = check_tile_rows(tile_rows)) return rc;  // (here too: the transpose below launches before launch_gemm)
    ORBIT_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)wt_scratch & 15) == 0,
                  "op_vit_linear_dgrad: dy, w and wt_scratch must be 16-byte aligned");
    ORBIT_REQUIRE(((uintptr_t)dx & 3) == 0 && ((uintptr_t)u & 3) == 0 && ((uintptr_t)residual & 3) == 0,
                  "op_vit_linear_dgrad: dx, u and residual must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = vit_transpose(w, wt_scratch, N, K, s)) return rc;
    const GemmArgs a{dy, wt_scratch, nullptr, u ? u : residual, nullptr, dx, M, K, N};
    if (u) return launch_gemm<EPI_DGELU, true>(a, "op_dgrad_gelu", s, tile_rows);
    if (residual) return launch_gemm<EPI_RESIDUAL, true>(a, "op_dgrad_residual", s, tile_rows);
    return launch_gemm<EPI_BIAS, true>(a, "op_dgrad", s, tile_rows);
}

int orbit_op_vit_layernorm_bwd(const float* x, size_t x_stride, const float* dy, size_t dy_stride, const float* gamma, float eps,
                               const float* dres, float* dx, size_t dx_stride, int rows, int D, float* dgamma, float* dbeta,
                               float* partial, size_t partial_floats, orbit_stream_t stream) {
    ORBIT_REQUIRE(x && dy && gamma && dgamma && dbeta && partial, "op_vit_layernorm_bwd: null pointer");
    ORBIT_REQUIRE(D == 384 || D == 768, "op_vit_layernorm_bwd: unsupported width %d (384 or 768)", D);
    ORBIT_REQUIRE(rows > 0 && rows <= VIT_MAX_B * VIT_N, "op_vit_layernorm_bwd: %d rows (1..%d)", rows, VIT_MAX_B * VIT_N);
    ORBIT_REQUIRE(x_stride >= (size_t)D && dy_stride >= (size_t)D && (!dx || dx_stride >= (size_t)D),
                  "op_vit_layernorm_bwd: row strides must be at least D");
    ORBIT_REQUIRE(dx || !dres, "op_vit_layernorm_bwd: dres without dx");
    ORBIT_REQUIRE(!dres || dx_stride == (size_t)D, "op_vit_layernorm_bwd: dres goes with contiguous rows (dx_stride == D) only");
    ORBIT_REQUIRE(eps >= 0.f, "op_vit_layernorm_bwd: negative eps");
    ORBIT_REQUIRE(partial_floats >= layernorm_bwd_partial_floats(rows, D),
                  "op_vit_layernorm_bwd: partial buffer too small (%zu < %zu floats)", partial_floats,
                  layernorm_bwd_partial_floats(rows, D));
    ORBIT_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)gamma | (uintptr_t)dres | (uintptr_t)dx | (uintptr_t)dgamma |
                    (uintptr_t)dbeta | (uintptr_t)partial) & 3) == 0,
                  "op_vit_layernorm_bwd: pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // the final-norm form: the rows x dx_stride stream is zeroed first, as orbit_vit_backward zeroes its gradient stream
    if (dx && dx_stride > (size_t)D)
        if (int rc = zero_gradient_stream(dx, (size_t)rows * dx_stride, s)) return rc;
    return launch_layernorm_bwd(x, x_stride, dy, dy_stride, gamma, eps, dres, dx, dx_stride, rows, D, partial, dgamma, dbeta, s);
}

int orbit_op_vit_attention_bwd_tokens(const float* qkv, const float* dout, float* dqkv, int B, int tokens, int D, int heads,
                                      orbit_stream_t stream) {
    ORBIT_REQUIRE(qkv && dout && dqkv, "op_vit_attention_bwd: null pointer");
    ORBIT_REQUIRE(tokens == VIT_N || tokens == VIT16_N, "op_vit_attention_bwd: %d tokens per frame (50 or 197)", tokens);
    ORBIT_REQUIRE(D == 384 || D == 768, "op_vit_attention_bwd: unsupported width %d (384 or 768)", D);
    ORBIT_REQUIRE(heads * VIT_HD == D, "op_vit_attention_bwd: %d heads of %d do not make D=%d", heads, VIT_HD, D);
    const int max_b = tokens == VIT16_N ? VIT16_MAX_B : VIT_MAX_B;
    ORBIT_REQUIRE(B > 0 && B <= max_b, "op_vit_attention_bwd: batch of %d frames (1..%d)", B, max_b);
    const uintptr_t mask = tokens == VIT16_N ? 15 : 3;  // (the 197-token kernel moves float4)
    ORBIT_REQUIRE((((uintptr_t)qkv | (uintptr_t)dout | (uintptr_t)dqkv) & mask) == 0,
                  "op_vit_attention_bwd: pointers must be %d-byte aligned", (int)mask + 1);
    return launch_attention_bwd(qkv, dout, dqkv, B, tokens, D, heads, (hipStream_t)stream);
}

int orbit_op_vit_attention_bwd(const float* qkv, const float* dout, float* dqkv, int B, int D, int heads,
                               orbit_stream_t stream) {
    return orbit_op_vit_attention_bwd_tokens(qkv, dout, dqkv, B, VIT_N, D, heads, stream);
}

size_t orbit_op_vit_linear_wgrad_workspace_floats(int M, int N, int K) {
    if (M <= 0 || M > VIT_MAX_B * VIT_N || N <= 0 || K <= 0 || N % W_BT || K % G_BK) return 0;
    return wgrad_ws_floats(M, N, K);
}

int orbit_op_vit_linear_wgrad(const float* dy, const float* x, float* dw, float* dbias_or_null, int M, int N, int K, int gelu_on_x,
                              float* workspace, size_t workspace_floats, orbit_stream_t stream) {
    ORBIT_REQUIRE(dy && x && dw, "op_vit_linear_wgrad: null pointer");
    ORBIT_REQUIRE(M > 0 && M <= VIT_MAX_B * VIT_N && N > 0 && K > 0, "op_vit_linear_wgrad: bad shape M=%d N=%d K=%d", M, N, K);
    ORBIT_REQUIRE(N % W_BT == 0 && K % G_BK == 0, "op_vit_linear_wgrad: N must be a multiple of %d and K of %d, got N=%d K=%d",
                  W_BT, G_BK, N, K);
    ORBIT_REQUIRE(gelu_on_x == 0 || gelu_on_x == 1, "op_vit_linear_wgrad: gelu_on_x must be 0 or 1, got %d", gelu_on_x);
    const size_t need = wgrad_ws_floats(M, N, K);
    ORBIT_REQUIRE(workspace || need == 0, "op_vit_linear_wgrad: null pointer");
    ORBIT_REQUIRE(workspace_floats >= need, "op_vit_linear_wgrad: workspace too small (%zu < %zu floats)", workspace_floats, need);
    ORBIT_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw | (uintptr_t)dbias_or_null | (uintptr_t)workspace) & 15) == 0,
                  "op_vit_linear_wgrad: dy, x, dw, dbias and workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (gelu_on_x) return launch_wgrad<WX_GELU>(dy, x, dw, dbias_or_null, M, N, K, workspace, "op_wgrad_gelu", s);
    return launch_wgrad<WX_PLAIN>(dy, x, dw, dbias_or_null, M, N, K, workspace, "op_wgrad", s);
}

// patch: 32 (dtokens [B][50][D], dw [D][3][32][32], B <= 8192) or 16 ([B][197][D], [D][3][16][16], B <= 2048)
int orbit_op_vit_patch_embed_bwd_p(const float* frames, const float* dtokens, float* dw, float* dbias_or_null, float* dpos,
                                   float* dcls, int B, int D, int patch, float* workspace, size_t workspace_floats,
                                   orbit_stream_t stream) {
    ORBIT_REQUIRE(frames && dtokens && dw && dpos && dcls, "op_vit_patch_embed_bwd: null pointer");
    ORBIT_REQUIRE(patch == VIT_PATCH || patch == VIT16_PATCH, "op_vit_patch_embed_bwd: patch size %d (32 or 16)", patch);
    const bool p16 = patch == VIT16_PATCH;
    const int max_b = p16 ? VIT16_MAX_B : VIT_MAX_B;
    ORBIT_REQUIRE(B > 0 && B <= max_b, "op_vit_patch_embed_bwd: batch of %d frames (1..%d)", B, max_b);
    ORBIT_REQUIRE(D == 384 || D == 768, "op_vit_patch_embed_bwd: unsupported width %d (384 or 768)", D);
    const size_t need = p16 ? wgrad_ws_floats(B * VIT16_P, D, VIT16_KPATCH) : wgrad_ws_floats(B * VIT_P, D, VIT_KPATCH);
    ORBIT_REQUIRE(workspace || need == 0, "op_vit_patch_embed_bwd: null pointer");
    ORBIT_REQUIRE(workspace_floats >= need, "op_vit_patch_embed_bwd: workspace too small (%zu < %zu floats)", workspace_floats, need);
    ORBIT_REQUIRE((((uintptr_t)frames | (uintptr_t)dtokens | (uintptr_t)dw | (uintptr_t)dbias_or_null | (uintptr_t)workspace) & 15) == 0,
                  "op_vit_patch_embed_bwd: frames, dtokens, dw, dbias and workspace must be 16-byte aligned");
    ORBIT_REQUIRE((((uintptr_t)dpos | (uintptr_t)dcls) & 3) == 0, "op_vit_patch_embed_bwd: dpos and dcls must be 4-byte aligned");
    return launch_patch_embed_bwd(frames, dtokens, dw, dbias_or_null, dpos, dcls, B, D, patch, workspace, (hipStream_t)stream);
}

int orbit_op_vit_patch_embed_bwd(const float* frames, const float* dtokens, float* dw, float* dbias_or_null, float* dpos,
                                 float* dcls, int B, int D, float* workspace, size_t workspace_floats, orbit_stream_t stream) {
    return orbit_op_vit_patch_embed_bwd_p(frames, dtokens, dw, dbias_or_null, dpos, dcls, B, D, VIT_PATCH, workspace,
                                          workspace_floats, stream);
}

}  // extern "C"
