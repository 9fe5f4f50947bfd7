// Narrow gated pointwise projections as ONE STREAM over the activations, with the squeeze-excite gate computed in the
// prologue. A member of the register-GEMM family of option conv_rgemm: it serves the layers it supports unless that is 0.
//
// EfficientNet-B0's early MBConv blocks end in a 1x1 projection y = scale * conv(x * gate) + shift (+ residual) with
// K = Cin <= 240 and Cout <= 40 on 112x112 / 56x56 / 28x28 maps. At 5-16 FLOP per byte these are HBM-bound; conv_igemm.hip
// serves them with an LDS-staged tile (two barriers per K-tile, a tile prologue and an LDS-staged epilogue per 128x32 tile,
// Cout 40 padded to 64), and every one of them waits for its own se_gate2 launch (one block per frame). Here:
//
//   * A is read as one contiguous stream: NHWC rows are the GEMM rows and K is the whole row, so a 16-pixel tile is
//     16 * K * 4 contiguous bytes. Lane (j, q) = (lane & 15, lane >> 4) loads x[pixel j][16 c + 4 q .. +3] (float4, 64 B of
//     every pixel row per instruction) straight into registers; the next tile's loads are issued before the current tile's
//     MFMAs, no LDS stage and no barrier in the loop.
//   * The weights (<= 48 x 240 floats) are copied once per block into LDS in fragment order wl[chunk][n_tile][lane] (one
//     ds_read_b128 per lane feeds four MFMAs). N is padded to 16, the v_mfma_f32_16x16x4_f32 width (40 -> 48, not 64).
//   * The MFMA runs transposed (A operand = weights, B operand = pixels, as pw_rgemm.hip): a lane's four accumulators are
//     four consecutive output channels of one pixel, so scale / shift / residual / store are float4s without an LDS stage.
//   * A block owns a run of 16-pixel tiles of ONE frame (H * W % 16 == 0) and computes that frame's gate itself with the
//     same se_gate_frame<256, 4> arithmetic as se_gate2_kernel<256> (bit-identical gates), into LDS. Its first tile loads
//     are issued before the gate, so the gate's first L2 round trip overlaps the first HBM latency.
//
// The K order of an output is fixed by the layer (chunk by chunk; inside a chunk of 16 channels MFMA e sums channels
// 16 c + 4 q + e, q = 0..3): the bits of a frame do not depend on the batch or on which block serves it.
#include <algorithm>
#include <type_traits>
#include "common.h"
#include "se_gate.h"

namespace orbit {

using f32x4 = __attribute__((ext_vector_type(4))) float;

struct PwsParams {
    const float* x;         // NHWC [B * HW][K]
    const float* w;         // packed [CoutPad][KT] (conv_pack_weights), rows >= Cout are zero
    float* y;               // NHWC [B * HW][Cout]
    const float* scale;     // [Cout]
    const float* shift;     // [Cout]
    const float* residual;  // like y, or nullptr
    const float* partial;   // squeeze-excite pooling partials [B][chunks][K]
    const float *w1, *b1, *w2t, *b2;
    float* gate_out;        // [B][K] or nullptr (tests: the gate the block computed)
    float inv_hw;
    int KT, chunks, R, HW, Cout;
    int tiles;              // 16-pixel tiles per frame
    int bpf;                // blocks per frame
};

template <int KC, int NG, int TP>  // K = 16 KC; NG 16-channel output tiles; TP pixel tiles per wave step
__global__ __launch_bounds__(256) void pw_stream_kernel(PwsParams p) {
    constexpr int K = 16 * KC;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    f32x4* wl = reinterpret_cast<f32x4*>(sm);  // [KC][NG][64]
    float* gl = sm + KC * NG * 256;            // [K] this frame's gate
    float* sg = gl + K;                        // se_gate_frame scratch: ((K + R + 3) & ~3) + 1024 floats
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4;
    const int b = blockIdx.x / p.bpf, seg = blockIdx.x - b * p.bpf;
    const int t_beg = (int)((long)seg * p.tiles / p.bpf), t_end = (int)((long)(seg + 1) * p.tiles / p.bpf);
    const size_t pix0 = (size_t)b * p.HW + (lane & 15);  // this lane's pixel in tile 0 of the frame
    const bool has_res = p.residual != nullptr;

    auto has = [&](int s) { return t_beg + (4 * s + wave) * TP < t_end; };  // wave-uniform
    auto tile_of = [&](int s, int u) { return t_beg + (4 * s + wave) * TP + u; };
    // the pixel row of this lane in tile u of step s; a tile past the block's range (only in the last step of a wave with
    // TP > 1) re-reads the step's first tile and is not stored
    auto row_of = [&](int s, int u) {
        const int t = tile_of(s, u);
        return pix0 + (size_t)16 * (t < t_end ? t : tile_of(s, 0));
    };

    f32x4 xa[TP][KC];
    if (has(0)) {  // in flight under the weight copy and the gate
#pragma unroll
        for (int u = 0; u < TP; ++u) {
            const float* px = p.x + row_of(0, u) * K + 4 * q;
#pragma unroll
            for (int c = 0; c < KC; ++c) xa[u][c] = *reinterpret_cast<const f32x4*>(px + 16 * c);
        }
    }

    for (int i = tid; i < KC * NG * 64; i += 256) {
        const int l = i & 63, g = (i >> 6) % NG, c = (i >> 6) / NG;
        wl[i] = *reinterpret_cast<const f32x4*>(p.w + (size_t)(16 * g + (l & 15)) * p.KT + 16 * c + 4 * (l >> 4));
    }
    se_gate_frame<256, 4>(p.partial + (size_t)b * p.chunks * K, p.chunks, p.inv_hw, p.w1, p.b1, p.w2t, p.b2, gl, K, p.R,
                          nullptr, sg);
    __syncthreads();
    if (p.gate_out != nullptr && seg == 0)
        for (int c4 = tid; c4 < K / 4; c4 += 256)
            reinterpret_cast<f32x4*>(p.gate_out + (size_t)b * K)[c4] = reinterpret_cast<const f32x4*>(gl)[c4];

    f32x4 sc[NG], sh[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int ch = 16 * g + 4 * q;
        const bool ok = ch < p.Cout;
        sc[g] = ok ? *reinterpret_cast<const f32x4*>(p.scale + ch) : (f32x4){0.f, 0.f, 0.f, 0.f};
        sh[g] = ok ? *reinterpret_cast<const f32x4*>(p.shift + ch) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    // One wave step: TP tiles x all of K. Each chunk's registers are refilled IN PLACE with the next step's chunk right after
    // they are read, so a whole tile of loads stays in flight under the MFMAs with one set of registers (REFILL: a next
    // step exists; the call without it keeps the loads exact, no re-reads at the end of a wave).
    auto step = [&](int s, auto refill) {
        constexpr bool REFILL = decltype(refill)::value;
        // the weight and gate reads below are loop-invariant: kept in LDS, not hoisted into ~(KC * NG + KC) * 4 registers
        __asm__ volatile("" ::: "memory");
        size_t row[TP], nrow[TP];
#pragma unroll
        for (int u = 0; u < TP; ++u) row[u] = row_of(s, u), nrow[u] = REFILL ? row_of(s + 1, u) : row[u];
        f32x4 rr[TP][NG];
        if (has_res)
#pragma unroll
            for (int u = 0; u < TP; ++u)
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const int ch = 16 * g + 4 * q;
                    rr[u][g] = *reinterpret_cast<const f32x4*>(p.residual + row[u] * p.Cout + (ch < p.Cout ? ch : 0));
                }
        f32x4 acc[TP][NG];
#pragma unroll
        for (int u = 0; u < TP; ++u)
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[u][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(gl + 16 * c + 4 * q);
            f32x4 xv[TP];
#pragma unroll
            for (int u = 0; u < TP; ++u) {
                xv[u] = xa[u][c] * gv;
                if (REFILL) xa[u][c] = *reinterpret_cast<const f32x4*>(p.x + nrow[u] * K + 4 * q + 16 * c);
            }
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const f32x4 wv = wl[(c * NG + g) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int u = 0; u < TP; ++u)
                        acc[u][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], xv[u][e], acc[u][g], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < TP; ++u) {
            if (tile_of(s, u) >= t_end) continue;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int ch = 16 * g + 4 * q;
                if (ch >= p.Cout) continue;
                f32x4 o = acc[u][g] * sc[g] + sh[g];
                if (has_res) o += rr[u][g];
                *reinterpret_cast<f32x4*>(p.y + row[u] * p.Cout + ch) = o;
            }
        }
    };
    int s = 0;
    for (; has(s + 1); ++s) step(s, std::true_type{});
    if (has(s)) step(s, std::false_type{});
}

namespace {
struct PwsVariant {
    int kc, ng, tp;
    void (*fn)(PwsParams);
};
// the EfficientNet-B0 narrow projections: 32 -> 16 @112, 96 / 144 -> 24 @56, 144 -> 40 @28. Two pixel tiles per wave step
// where a tile is only 2 KiB (K = 32), so that a wave keeps 4 KiB of loads in flight. 240 -> 40 @28 (block 3.1) stays on
// se_gate2 + conv_igemm: this kernel measured 73.6 us there against 67.4 for the pair (profiles/r07_pw_stream.txt; 180
// MFMAs per 16-pixel tile at 2 waves per SIMD).
const PwsVariant kVariants[] = {
    {2, 1, 2, pw_stream_kernel<2, 1, 2>},
    {6, 2, 1, pw_stream_kernel<6, 2, 1>},
    {9, 2, 1, pw_stream_kernel<9, 2, 1>},
    {9, 3, 1, pw_stream_kernel<9, 3, 1>},
};
const PwsVariant* find_variant(int Cin, int Cout) {
    if (Cin % 16 != 0 || Cout % 8 != 0 || Cout > 48) return nullptr;
    for (const PwsVariant& v : kVariants)
        if (v.kc == Cin / 16 && v.ng == cdiv(Cout, 16)) return &v;
    return nullptr;
}
}  // namespace

// a function of the layer only (never of the batch): which kernel serves a layer fixes its summation order
bool pw_stream_supported(int Cin, int Cout, int H, int W) {
    return find_variant(Cin, Cout) != nullptr && (H * W) % 16 == 0;
}

int launch_pw_stream(const PwStreamDesc& d, hipStream_t s) {
    ORBIT_REQUIRE(d.x && d.w_packed && d.y && d.scale && d.shift && d.partial && d.w1 && d.b1 && d.w2t && d.b2,
                  "pw_stream: null pointer");
    ORBIT_REQUIRE(pw_stream_supported(d.Cin, d.Cout, d.H, d.W), "pw_stream: unsupported layer %d -> %d @%dx%d", d.Cin, d.Cout,
                  d.H, d.W);
    ORBIT_REQUIRE(d.B > 0 && d.chunks > 0 && d.se_hw > 0 && d.R > 0, "pw_stream: bad sizes");
    const PwsVariant& v = *find_variant(d.Cin, d.Cout);
    const ConvPackGeom geom = conv_pack_geom(d.Cin, d.Cout, 1, 1, 0);
    ORBIT_REQUIRE(geom.kt >= d.Cin && geom.cout_pad >= 16 * v.ng, "pw_stream: packed filter too small");
    PwsParams p;
    p.x = d.x, p.w = d.w_packed, p.y = d.y, p.scale = d.scale, p.shift = d.shift, p.residual = d.residual;
    p.partial = d.partial, p.w1 = d.w1, p.b1 = d.b1, p.w2t = d.w2t, p.b2 = d.b2, p.gate_out = d.gate_out;
    p.inv_hw = 1.0f / (float)d.se_hw;  // as launch_se_gate2
    p.KT = geom.kt, p.chunks = d.chunks, p.R = d.R, p.HW = d.H * d.W, p.Cout = d.Cout;
    p.tiles = p.HW / 16;
    // about six wave steps per block: long enough to amortise the block's gate and weight copy, short enough that the
    // 28x28 layers (49 tiles per frame) still give 3 blocks per frame
    p.bpf = std::max(1, std::min(p.tiles, cdiv(p.tiles, 24 * v.tp)));
    ORBIT_REQUIRE((long long)d.B * p.bpf < (1ll << 31), "pw_stream: grid too large");
    const size_t lds = ((size_t)v.kc * v.ng * 256 + d.Cin + ((d.Cin + d.R + 3) & ~3) + 4 * 256) * sizeof(float);
    const double M = (double)d.B * p.HW;
    char name[48];
    snprintf(name, sizeof(name), "conv_pw_stream<%dx%d%s>", d.Cin, d.Cout, d.residual ? ",res" : "");
    const int rec = prof_start(name, 2.0 * M * d.Cin * d.Cout,
                               4.0 * (M * d.Cin + M * d.Cout * (d.residual ? 2.0 : 1.0) + (double)d.B * d.chunks * d.Cin), s);
    hipLaunchKernelGGL(v.fn, dim3((unsigned)(d.B * p.bpf)), dim3(256), lds, s, p);
    prof_stop(rec, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

}  // namespace orbit

extern "C" {

int orbit_pw_stream_supported(int Cin, int Cout, int H, int W) { return orbit::pw_stream_supported(Cin, Cout, H, W) ? 1 : 0; }

/* Gated projection with its squeeze-excite gate, single-operator form (parity tests, tools/pw_stream_bench.py):
 *   gate = sigmoid(W2 silu(W1 (sum_chunks partial) / HW + b1) + b2),  y = scale * conv1x1(x * gate) + shift (+ residual).
 * With option conv_rgemm != 0 and the layer supported, one pw_stream launch; otherwise the pair the plan runs for other
 * layers, se_gate2 + launch_conv. w: torch [Cout][Cin][1][1]; w2t: W2 transposed to [R][Cin]; gate_out: [B][Cin] or nullptr. */
int orbit_op_pw_stream(const float* x, const float* w, const float* scale, const float* shift, const float* residual,
                       const float* partial, int chunks, const float* w1, const float* b1, const float* w2t, const float* b2,
                       int R, float* y, float* gate_out, int B, int H, int W, int Cin, int Cout, orbit_stream_t stream) {
    using namespace orbit;
    ORBIT_REQUIRE(x && w && scale && shift && partial && w1 && b1 && w2t && b2 && y, "op_pw_stream: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const bool fused = get_option("conv_rgemm") && pw_stream_supported(Cin, Cout, H, W);
    TempPackedFilter f;  // (+ the gate, where the caller does not take it)
    if (int rc = f.pack(w, Cin, Cout, 1, 1, 0, true, (fused || gate_out) ? 0 : (size_t)B * Cin, s)) return rc;
    if (fused) {
        PwStreamDesc d;
        d.x = x, d.w_packed = f.packed, d.y = y, d.scale = scale, d.shift = shift, d.residual = residual;
        d.partial = partial, d.chunks = chunks, d.se_hw = H * W, d.w1 = w1, d.b1 = b1, d.w2t = w2t, d.b2 = b2, d.R = R;
        d.gate_out = gate_out, d.B = B, d.H = H, d.W = W, d.Cin = Cin, d.Cout = Cout;
        return launch_pw_stream(d, s);
    }
    float* gate = gate_out ? gate_out : f.extra;
    if (int rc = launch_se_gate2(partial, chunks, H * W, w1, b1, w2t, b2, gate, B, Cin, R, s)) return rc;
    ConvDesc d;
    d.x = x, d.w_packed = f.packed, d.w_frag = f.frag, d.y = y, d.scale = scale, d.shift = shift;
    d.residual = residual, d.gate = gate;
    d.geom() = LayerGeom{B, H, W, Cin, Cout, 1, 1, 1, 0, 0, H, W};
    return launch_conv(d, s);  // (no split-K workspace: as the plan, these layers never split)
}

}  // extern "C"
