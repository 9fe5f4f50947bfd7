// Input side of the path: 8-bit frames -> normalised fp32 NCHW frames, on the GPU.
// Reference: data/datasets.py:422-431 load_and_transform_frame = torchvision to_tensor (HWC uint8 -> CHW float / 255)
// followed by normalize((x - mean) / std) with the statistics of :82-87, executed per frame on the host and shipped as
// fp32 (602 KB per 224x224 frame). Uploading the decoded 8-bit pixels instead (150 KB per frame) and normalising here
// quarters the PCIe bytes; the arithmetic is the same two fp32 operations in the same order, so the result is
// bit-identical to the reference transform.
//
// frames_resize_u8_kernel does the same for frames stored at another size than the extractor runs at: Pillow's 8-bit
// Image.resize (the reference's offline scripts/resize_videos.py:46 pass) restated in integers, then the same transform.
// The coefficient tables are Pillow's (src/libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc), built on the
// host in double by orbit_resize_coeffs and cached on the device per (in, out, filter); the kernel only multiplies,
// shifts and clamps, so the resized pixels equal Pillow's bit for bit. What a tile needs in LDS, and with it the sizes the
// launcher refuses, is stated at orbit_frames_resize_from_uint8 in include/orbit_hip.h.
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
#include "common.h"

namespace orbit {

// one thread per output pixel (b, h, w): reads 3 bytes, writes 3 floats into the three channel planes
__global__ __launch_bounds__(256) void frames_u8_kernel(const uint8_t* __restrict__ in, int hwc, int HW, size_t total,
                                                        float m0, float m1, float m2, float s0, float s1, float s2,
                                                        float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t b = i / HW, p = i - b * HW;
        uint8_t r, g, bl;
        if (hwc) {
            const uint8_t* px = in + i * 3;
            r = px[0], g = px[1], bl = px[2];
        } else {
            const uint8_t* px = in + b * 3 * HW + p;
            r = px[0], g = px[HW], bl = px[2 * (size_t)HW];
        }
        float* o = out + b * 3 * HW + p;
        o[0] = ((float)r / 255.0f - m0) / s0;
        o[HW] = ((float)g / 255.0f - m1) / s1;
        o[2 * (size_t)HW] = ((float)bl / 255.0f - m2) / s2;
    }
}

// ---- Pillow-exact resize ----------------------------------------------------------------------------------------------------
constexpr int RS_TW = 32;               // output columns of a tile: one 128-byte float segment per output row and channel
constexpr int RS_TH = 16;               // output rows of a tile; halved until the tile's working set fits the LDS
constexpr int RS_THREADS = 256;
constexpr int RS_ROWS = RS_THREADS / RS_TW;  // input rows the block resamples side by side
constexpr int RS_ROWS_PER_THREAD = 4;        // ... and one below the other in every thread, sharing its coefficient loads
constexpr int RS_RC = RS_ROWS * RS_ROWS_PER_THREAD;  // input rows staged per round (fewer where the LDS is short)
constexpr int RS_LDS_BYTES = 64 * 1024;
constexpr int RS_MAX_BLOCKS = 1 << 23;  // per launch (2^31 threads); more frames than that go in several launches

// one axis' table on the device: output index i reads inputs xmin[i] .. xmin[i] + n[i] - 1 with the weights kk[t][i], t < n[i]
// (tap-major, so that lanes on neighbouring outputs load neighbouring words)
struct ResizeAxis {
    const int32_t* kk;
    const int* xmin;
    const int* n;
    int out;
};

__device__ __forceinline__ uint8_t resize_clip8(int acc) {  // Pillow's clip8: arithmetic shift, then clamp
    const int v = acc >> 22;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One block per (frame, tile of th x RS_TW output pixels); lanes run along x in every stage.
//   stage 0  copies the input rows the tile's vertical windows cover - only the columns its horizontal windows cover - into
//            LDS, rc rows per round, as contiguous 4-byte loads: one run of 3 * wc bytes per row (pixels interleaved) or one
//            run of wc bytes per row and channel (planes). A run starts at LDS offset run * pitch whatever its address in
//            memory, so the loads are not aligned; the last word of the buffer is read byte by byte, never past its end.
//   stage 1  resamples those rows horizontally from LDS, rounds and clamps them to 8 bits as Pillow's first pass does, and
//            keeps them in LDS, one plane per channel: rs_rows [3][span][RS_TW]. A thread owns one output column and
//            RS_ROWS_PER_THREAD rows of the round: one coefficient load serves 12 multiply-adds.
//   stage 2  resamples rs_rows vertically, normalises and stores the three planes, one contiguous float segment per row.
// The table lookups stay inside the frame by construction of the tables (xmin >= 0, xmin + n <= in, both nondecreasing): the
// columns of stage 1 inside [col0, col0 + wc), the rows of stage 2 inside [row0, row0 + span).
// U8OUT: stage 2 stores the resized pixels themselves, interleaved ([B][H_out][W_out][3], out_u8), instead of normalising them.
template <bool U8OUT>
__global__ __launch_bounds__(RS_THREADS) void frames_resize_u8_kernel(const uint8_t* __restrict__ in, size_t in_bytes, int hwc,
                                                                      int H_in, int W_in, int H_out, int W_out, int th_max,
                                                                      int tiles_x, int tiles_y, int rc, int pitch, int stage_off,
                                                                      ResizeAxis ax, ResizeAxis ay, float m0, float m1, float m2,
                                                                      float s0, float s1, float s2, float* __restrict__ out,
                                                                      uint8_t* __restrict__ out_u8) {
    extern __shared__ __align__(16) uint8_t rs_lds[];
    uint8_t* rs_rows = rs_lds;             // [3][span][RS_TW]
    uint8_t* rs_in = rs_lds + stage_off;   // [rc][hwc ? 1 : 3][pitch]
    const int tile = blockIdx.x % (tiles_x * tiles_y);
    const size_t b = blockIdx.x / (tiles_x * tiles_y);
    const int x0 = (tile % tiles_x) * RS_TW, y0 = (tile / tiles_x) * th_max;
    const int tw = min(RS_TW, W_out - x0), th = min(th_max, H_out - y0);
    const int row0 = ay.xmin[y0];
    const int span = ay.xmin[y0 + th - 1] + ay.n[y0 + th - 1] - row0;
    const int col0 = ax.xmin[x0];
    const int wc = ax.xmin[x0 + tw - 1] + ax.n[x0 + tw - 1] - col0;
    const size_t plane_in = (size_t)H_in * W_in, frame = b * 3 * plane_in;
    const int runs = hwc ? 1 : 3, run_len = hwc ? 3 * wc : wc, words = pitch >> 2;
    const int x = threadIdx.x % RS_TW, rl = threadIdx.x / RS_TW;
    const int xo = x0 + min(x, tw - 1), n_x = ax.n[xo];
    const int tap = hwc ? 3 : 1, chan = hwc ? 1 : pitch;  // LDS strides between taps and between channels of a pixel
    const int x_off = (ax.xmin[xo] - col0) * tap;

    for (int r0 = 0; r0 < span; r0 += rc) {
        const int nr = min(rc, span - r0);
        __syncthreads();  // the previous round's rows have been read
        for (int i = threadIdx.x; i < nr * runs * words; i += RS_THREADS) {
            const int q = i / words, d = i - q * words;  // run q = row * runs + channel, word d of it
            if (4 * d >= run_len) continue;
            const int r = q / runs, c = q - r * runs;
            const size_t pix = (size_t)(row0 + r0 + r) * W_in + col0;
            const size_t g = frame + (hwc ? 3 * pix : c * plane_in + pix) + 4 * d;
            uint32_t v = 0;
            if (g + 4 <= in_bytes) {
                __builtin_memcpy(&v, in + g, 4);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (g + j < in_bytes) v |= (uint32_t)in[g + j] << (8 * j);
            }
            *reinterpret_cast<uint32_t*>(rs_in + q * pitch + 4 * d) = v;
        }
        __syncthreads();
        if (x < tw && rl < nr) {
            int p[RS_ROWS_PER_THREAD];  // offsets into rs_in (indices, not pointers: the reads stay LDS instructions)
            int acc[RS_ROWS_PER_THREAD][3];
#pragma unroll
            for (int j = 0; j < RS_ROWS_PER_THREAD; ++j) {
                const int r = rl + RS_ROWS * j < nr ? rl + RS_ROWS * j : rl;  // (a row past the round: recompute row rl, store nothing)
                p[j] = r * runs * pitch + x_off;
                acc[j][0] = acc[j][1] = acc[j][2] = 1 << 21;
            }
            const int32_t* k = ax.kk + xo;
            for (int t = 0; t < n_x; ++t, k += ax.out) {
                const int w = *k;
#pragma unroll
                for (int j = 0; j < RS_ROWS_PER_THREAD; ++j) {
                    acc[j][0] += __mul24((int)rs_in[p[j]], w);  // |w| <= 1 << 22 and the pixel fit 24 bits: exact
                    acc[j][1] += __mul24((int)rs_in[p[j] + chan], w);
                    acc[j][2] += __mul24((int)rs_in[p[j] + 2 * chan], w);
                    p[j] += tap;
                }
            }
#pragma unroll
            for (int j = 0; j < RS_ROWS_PER_THREAD; ++j) {
                const int r = r0 + rl + RS_ROWS * j;
                if (rl + RS_ROWS * j < nr) {
                    rs_rows[(0 * span + r) * RS_TW + x] = resize_clip8(acc[j][0]);
                    rs_rows[(1 * span + r) * RS_TW + x] = resize_clip8(acc[j][1]);
                    rs_rows[(2 * span + r) * RS_TW + x] = resize_clip8(acc[j][2]);
                }
            }
        }
    }
    __syncthreads();
    const size_t plane = (size_t)H_out * W_out;
    for (int i = threadIdx.x; i < th * RS_TW; i += RS_THREADS) {
        const int yo = y0 + i / RS_TW;  // (i % RS_TW == x)
        if (x >= tw) continue;
        const int n = ay.n[yo];
        const int32_t* k = ay.kk + yo;
        int p = (ay.xmin[yo] - row0) * RS_TW + x;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int t = 0; t < n; ++t, p += RS_TW, k += ay.out) {
            const int w = *k;
            a0 += __mul24((int)rs_rows[p], w);
            a1 += __mul24((int)rs_rows[p + span * RS_TW], w);
            a2 += __mul24((int)rs_rows[p + 2 * span * RS_TW], w);
        }
        if (U8OUT) {
            uint8_t* o8 = out_u8 + (b * plane + (size_t)yo * W_out + x0 + x) * 3;
            o8[0] = resize_clip8(a0), o8[1] = resize_clip8(a1), o8[2] = resize_clip8(a2);
            continue;
        }
        float* o = out + b * 3 * plane + (size_t)yo * W_out + x0 + x;
        o[0] = ((float)resize_clip8(a0) / 255.0f - m0) / s0;
        o[plane] = ((float)resize_clip8(a1) / 255.0f - m1) / s1;
        o[2 * plane] = ((float)resize_clip8(a2) / 255.0f - m2) / s2;
    }
}

// ---- coefficient tables (host) ------------------------------------------------------------------------------------------------
// Pillow's filters (Resample.c bilinear_filter / bicubic_filter / lanczos_filter), evaluated in double without contraction
#pragma clang fp contract(off)
static double resize_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static double resize_filter(int filter, double x) {
    if (filter == ORBIT_RESIZE_LANCZOS) return (-3.0 <= x && x < 3.0) ? resize_sinc(x) * resize_sinc(x / 3) : 0.0;
    if (x < 0.0) x = -x;
    if (filter == ORBIT_RESIZE_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static double resize_support(int filter) { return filter == ORBIT_RESIZE_BILINEAR ? 1.0 : (filter == ORBIT_RESIZE_BICUBIC ? 2.0 : 3.0); }
static const char* resize_filter_name(int filter) {
    return filter == ORBIT_RESIZE_BILINEAR ? "bilinear" : (filter == ORBIT_RESIZE_BICUBIC ? "bicubic" : "lanczos");
}
static bool resize_filter_known(int filter) {
    return filter == ORBIT_RESIZE_BILINEAR || filter == ORBIT_RESIZE_BICUBIC || filter == ORBIT_RESIZE_LANCZOS;
}
static int resize_ksize(int in_size, int out_size, int filter) {
    double fs = (double)in_size / out_size;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(resize_support(filter) * fs) * 2 + 1;
}
// precompute_coeffs + normalize_coeffs_8bpc: kk [out][ksize] (zero behind count[i]), xmin [out], count [out]
static void resize_table(int in_size, int out_size, int filter, int ksize, int32_t* kk, int* xmin, int* count) {
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = resize_support(filter) * fs, ss = 1.0 / fs;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        const int n = hi - lo;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            k[x] = resize_filter(filter, (x + lo - center + 0.5) * ss);
            ww += k[x];
        }
        for (int x = 0; x < ksize; ++x) {
            double w = x < n ? k[x] : 0.0;
            if (x < n && ww != 0.0) w /= ww;
            kk[(size_t)xx * ksize + x] = w < 0 ? (int)(-0.5 + w * (1 << 22)) : (int)(0.5 + w * (1 << 22));
        }
        xmin[xx] = lo;
        count[xx] = n;
    }
}

// Device copies of the tables, one per (device, in, out, filter), uploaded on first use and kept for the life of the library.
// The prefetcher's staging thread and the main thread both resize: the map is guarded, and the upload is a blocking copy
// made under the lock, so a table is complete before any launch can name it. in == out is the identity table (one tap of
// weight 1 << 22, which (v << 22 + (1 << 21)) >> 22 = v makes exact): the axis Pillow skips.
struct ResizeTables {
    std::mutex mu;
    std::map<std::tuple<int, int, int, int>, ResizeAxis> axes;
    std::map<std::tuple<int, int, int, int>, std::vector<int>> host;  // xmin then count, for the launcher's tile arithmetic
};
static ResizeTables& resize_tables() {
    static ResizeTables t;
    return t;
}
static int resize_axis(int in_size, int out_size, int filter, ResizeAxis* axis, const int** xmin_host, const int** count_host) {
    int dev = 0;
    ORBIT_HIP_CHECK(hipGetDevice(&dev));
    ResizeTables& t = resize_tables();
    std::lock_guard<std::mutex> lock(t.mu);
    const auto key = std::make_tuple(dev, in_size, out_size, in_size == out_size ? -1 : filter);
    auto it = t.axes.find(key);
    if (it == t.axes.end()) {
        const int ksize = in_size == out_size ? 1 : resize_ksize(in_size, out_size, filter);
        std::vector<int32_t> kk((size_t)out_size * ksize);
        std::vector<int> idx(2 * (size_t)out_size);
        if (in_size == out_size) {
            for (int i = 0; i < out_size; ++i) kk[i] = 1 << 22, idx[i] = i, idx[out_size + i] = 1;
        } else {
            resize_table(in_size, out_size, filter, ksize, kk.data(), idx.data(), idx.data() + out_size);
        }
        std::vector<int32_t> kk_t(kk.size());  // tap-major for the device
        for (int i = 0; i < out_size; ++i)
            for (int k = 0; k < ksize; ++k) kk_t[(size_t)k * out_size + i] = kk[(size_t)i * ksize + k];
        const size_t kk_bytes = kk.size() * sizeof(int32_t), idx_bytes = idx.size() * sizeof(int);
        char* d = nullptr;
        ORBIT_HIP_CHECK(hipMalloc((void**)&d, kk_bytes + idx_bytes));
        hipError_t e = hipMemcpy(d, kk_t.data(), kk_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d + kk_bytes, idx.data(), idx_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return set_err(ORBIT_ERR_HIP, "frames_resize: table upload failed: %s", hipGetErrorString(e));
        }
        ResizeAxis a;
        a.kk = (const int32_t*)d;
        a.xmin = (const int*)(d + kk_bytes);
        a.n = a.xmin + out_size;
        a.out = out_size;
        it = t.axes.emplace(key, a).first;
        t.host.emplace(key, std::move(idx));
    }
    *axis = it->second;
    const std::vector<int>& h = t.host.find(key)->second;  // (map nodes do not move: the pointers outlive the lock)
    *xmin_host = h.data();
    *count_host = h.data() + out_size;
    return ORBIT_OK;
}

}  // namespace orbit

using namespace orbit;

extern "C" {

int orbit_frames_from_uint8(const uint8_t* frames, int layout_hwc, int B, int H, int W, const float* mean3,
                            const float* std3, float* out_nchw, orbit_stream_t stream) {
    ORBIT_REQUIRE(frames && mean3 && std3 && out_nchw, "frames_from_uint8: null pointer");
    ORBIT_REQUIRE(B > 0 && H > 0 && W > 0, "frames_from_uint8: bad sizes");
    ORBIT_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "frames_from_uint8: zero std");
    const size_t total = (size_t)B * H * W;
    size_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    frames_u8_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(frames, layout_hwc, H * W, total, mean3[0], mean3[1],
                                                                  mean3[2], std3[0], std3[1], std3[2], out_nchw);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int orbit_resize_coeffs(int in_size, int out_size, int filter, int* ksize, int32_t* kk, int* xmin, int* count) {
    ORBIT_REQUIRE(in_size > 0 && out_size > 0, "resize_coeffs: bad sizes (in %d, out %d)", in_size, out_size);
    ORBIT_REQUIRE(resize_filter_known(filter), "resize_coeffs: unknown filter %d", filter);
    ORBIT_REQUIRE(ksize, "resize_coeffs: null ksize");
    ORBIT_REQUIRE(in_size <= ORBIT_RESIZE_MAX_SIZE && out_size <= ORBIT_RESIZE_MAX_SIZE,
                  "resize_coeffs: %d -> %d exceeds the limit of %d pixels", in_size, out_size, ORBIT_RESIZE_MAX_SIZE);
    *ksize = resize_ksize(in_size, out_size, filter);
    if (!kk) return ORBIT_OK;
    ORBIT_REQUIRE(xmin && count, "resize_coeffs: null xmin / count");
    resize_table(in_size, out_size, filter, *ksize, kk, xmin, count);
    return ORBIT_OK;
}

// The body of both resize entry points (`who` names the one in the messages): out_u8 set -> the 8-bit store, else normalise
// with mean3 / std3 into out_nchw.
static int frames_resize(const char* who, const uint8_t* frames, int layout_hwc, int B, int H_in, int W_in, int H_out, int W_out,
                         int filter, const float* mean3, const float* std3, float* out_nchw, uint8_t* out_u8, orbit_stream_t stream) {
    ORBIT_REQUIRE(B > 0 && H_in > 0 && W_in > 0 && H_out > 0 && W_out > 0, "%s: bad sizes", who);
    ORBIT_REQUIRE(resize_filter_known(filter), "%s: unknown filter %d", who, filter);
    ORBIT_REQUIRE(out_u8 || (std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f), "%s: zero std", who);
    ORBIT_REQUIRE(H_in <= ORBIT_RESIZE_MAX_SIZE && W_in <= ORBIT_RESIZE_MAX_SIZE && H_out <= ORBIT_RESIZE_MAX_SIZE &&
                      W_out <= ORBIT_RESIZE_MAX_SIZE,
                  "%s: %dx%d -> %dx%d exceeds the limit of %d pixels per side", who, H_in, W_in, H_out, W_out,
                  ORBIT_RESIZE_MAX_SIZE);
    // A tile keeps 3 * RS_TW bytes per input row of its vertical windows in LDS. Where the window of ONE output row cannot fit,
    // no tile can: refused before any table is built or uploaded.
    const int ksize_y = H_in == H_out ? 1 : resize_ksize(H_in, H_out, filter);
    ORBIT_REQUIRE(3 * RS_TW * (size_t)std::min(ksize_y, H_in) < RS_LDS_BYTES,
                  "%s: %d -> %d rows (%s) needs a window of %d rows per output row, more than a tile's LDS "
                  "holds (%d)", who, H_in, H_out, resize_filter_name(filter), std::min(ksize_y, H_in), RS_LDS_BYTES / (3 * RS_TW));
    ResizeAxis ax, ay;
    const int *xmin_x, *n_x, *xmin_y, *n_y;
    int rc = resize_axis(W_in, W_out, filter, &ax, &xmin_x, &n_x);
    if (rc != ORBIT_OK) return rc;
    rc = resize_axis(H_in, H_out, filter, &ay, &xmin_y, &n_y);
    if (rc != ORBIT_OK) return rc;
    // one staged input row: the columns the horizontal windows of a tile's RS_TW output columns cover
    int wc = 0;
    for (int x0 = 0; x0 < W_out; x0 += RS_TW) {
        const int xl = std::min(x0 + RS_TW, W_out) - 1;
        wc = std::max(wc, xmin_x[xl] + n_x[xl] - xmin_x[x0]);
    }
    const int pitch = (int)align_up(layout_hwc ? 3 * (size_t)wc : (size_t)wc, 4), row_bytes = (layout_hwc ? 1 : 3) * pitch;
    // the tallest tile (16, 8, .. 1 output rows) that leaves room for 8 staged rows beside its resampled ones; failing that, one
    // output row per tile with as many staged rows as fit
    int th = RS_TH, span = 0, stage_rows = 0;
    for (;; th /= 2) {
        span = 0;
        for (int y0 = 0; y0 < H_out; y0 += th) {
            const int yl = std::min(y0 + th, H_out) - 1;
            span = std::max(span, xmin_y[yl] + n_y[yl] - xmin_y[y0]);
        }
        const int room = RS_LDS_BYTES - 3 * RS_TW * span;
        stage_rows = room <= 0 ? 0 : std::min(std::min(room / row_bytes, span), RS_RC);
        if (stage_rows >= std::min(span, RS_ROWS) || th == 1) break;
    }
    ORBIT_REQUIRE(stage_rows >= 1,
                  "%s: %dx%d -> %dx%d (%s): the window of one output row (%d rows of %d bytes) and one input "
                  "row of a tile (%d bytes) exceed a tile's %d bytes of LDS", who, H_in, W_in, H_out, W_out, resize_filter_name(filter),
                  span, 3 * RS_TW, row_bytes, RS_LDS_BYTES);
    const int stage_off = 3 * RS_TW * span;
    const size_t lds = (size_t)stage_off + (size_t)stage_rows * row_bytes;
    const int tiles_x = cdiv(W_out, RS_TW), tiles_y = cdiv(H_out, th);
    const int per_frame = tiles_x * tiles_y;  // <= (ORBIT_RESIZE_MAX_SIZE / RS_TW) * ORBIT_RESIZE_MAX_SIZE = RS_MAX_BLOCKS
    const int chunk = RS_MAX_BLOCKS / per_frame;
    hipStream_t s = (hipStream_t)stream;
    const size_t in_frame = 3 * (size_t)H_in * W_in, out_frame = 3 * (size_t)H_out * W_out;
    char name[48];
    snprintf(name, sizeof(name), out_u8 ? "frames_resize_u8<%s>" : "frames_resize<%s>", resize_filter_name(filter));
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const int rec = prof_start(name, 0.0, (double)nb * (in_frame + (out_u8 ? 1.0 : 4.0) * out_frame), s);
        if (out_u8)
            frames_resize_u8_kernel<true><<<nb * per_frame, RS_THREADS, lds, s>>>(
                frames + b0 * in_frame, nb * in_frame, layout_hwc, H_in, W_in, H_out, W_out, th, tiles_x, tiles_y, stage_rows, pitch,
                stage_off, ax, ay, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, nullptr, out_u8 + b0 * out_frame);
        else
            frames_resize_u8_kernel<false><<<nb * per_frame, RS_THREADS, lds, s>>>(
                frames + b0 * in_frame, nb * in_frame, layout_hwc, H_in, W_in, H_out, W_out, th, tiles_x, tiles_y, stage_rows, pitch,
                stage_off, ax, ay, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out_nchw + b0 * out_frame, nullptr);
        prof_stop(rec, s);
        ORBIT_LAUNCH_CHECK();
    }
    return ORBIT_OK;
}

int orbit_frames_resize_from_uint8(const uint8_t* frames, int layout_hwc, int B, int H_in, int W_in, int H_out, int W_out,
                                   int filter, const float* mean3, const float* std3, float* out_nchw, orbit_stream_t stream) {
    ORBIT_REQUIRE(frames && mean3 && std3 && out_nchw, "frames_resize_from_uint8: null pointer");
    return frames_resize("frames_resize_from_uint8", frames, layout_hwc, B, H_in, W_in, H_out, W_out, filter, mean3, std3, out_nchw,
                         nullptr, stream);
}

int orbit_frames_resize_u8(const uint8_t* frames, int layout_hwc, int B, int H_in, int W_in, int H_out, int W_out, int filter,
                           uint8_t* out_u8_hwc, orbit_stream_t stream) {
    ORBIT_REQUIRE(frames && out_u8_hwc, "frames_resize_u8: null pointer");
    return frames_resize("frames_resize_u8", frames, layout_hwc, B, H_in, W_in, H_out, W_out, filter, nullptr, nullptr, nullptr,
                         out_u8_hwc, stream);
}

}  // extern "C"
