// JPEG decode on the device: baseline files in one arena -> 8-bit RGB frames [B][H][W][3], equal to Pillow's decode bit for bit.
// Reference: data/datasets.py:422-431 opens every frame with PIL on the host (libjpeg's default path: Huffman decode, integer
// "islow" inverse DCT, triangle chroma upsampling, table-driven YCbCr -> RGB). The arithmetic of those stages is restated in
// csrc/jpeg_core.h as host + device code; this file is the three kernels around it and the launchers.
//   jpeg_entropy_kernel  one wave per frame. Entropy decoding is sequential inside an image, a task is hundreds of images: the
//                        64 lanes copy the descriptor (Huffman and quantisation tables) into LDS, zero the frame's
//                        coefficients and keep two 1 KB tiles of the byte stream resident in LDS; lane 0 walks the symbols
//                        and scatters the non-zero coefficients, handing control back at every tile end for the next load.
//                        A frame with restart markers where its geometry puts them (2 .. JPEG_PAR_MAX_INTERVALS intervals)
//                        is walked by one lane per restart interval instead, 64 intervals at a time: the wave scans the
//                        segment for markers into an LDS table, lane j decodes intervals j, j + 64, .. from a register window
//                        on the arena; any status sends the frame through the serial walk again, so a damaged file's status
//                        and coefficients do not depend on the form.
//   jpeg_entropy_sub_kernel  launched behind it for the frames WITHOUT restart markers that jpeg_sub_size admits (the first
//                        kernel leaves those alone): one block of 256 threads per frame, one thread per subsequence of the
//                        segment; walkers from guessed states hand their exits on in rounds until nothing changes, a scan gives
//                        block ordinals and DC predictors, a last pass writes the coefficients; a failed check sends the
//                        frame through the same serial walk.
//   jpeg_idct_kernel     one thread per 8 x 8 block: dequantise, both passes of the inverse DCT in registers, range limit.
//   jpeg_color_kernel    one thread per output pixel: chroma upsampling with libjpeg's edge rules, colour conversion, store.
// A frame whose stream is damaged ends with a non-zero status and whatever was decoded so far stays inside its own workspace
// slice: every stream read is bounded by the segment length (itself checked against the arena), every coefficient write by
// the frame's block count (checked against the slice).
#include <algorithm>
#include "common.h"
#include "jpeg_core.h"

namespace orbit {
using namespace orbit_jpeg;

constexpr int JP_STAGE = ORBIT_JPEG_STAGE_BYTES;
constexpr size_t JP_MAX_THREADS = (size_t)1 << 30;  // per launch of the block / pixel kernels; more frames go in another chunk
static_assert(JP_STAGE == 64 * 16, "a tile is one 16-byte load per lane");
static_assert(sizeof(orbit_jpeg_desc_t) % 8 == 0, "descriptors are copied by words and follow each other in an array");

__device__ const uint8_t jpeg_natural_dev[64] = ORBIT_JPEG_NATURAL_ORDER;

// the byte stream as the walker sees it: tiles tile0 and tile0 + 1 from LDS (tile t lives in slot t & 1), anything else - a
// block that runs past both tiles - from memory
struct JpegLdsSrc {
    const uint8_t* lds;
    const uint8_t* mem;
    uint32_t tile0;
    __device__ __forceinline__ uint8_t at(uint32_t pos) const {
        return (pos / JP_STAGE - tile0 < 2u) ? lds[pos & (2 * JP_STAGE - 1)] : mem[pos];
    }
};

// lane's 16 bytes of tile t -> its slot; bytes behind the segment read as zero
__device__ __forceinline__ void jpeg_load_tile(uint8_t* stage, const uint8_t* mem, uint32_t len, uint32_t t, int lane) {
    const uint64_t o = (uint64_t)t * JP_STAGE + 16u * lane;
    uint32_t v[4] = {0, 0, 0, 0};
    if (o + 16 <= len) {
        __builtin_memcpy(v, mem + o, 16);
    } else {
        for (int j = 0; j < 16; ++j)
            if (o + j < len) v[j >> 2] |= (uint32_t)mem[o + j] << (8 * (j & 3));
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(stage + (t & 1u) * JP_STAGE + 16 * lane);
    dst[0] = v[0], dst[1] = v[1], dst[2] = v[2], dst[3] = v[3];
}

// The markers of the segment, for a frame that may take the interval form: the wave reads the segment tile by tile, every lane
// looks through its 16 bytes (and the byte behind them), and the markers' positions go to ends[] in stream order - a marker's
// index is the count of the tiles before plus a prefix count over the ballots of this tile, so no order depends on timing.
// True when the first nseg markers are RST0, RST1, .. (mod 8) and EOI; only ends[0 .. nseg - 1) are used afterwards. The
// result is uniform over the wave. The caller puts a barrier between this and its next use of the staging tiles.
__device__ __forceinline__ bool jpeg_scan_markers(uint8_t* stage, const uint8_t* mem, uint32_t len, int nseg, uint32_t* ends, int lane) {
    const uint32_t ntiles = (len + JP_STAGE - 1) / JP_STAGE;
    int count = 0;  // markers in the tiles before this one (uniform)
    bool bad = false;
    for (uint32_t t = 0; t < ntiles && count < nseg; ++t) {
        jpeg_load_tile(stage, mem, len, t, lane);
        __syncthreads();  // (tile t + 1 goes to the other slot, tile t + 2 comes behind the next barrier)
        const uint8_t* slot = stage + (t & 1u) * JP_STAGE;
        const uint32_t o = t * JP_STAGE + 16u * lane;
        const uint4 q = *reinterpret_cast<const uint4*>(slot + 16 * lane);
        const int n = o >= len ? 0 : (len - o < 16u ? (int)(len - o) : 16);
        int next = -1;
        if (n == 16 && o + 16 < len) next = lane < 63 ? slot[16 * lane + 16] : mem[o + 16];
        const uint32_t m = jpeg_scan_slice(q.x, q.y, q.z, q.w, n, next);
        if (__ballot(m != 0) == 0) continue;
        int before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned long long b = __ballot((m >> j) & 1u);
            before += __popcll(b & ((1ull << lane) - 1ull));
            total += __popcll(b);
        }
        int k = count + before;
        for (uint32_t mm = m; mm != 0; mm &= mm - 1, ++k) {
            const int j = __ffs(mm) - 1;
            if (k >= nseg) break;  // (nseg <= JPEG_PAR_MAX_INTERVALS, the size of ends[])
            const int code = j < 15 ? jpeg_slice_byte(q.x, q.y, q.z, q.w, j + 1) : next;
            if (!jpeg_par_marker_ok(k, code, nseg)) bad = true;
            ends[k] = o + (uint32_t)j;
        }
        count += total;
    }
    return __ballot(bad) == 0 && count >= nseg;
}

// The serial walk of one frame, by a block of T threads: the first 64 keep two tiles of the stream in LDS, thread 0 walks the
// symbols and hands control back at every tile end for the next load. coef: zeroed (a barrier in here comes before the first
// write). Returns the walk's status in thread 0.
template <int T>
__device__ __forceinline__ int jpeg_walk_tiled(uint8_t* stage, uint32_t* ctl, const uint8_t* mem, uint32_t len, const orbit_jpeg_desc_t& d,
                                               const JpegGeom& g, const uint8_t* natural, int16_t* coef, int tid) {
    const bool loader = T == 64 || tid < 64;
    uint32_t tile0 = 0;
    if (loader) {
        jpeg_load_tile(stage, mem, len, 0, tid);
        jpeg_load_tile(stage, mem, len, 1, tid);
    }
    JpegWalk w;
    jpeg_walk_init(w, d);
    __syncthreads();
    for (;;) {
        if (tid == 0) {
            const JpegLdsSrc src{stage, mem, tile0};
            jpeg_walk(w, src, d, g, natural, coef, (tile0 + 1) * JP_STAGE - 1);
            ctl[0] = (uint32_t)w.done;
            ctl[1] = w.bits.pos;
        }
        __syncthreads();
        const uint32_t done = ctl[0], next = ctl[1] / JP_STAGE;  // next > tile0 unless done
        if (done) break;
        if (loader) {
            if (next != tile0 + 1) jpeg_load_tile(stage, mem, len, next, tid);
            jpeg_load_tile(stage, mem, len, next + 1, tid);
        }
        tile0 = next;
        __syncthreads();
    }
    return w.status;
}

// form: 0 walks every frame serially, 1 takes the interval form where the rule of csrc/jpeg_core.h holds. sub: < 0, or the
// sub_bytes of the jpeg_entropy_sub_kernel launched behind this one, whose frames (jpeg_sub_size) are left alone here. taken
// (nullable): 0 serial, 1 interval-parallel, 2 parallel attempted, then walked serially.
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ arena, size_t arena_bytes,
                                                          const orbit_jpeg_desc_t* __restrict__ descs, int H, int W,
                                                          size_t cap_blocks, int16_t* __restrict__ coef_ws,
                                                          int32_t* __restrict__ status, int form, int sub,
                                                          int32_t* __restrict__ taken) {
    __shared__ __align__(16) orbit_jpeg_desc_t d;
    __shared__ __align__(16) uint8_t stage[2 * JP_STAGE];
    __shared__ uint8_t natural[64];
    __shared__ uint32_t ctl[2];
    __shared__ uint32_t ends[JPEG_PAR_MAX_INTERVALS];
    const int f = blockIdx.x, lane = threadIdx.x;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(descs + f);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&d);
        for (int i = lane; i < (int)(sizeof(orbit_jpeg_desc_t) / 4); i += 64) dst[i] = src[i];
        natural[lane] = jpeg_natural_dev[lane];
    }
    __syncthreads();
    if (taken && lane == 0) taken[f] = 0;
    if (d.status != 0) {  // the host decodes this frame
        if (lane == 0) status[f] = d.status > 0 ? -d.status : d.status;
        return;
    }
    JpegGeom g;
    const bool ok = jpeg_geom(d, g) && d.width == W && d.height == H && (size_t)g.total_blocks <= cap_blocks &&
                    d.file_offset <= arena_bytes && (uint64_t)d.ecs_offset + d.ecs_bytes <= arena_bytes - d.file_offset;
    if (!ok) {
        if (lane == 0) status[f] = ORBIT_JPEG_ST_DESC;
        return;
    }
    if (jpeg_sub_size(d, sub) != 0) return;  // jpeg_entropy_sub_kernel's frame (sub < 0: there is none)
    int16_t* coef = coef_ws + (size_t)f * cap_blocks * 64;
    {
        uint4* z = reinterpret_cast<uint4*>(coef);  // (the slice starts at a multiple of 128 bytes)
        for (int i = lane; i < g.total_blocks * 8; i += 64) z[i] = make_uint4(0, 0, 0, 0);
    }
    const uint8_t* mem = arena + d.file_offset + d.ecs_offset;
    const uint32_t len = d.ecs_bytes;
    const int nseg = form ? jpeg_par_intervals(d, g) : 0;
    if (nseg != 0) {  // (uniform: the descriptor is in LDS)
        const bool valid = jpeg_scan_markers(stage, mem, len, nseg, ends, lane);
        __syncthreads();  // ends[] is complete, the zeroes are written, nobody reads the tiles any more
        if (valid) {
            int st = 0;
            for (int k = lane; k < nseg; k += 64) st |= jpeg_walk_interval(k, nseg, ends, mem, d, g, natural, coef);
            if (__ballot(st != 0) == 0) {
                if (lane == 0) {
                    status[f] = 0;
                    if (taken) taken[f] = 1;
                }
                return;
            }
            // a damaged file: its status and coefficients are the serial walk's
            if (taken && lane == 0) taken[f] = 2;
            __syncthreads();
            uint4* z = reinterpret_cast<uint4*>(coef);
            for (int i = lane; i < g.total_blocks * 8; i += 64) z[i] = make_uint4(0, 0, 0, 0);
        }
    }
    const int st = jpeg_walk_tiled<64>(stage, ctl, mem, len, d, g, natural, coef, lane);
    if (lane == 0) status[f] = st;
}

// The subsequence-parallel form (csrc/jpeg_core.h) for the frames without restart markers that jpeg_sub_size admits; every
// other frame of the launch is jpeg_entropy_kernel's and returns at once. One block of JP_SUB_THREADS threads per frame, the
// threads striding over the N subsequences; the table of N rows lives in LDS. A round is: walk what changed, barrier, hand the
// exits over, barrier - so entries are read from the round before - until a round walks nothing, at most N rounds. Then the
// exclusive scan over blocks and DC sums (a run of consecutive rows per thread, the runs' sums through LDS), the checks, the
// write pass, and on any failure the serial walk of jpeg_entropy_kernel over the zeroed frame. rounds (nullable): rounds taken.
constexpr int JP_SUB_THREADS = JPEG_SUB_PER_ROUND;
static_assert(JP_SUB_THREADS == 256 && JPEG_SUB_MAX % JP_SUB_THREADS == 0, "the production rule sizes S by the block's width");

__global__ __launch_bounds__(JP_SUB_THREADS) void jpeg_entropy_sub_kernel(const uint8_t* __restrict__ arena, size_t arena_bytes,
                                                                          const orbit_jpeg_desc_t* __restrict__ descs, int H, int W,
                                                                          size_t cap_blocks, int16_t* __restrict__ coef_ws,
                                                                          int32_t* __restrict__ status, int sub, int32_t* __restrict__ taken,
                                                                          int32_t* __restrict__ rounds) {
    constexpr int T = JP_SUB_THREADS;
    __shared__ __align__(16) orbit_jpeg_desc_t d;
    __shared__ __align__(16) uint8_t stage[2 * JP_STAGE];
    __shared__ uint8_t natural[64];
    __shared__ uint32_t ctl[2];
    __shared__ __align__(16) JpegSubRow rows[JPEG_SUB_MAX];
    __shared__ uint4 part[T];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (rounds && tid == 0) rounds[f] = 0;
    // the other kernel's frame: three words of the descriptor say so, before anything is copied (a launch of restart-marked
    // frames then costs little more than the launch itself)
    if (descs[f].status != 0 || jpeg_sub_size(descs[f], sub) == 0) return;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(descs + f);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&d);
        for (int i = tid; i < (int)(sizeof(orbit_jpeg_desc_t) / 4); i += T) dst[i] = src[i];
        if (tid < 64) natural[tid] = jpeg_natural_dev[tid];
    }
    __syncthreads();
    JpegGeom g;
    // (what jpeg_entropy_kernel checks, and answers in status[] when it does not hold)
    if (d.status != 0 || !jpeg_geom(d, g) || d.width != W || d.height != H || (size_t)g.total_blocks > cap_blocks ||
        d.file_offset > arena_bytes || (uint64_t)d.ecs_offset + d.ecs_bytes > arena_bytes - d.file_offset)
        return;
    const uint32_t S = jpeg_sub_size(d, sub);
    if (S == 0) return;  // (uniform: the descriptor is in LDS)
    const int N = jpeg_sub_count(d, S);  // 2 .. JPEG_SUB_MAX
    int16_t* coef = coef_ws + (size_t)f * cap_blocks * 64;
    uint4* z = reinterpret_cast<uint4*>(coef);  // (the slice starts at a multiple of 128 bytes)
    for (int i = tid; i < g.total_blocks * 8; i += T) z[i] = make_uint4(0, 0, 0, 0);
    const uint8_t* mem = arena + d.file_offset + d.ecs_offset;
    const uint32_t len = d.ecs_bytes;
    for (int i = tid; i < N; i += T) {
        rows[i].entry = jpeg_sub_guess(mem, len, S, i);
        rows[i].exit.pos = 0, rows[i].exit.st = 0;
        rows[i].blocks = rows[i].dc0 = rows[i].dc1 = rows[i].dc2 = 0;
    }
    int nrounds = 0;
    while (nrounds < N) {
        __syncthreads();
        int walked = 0;
        for (int i = tid; i < N; i += T)
            if (rows[i].entry.st & JPEG_SUB_CHANGED) {
                rows[i].entry.st &= ~JPEG_SUB_CHANGED;
                jpeg_sub_walk<false>(rows[i], (uint32_t)(i + 1) * S, mem, d, g, natural, nullptr);
                walked = 1;
            }
        if (!__syncthreads_or(walked)) break;
        ++nrounds;
        for (int i = tid; i + 1 < N; i += T) jpeg_sub_hand_over(rows[i], rows[i + 1]);
    }
    __syncthreads();
    // exclusive scan: thread t owns rows t * run .. ; part[t] = their sums
    const int run = (N + T - 1) / T, first = tid * run;
    uint4 own = make_uint4(0, 0, 0, 0);
    for (int i = first; i < first + run && i < N; ++i) own.x += rows[i].blocks, own.y += rows[i].dc0, own.z += rows[i].dc1, own.w += rows[i].dc2;
    part[tid] = own;
    __syncthreads();
    uint4 at = make_uint4(0, 0, 0, 0);
    uint32_t total = 0;
    for (int u = 0; u < T; ++u) {
        const uint4 p = part[u];
        if (u < tid) at.x += p.x, at.y += p.y, at.z += p.z, at.w += p.w;
        total += p.x;
    }
    const int bpm = jpeg_sub_blocks_per_mcu(d);
    int bad = 0;
    for (int i = first; i < first + run && i < N; ++i) {
        const uint4 r = make_uint4(rows[i].blocks, rows[i].dc0, rows[i].dc1, rows[i].dc2);
        rows[i].blocks = at.x, rows[i].dc0 = at.y, rows[i].dc1 = at.z, rows[i].dc2 = at.w;
        at.x += r.x, at.y += r.y, at.z += r.z, at.w += r.w;
        if (!jpeg_sub_row_ok(rows[i], bpm)) bad = 1;
    }
    if (tid == 0 && (total != (uint32_t)g.total_blocks || !jpeg_sub_last_ok(rows[N - 1].exit, mem, len))) bad = 1;
    if (!__syncthreads_or(bad)) {
        int st = 0;
        for (int i = tid; i < N; i += T) st |= jpeg_sub_walk<true>(rows[i], (uint32_t)(i + 1) * S, mem, d, g, natural, coef);
        if (!__syncthreads_or(st)) {
            if (tid == 0) {
                status[f] = 0;
                if (taken) taken[f] = 3;
                if (rounds) rounds[f] = nrounds;
            }
            return;
        }
    }
    // a damaged file: its status and coefficients are the serial walk's
    if (tid == 0) {
        if (taken) taken[f] = 4;
        if (rounds) rounds[f] = nrounds;
    }
    for (int i = tid; i < g.total_blocks * 8; i += T) z[i] = make_uint4(0, 0, 0, 0);
    const int st = jpeg_walk_tiled<T>(stage, ctl, mem, len, d, g, natural, coef, tid);
    if (tid == 0) status[f] = st;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const orbit_jpeg_desc_t* __restrict__ descs, size_t cap_blocks, size_t total,
                                                        const int16_t* __restrict__ coef_ws, uint8_t* __restrict__ plane_ws,
                                                        int32_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t f = i / cap_blocks;
    const int j = (int)(i - f * cap_blocks);
    if (status[f] != 0) return;
    const orbit_jpeg_desc_t& d = descs[f];
    JpegGeom g;
    if (!jpeg_geom(d, g) || j >= g.total_blocks) return;  // (the entropy kernel has vouched for the descriptor)
    const int c = (d.ncomp == 3 && j >= g.base[2]) ? 2 : ((d.ncomp == 3 && j >= g.base[1]) ? 1 : 0);
    const int wbc = c == 0 ? g.wb[0] : (c == 1 ? g.wb[1] : g.wb[2]), basec = c == 0 ? g.base[0] : (c == 1 ? g.base[1] : g.base[2]);
    const int k = j - basec, by = k / wbc, bx = k - by * wbc;
    const size_t pitch = (size_t)wbc * 8;
    uint8_t* out = plane_ws + f * cap_blocks * 64 + (size_t)basec * 64 + (size_t)by * 8 * pitch + (size_t)bx * 8;
    const int flag = jpeg_idct_block(coef_ws + (f * cap_blocks + j) * 64, d.qt[c], out, pitch);
    if (flag) atomicOr(status + f, flag);
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const orbit_jpeg_desc_t* __restrict__ descs, size_t cap_blocks, int H, int W,
                                                         size_t total, const uint8_t* __restrict__ plane_ws,
                                                         const int32_t* __restrict__ status, uint8_t* __restrict__ out) {
    const size_t HW = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t f = i / HW, p = i - f * HW;
        if (status[f] != 0) continue;
        const orbit_jpeg_desc_t& d = descs[f];
        JpegGeom g;
        if (!jpeg_geom(d, g)) continue;
        const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
        uint8_t rgb[3];
        jpeg_rgb_at(d, g, plane_ws + f * cap_blocks * 64, x, y, rgb);
        uint8_t* o = out + i * 3;
        o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
    }
}

static size_t jpeg_frame_workspace(int H, int W) { return jpeg_cap_blocks(H, W) * 64 * (sizeof(int16_t) + 1); }

}  // namespace orbit

using namespace orbit;

extern "C" {

int orbit_jpeg_parse(const uint8_t* data, size_t bytes, orbit_jpeg_desc_t* desc, size_t desc_bytes) {
    ORBIT_REQUIRE(desc, "jpeg_parse: null descriptor");
    ORBIT_REQUIRE(desc_bytes == sizeof(orbit_jpeg_desc_t), "jpeg_parse: the descriptor is %zu bytes, the caller's %zu",
                  sizeof(orbit_jpeg_desc_t), desc_bytes);
    char msg[160];
    const int rc = orbit_jpeg::jpeg_parse(data, bytes, desc, msg, sizeof(msg));
    if (rc < 0) return set_err(ORBIT_ERR_ARG, "%s", msg);
    return rc;
}

size_t orbit_jpeg_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || H > ORBIT_RESIZE_MAX_SIZE || W > ORBIT_RESIZE_MAX_SIZE) return 0;
    return (size_t)B * jpeg_frame_workspace(H, W);
}

int orbit_frames_from_jpeg(const uint8_t* arena, size_t arena_bytes, const orbit_jpeg_desc_t* descs, int B, int H, int W,
                           uint8_t* out_u8_hwc, int32_t* status, void* workspace, size_t workspace_bytes, orbit_stream_t stream) {
    ORBIT_REQUIRE(arena && descs && out_u8_hwc && status && workspace, "frames_from_jpeg: null pointer");
    ORBIT_REQUIRE(B > 0 && H > 0 && W > 0, "frames_from_jpeg: bad sizes");
    ORBIT_REQUIRE(H <= ORBIT_RESIZE_MAX_SIZE && W <= ORBIT_RESIZE_MAX_SIZE, "frames_from_jpeg: %dx%d exceeds the limit of %d pixels per side",
                  H, W, ORBIT_RESIZE_MAX_SIZE);
    ORBIT_REQUIRE(arena_bytes > 0, "frames_from_jpeg: empty arena");
    ORBIT_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)descs & 7) == 0, "frames_from_jpeg: workspace must be 16-byte aligned, descs 8-byte");
    const size_t per_frame = jpeg_frame_workspace(H, W), cap_blocks = jpeg_cap_blocks(H, W);
    ORBIT_REQUIRE(workspace_bytes >= per_frame, "frames_from_jpeg: workspace of %zu bytes, one %dx%d frame needs %zu", workspace_bytes, H,
                  W, per_frame);
    const size_t by_threads = std::max<size_t>(1, JP_MAX_THREADS / std::max(cap_blocks, (size_t)H * W));
    const int chunk = (int)std::min<size_t>(std::min(workspace_bytes / per_frame, by_threads), (size_t)B);
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        int16_t* coef = (int16_t*)workspace;
        uint8_t* planes = (uint8_t*)workspace + (size_t)nb * cap_blocks * 64 * sizeof(int16_t);
        int rec = prof_start("jpeg_entropy", 0.0, (double)nb * cap_blocks * 64 * sizeof(int16_t), s);
        jpeg_entropy_kernel<<<nb, 64, 0, s>>>(arena, arena_bytes, descs + b0, H, W, cap_blocks, coef, status + b0, 1, 0, nullptr);
        jpeg_entropy_sub_kernel<<<nb, JP_SUB_THREADS, 0, s>>>(arena, arena_bytes, descs + b0, H, W, cap_blocks, coef, status + b0, 0, nullptr,
                                                              nullptr);
        prof_stop(rec, s);
        ORBIT_LAUNCH_CHECK();
        const size_t blocks = (size_t)nb * cap_blocks;
        rec = prof_start("jpeg_idct", 0.0, (double)blocks * 64 * 3, s);
        jpeg_idct_kernel<<<(unsigned)((blocks + 255) / 256), 256, 0, s>>>(descs + b0, cap_blocks, blocks, coef, planes, status + b0);
        prof_stop(rec, s);
        ORBIT_LAUNCH_CHECK();
        const size_t pixels = (size_t)nb * H * W;
        rec = prof_start("jpeg_color", 0.0, (double)pixels * 6, s);
        jpeg_color_kernel<<<(unsigned)std::min<size_t>((pixels + 255) / 256, 1u << 20), 256, 0, s>>>(
            descs + b0, cap_blocks, H, W, pixels, planes, status + b0, out_u8_hwc + (size_t)b0 * H * W * 3);
        prof_stop(rec, s);
        ORBIT_LAUNCH_CHECK();
    }
    return ORBIT_OK;
}

int orbit_op_jpeg_entropy(const uint8_t* arena, size_t arena_bytes, const orbit_jpeg_desc_t* descs, int B, int H, int W, int form,
                          int16_t* coef_out, size_t coef_bytes, int32_t* status, int32_t* taken, orbit_stream_t stream) {
    ORBIT_REQUIRE(arena && descs && coef_out && status && taken, "op_jpeg_entropy: null pointer");
    ORBIT_REQUIRE(B > 0 && H > 0 && W > 0, "op_jpeg_entropy: bad sizes");
    ORBIT_REQUIRE(H <= ORBIT_RESIZE_MAX_SIZE && W <= ORBIT_RESIZE_MAX_SIZE, "op_jpeg_entropy: %dx%d exceeds the limit of %d pixels per side", H,
                  W, ORBIT_RESIZE_MAX_SIZE);
    ORBIT_REQUIRE(form == 0 || form == 1, "op_jpeg_entropy: form %d (0 = serial, 1 = one lane per restart interval)", form);
    ORBIT_REQUIRE(arena_bytes > 0, "op_jpeg_entropy: empty arena");
    ORBIT_REQUIRE(((uintptr_t)coef_out & 15) == 0 && ((uintptr_t)descs & 7) == 0, "op_jpeg_entropy: coef_out must be 16-byte aligned, descs 8-byte");
    const size_t cap_blocks = jpeg_cap_blocks(H, W), need = (size_t)B * cap_blocks * 64 * sizeof(int16_t);
    ORBIT_REQUIRE(coef_bytes >= need, "op_jpeg_entropy: coef_out of %zu bytes, %d frames of %dx%d need %zu", coef_bytes, B, H, W, need);
    hipStream_t s = (hipStream_t)stream;
    jpeg_entropy_kernel<<<B, 64, 0, s>>>(arena, arena_bytes, descs, H, W, cap_blocks, coef_out, status, form, -1, taken);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int orbit_op_jpeg_entropy_sub(const uint8_t* arena, size_t arena_bytes, const orbit_jpeg_desc_t* descs, int B, int H, int W, int sub_bytes,
                              int16_t* coef_out, size_t coef_bytes, int32_t* status, int32_t* taken, int32_t* rounds, orbit_stream_t stream) {
    ORBIT_REQUIRE(arena && descs && coef_out && status && taken && rounds, "op_jpeg_entropy_sub: null pointer");
    ORBIT_REQUIRE(B > 0 && H > 0 && W > 0, "op_jpeg_entropy_sub: bad sizes");
    ORBIT_REQUIRE(H <= ORBIT_RESIZE_MAX_SIZE && W <= ORBIT_RESIZE_MAX_SIZE, "op_jpeg_entropy_sub: %dx%d exceeds the limit of %d pixels per side",
                  H, W, ORBIT_RESIZE_MAX_SIZE);
    ORBIT_REQUIRE(sub_bytes == 0 || sub_bytes >= 4, "op_jpeg_entropy_sub: sub_bytes %d (0 = the production rule, or at least 4)", sub_bytes);
    ORBIT_REQUIRE(arena_bytes > 0, "op_jpeg_entropy_sub: empty arena");
    ORBIT_REQUIRE(((uintptr_t)coef_out & 15) == 0 && ((uintptr_t)descs & 7) == 0,
                  "op_jpeg_entropy_sub: coef_out must be 16-byte aligned, descs 8-byte");
    const size_t cap_blocks = jpeg_cap_blocks(H, W), need = (size_t)B * cap_blocks * 64 * sizeof(int16_t);
    ORBIT_REQUIRE(coef_bytes >= need, "op_jpeg_entropy_sub: coef_out of %zu bytes, %d frames of %dx%d need %zu", coef_bytes, B, H, W, need);
    hipStream_t s = (hipStream_t)stream;
    jpeg_entropy_kernel<<<B, 64, 0, s>>>(arena, arena_bytes, descs, H, W, cap_blocks, coef_out, status, 1, sub_bytes, taken);
    ORBIT_LAUNCH_CHECK();
    jpeg_entropy_sub_kernel<<<B, JP_SUB_THREADS, 0, s>>>(arena, arena_bytes, descs, H, W, cap_blocks, coef_out, status, sub_bytes, taken, rounds);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

}  // extern "C"
