// JPEG encode on the device: 8-bit RGB frames [B][H][W][3] -> the baseline 4:2:0 files Pillow's Image.save(quality=q) writes for
// them, byte for byte. Reference: scripts/resize_videos.py:46-47 saves every resized frame with PIL on host threads. The
// arithmetic is csrc/jpeg_enc_core.h (host + device); this file is the kernels around it and the launcher. Encoding has no
// serial symbol walk: every stage is a wide launch over pixels, blocks or bytes, with one prefix sum per frame between them.
//   enc_color_kernel     one thread per 8 x 2 pixels: colour conversion and 2 x 2 chroma averaging into padded Y / Cb / Cr planes.
//   enc_dct_kernel       one thread per 8 x 8 block of the scan (MCU-major, six per MCU, dummy blocks included): forward DCT and
//                        quantisation in registers, 64 int16 in zigzag order.
//   enc_size_kernel      one thread per block: the bits it codes to (its DC predictor is found by index arithmetic).
//   enc_scan_kernel      one workgroup per frame: inclusive sum of those bits, first byte of every restart interval (each
//                        rounded up to whole bytes), and the zeroing of the part of the bit buffer the frame will use.
//   enc_pack_kernel      one thread per block: its codes at its bit offset. Whole words are stored; the first and the last
//                        word, which neighbours share, are OR-ed in atomically (OR commutes: the result is deterministic).
//   enc_ff_kernel        one workgroup per frame: FF bytes in front of every 32-byte chunk of the unstuffed stream, and in all of it.
//   enc_assemble_kernel  one thread per chunk: stuffed bytes and restart markers to their final place; one workgroup per
//                        frame writes header, COM segment, EOI and the file's length.
// Integer arithmetic only; the one atomic is the OR above. Every index into a frame's workspace slice and output slice is
// bounded by quantities the host derived from H and W alone (enc_layout, enc_bound), not by pixel content.
#include <algorithm>
#include "common.h"
#include "jpeg_enc_core.h"

namespace orbit {
using namespace orbit_jpegenc;

constexpr int ENC_MAX_FRAMES = 512;  // per launch: their comment offsets travel as a kernel argument

struct EncQuantArg {
    uint32_t q[2][64], recip[2][64];
};
struct EncHuffArg {
    uint32_t dc[2][16], ac[2][256];
};
struct EncHeadArg {
    uint8_t head[20];
    uint8_t tail[ENC_HEADER_MAX - 20];
    uint32_t tail_len;
    uint32_t com_off[ENC_MAX_FRAMES + 1];
};
static_assert(sizeof(EncHeadArg) + 128 <= 4096 && sizeof(EncHuffArg) + 128 <= 4096, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(256) void enc_color_kernel(const uint8_t* __restrict__ frames, EncGeom g, size_t total,
                                                        uint8_t* __restrict__ ws, EncLayout l) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int sxn = 2 * g.mcux, qyn = 8 * g.mcuy;
    const size_t per_frame = (size_t)sxn * qyn;
    const size_t f = i / per_frame;
    const int j = (int)(i - f * per_frame), qy = j / sxn, sx = j - qy * sxn;
    const uint8_t* rgb = frames + f * (size_t)g.H * g.W * 3;
    uint32_t ylo[2], yhi[2], cb4, cr4;
    enc_strip_at(rgb, g.H, g.W, sx, qy, ylo, yhi, cb4, cr4);
    uint8_t* w = ws + f * l.total;
    const size_t ypitch = 16 * (size_t)g.mcux, cpitch = 8 * (size_t)g.mcux;
    *reinterpret_cast<uint2*>(w + l.y + (size_t)(2 * qy) * ypitch + 8 * sx) = make_uint2(ylo[0], ylo[1]);
    *reinterpret_cast<uint2*>(w + l.y + (size_t)(2 * qy + 1) * ypitch + 8 * sx) = make_uint2(yhi[0], yhi[1]);
    *reinterpret_cast<uint32_t*>(w + l.cb + (size_t)qy * cpitch + 4 * sx) = cb4;
    *reinterpret_cast<uint32_t*>(w + l.cr + (size_t)qy * cpitch + 4 * sx) = cr4;
}

__global__ __launch_bounds__(256) void enc_dct_kernel(EncGeom g, size_t total, uint8_t* __restrict__ ws, EncLayout l, EncQuantArg qa) {
    __shared__ uint32_t s_q[2][64], s_r[2][64];
    if (threadIdx.x < 128) {
        s_q[threadIdx.x >> 6][threadIdx.x & 63] = qa.q[threadIdx.x >> 6][threadIdx.x & 63];
        s_r[threadIdx.x >> 6][threadIdx.x & 63] = qa.recip[threadIdx.x >> 6][threadIdx.x & 63];
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t f = i / g.blocks;
    const int blk = (int)(i - f * g.blocks);
    EncBlockPos p = enc_block_pos(g, blk);
    const bool dummy = p.dummy;
    for (int b = blk; p.dummy;) p = enc_block_pos(g, --b);  // a dummy block takes the DC of the block before it (Y00 is never one)
    uint8_t* w = ws + f * l.total;
    const size_t pitch = (p.comp == 0 ? 16 : 8) * (size_t)g.mcux;
    const uint8_t* in = w + (p.comp == 0 ? l.y : (p.comp == 1 ? l.cb : l.cr)) + (size_t)p.by * 8 * pitch + (size_t)p.bx * 8;
    const int t = p.comp == 0 ? 0 : 1;
    int16_t zz[64];
    enc_fdct_block(in, pitch, s_q[t], s_r[t], zz);
    uint4* out = reinterpret_cast<uint4*>(w + l.coef + (size_t)blk * 128);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            v[e] = (dummy && (k | e)) ? 0u : ((uint32_t)(uint16_t)zz[8 * k + 2 * e] | (dummy ? 0u : (uint32_t)(uint16_t)zz[8 * k + 2 * e + 1] << 16));
        out[k] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

__device__ __forceinline__ void enc_load_huff(const EncHuffArg& ha, uint32_t* s_dc, uint32_t* s_ac) {
    for (int i = threadIdx.x; i < 32; i += blockDim.x) s_dc[i] = ha.dc[i >> 4][i & 15];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) s_ac[i] = ha.ac[i >> 8][i & 255];
    __syncthreads();
}

__global__ __launch_bounds__(256) void enc_size_kernel(EncGeom g, size_t total, uint8_t* __restrict__ ws, EncLayout l, EncHuffArg ha) {
    __shared__ uint32_t s_dc[32], s_ac[512];
    enc_load_huff(ha, s_dc, s_ac);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t f = i / g.blocks;
    const int blk = (int)(i - f * g.blocks);
    uint8_t* w = ws + f * l.total;
    reinterpret_cast<uint32_t*>(w + l.sums)[blk] = enc_block_bits(g, blk, reinterpret_cast<const int16_t*>(w + l.coef), s_dc, s_ac);
}

// inclusive sum over the 256 threads of a block; *total receives the sum of all. wsum: 4 words of LDS.
__device__ __forceinline__ uint32_t enc_block_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    __syncthreads();  // wsum of the previous call has been read
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    uint32_t add = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < wave) add += wsum[k];
        all += wsum[k];
    }
    *total = all;
    return v + add;
}

__global__ __launch_bounds__(256) void enc_scan_kernel(EncGeom g, uint8_t* __restrict__ ws, EncLayout l) {
    __shared__ uint32_t wsum[4];
    uint8_t* w = ws + (size_t)blockIdx.x * l.total;
    uint32_t* sums = reinterpret_cast<uint32_t*>(w + l.sums);
    uint32_t* seg = reinterpret_cast<uint32_t*>(w + l.seg);
    uint32_t carry = 0;
    for (int b0 = 0; b0 < g.blocks; b0 += 1024) {  // four blocks per thread: (g.blocks is a multiple of 6, not of 4)
        const int i = b0 + 4 * (int)threadIdx.x;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i + k < g.blocks ? sums[i + k] : 0u;
        v[1] += v[0], v[2] += v[1], v[3] += v[2];
        uint32_t all;
        const uint32_t before = carry + enc_block_scan(v[3], wsum, &all) - v[3];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < g.blocks) sums[i + k] = before + v[k];
        carry += all;
    }
    __syncthreads();  // the sums are visible to the whole workgroup
    carry = 0;
    for (int s0 = 0; s0 < g.nseg; s0 += 256) {
        const int s = s0 + (int)threadIdx.x;
        const uint32_t v = s < g.nseg ? enc_seg_bytes(g, sums, s) : 0u;
        uint32_t all;
        const uint32_t incl = enc_block_scan(v, wsum, &all);
        if (s < g.nseg) seg[s] = carry + incl - v;
        carry += all;
    }
    if (threadIdx.x == 0) seg[g.nseg] = carry;
    // the words the frame's bits will be OR-ed into: carry <= enc_unstuffed_cap by the bound of a block's bits
    const uint32_t cap_words = (uint32_t)(enc_unstuffed_cap(g.blocks) / 4);
    const uint32_t words = min(carry / 4 + 1, cap_words);
    uint4* z = reinterpret_cast<uint4*>(w + l.bits);
    for (uint32_t k = threadIdx.x; k < (words + 3) / 4; k += 256) z[k] = make_uint4(0, 0, 0, 0);  // (cap_words is a multiple of 4)
}

struct EncDeviceMem {
    uint32_t* buf;
    __device__ __forceinline__ void or_word(uint32_t i, uint32_t v) const { atomicOr(buf + i, v); }
    __device__ __forceinline__ void set_word(uint32_t i, uint32_t v) const { buf[i] = v; }
};

__global__ __launch_bounds__(256) void enc_pack_kernel(EncGeom g, size_t total, uint8_t* __restrict__ ws, EncLayout l, EncHuffArg ha) {
    __shared__ uint32_t s_dc[32], s_ac[512];
    enc_load_huff(ha, s_dc, s_ac);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t f = i / g.blocks;
    const int blk = (int)(i - f * g.blocks);
    uint8_t* w = ws + f * l.total;
    enc_pack_block(g, blk, reinterpret_cast<const int16_t*>(w + l.coef), reinterpret_cast<const uint32_t*>(w + l.sums),
                   reinterpret_cast<const uint32_t*>(w + l.seg), s_dc, s_ac, EncDeviceMem{reinterpret_cast<uint32_t*>(w + l.bits)});
}

__device__ __forceinline__ uint32_t enc_header_len(const EncHeadArg& h, int f) {
    const uint32_t clen = h.com_off[f + 1] - h.com_off[f];
    return 20u + (clen ? 4u + clen : 0u) + h.tail_len;
}

__global__ __launch_bounds__(256) void enc_ff_kernel(EncGeom g, uint8_t* __restrict__ ws, EncLayout l) {
    __shared__ uint32_t wsum[4];
    uint8_t* w = ws + (size_t)blockIdx.x * l.total;
    const uint32_t total = reinterpret_cast<const uint32_t*>(w + l.seg)[g.nseg];
    const uint8_t* bits = w + l.bits;
    uint32_t* ff = reinterpret_cast<uint32_t*>(w + l.ff);
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < total; c0 += 256 * ENC_CHUNK) {
        const uint32_t a = c0 + ENC_CHUNK * threadIdx.x;
        const uint32_t v = a < total ? enc_count_ff(bits, a, min(a + ENC_CHUNK, total)) : 0u;
        uint32_t all;
        const uint32_t incl = enc_block_scan(v, wsum, &all);
        if (a < total) ff[a / ENC_CHUNK] = carry + incl - v;
        carry += all;
    }
    if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(w + l.seg)[g.nseg + 1] = carry;  // all FF bytes of the stream
}

// grid (1 + chunk blocks, frames): block x = 0 writes the frame's header and EOI, the others stuff 256 chunks each
__global__ __launch_bounds__(256) void enc_assemble_kernel(EncGeom g, const uint8_t* __restrict__ ws, EncLayout l, EncHeadArg h,
                                                           const uint8_t* __restrict__ comments, uint8_t* __restrict__ out,
                                                           size_t out_stride, uint32_t* __restrict__ out_bytes) {
    const int f = blockIdx.y;
    const uint8_t* w = ws + (size_t)f * l.total;
    uint8_t* o = out + (size_t)f * out_stride;
    const uint32_t* seg = reinterpret_cast<const uint32_t*>(w + l.seg);
    const uint32_t total = seg[g.nseg];
    const uint32_t clen = h.com_off[f + 1] - h.com_off[f], hlen = enc_header_len(h, f);
    if (blockIdx.x == 0) {
        const uint32_t com = clen ? 4u + clen : 0u;
        for (uint32_t i = threadIdx.x; i < hlen; i += 256) {
            uint8_t v;
            if (i < 20) v = h.head[i];
            else if (i >= 20 + com) v = h.tail[i - 20 - com];
            else if (i == 20) v = 0xFF;
            else if (i == 21) v = 0xFE;
            else if (i == 22) v = (uint8_t)((clen + 2) >> 8);
            else if (i == 23) v = (uint8_t)(clen + 2);
            else v = comments[h.com_off[f] + (i - 24)];
            o[i] = v;
        }
        if (threadIdx.x == 0) {
            // header, stuffed scan, a marker between intervals, EOI: <= out_stride, which the launcher checked against enc_bound
            const uint32_t n = hlen + total + seg[g.nseg + 1] + 2u * (uint32_t)(g.nseg - 1) + 2u;
            o[n - 2] = 0xFF, o[n - 1] = 0xD9;
            out_bytes[f] = n;
        }
        return;
    }
    const uint32_t c = (blockIdx.x - 1) * 256 + threadIdx.x;
    if ((uint64_t)c * ENC_CHUNK >= total) return;
    const uint32_t c0 = c * ENC_CHUNK;
    enc_stuff_chunk(w + l.bits, c0, min(c0 + ENC_CHUNK, total), reinterpret_cast<const uint32_t*>(w + l.ff)[c], seg, g.nseg, o + hlen);
}

// one workgroup per file: its offset is the sum of the lengths in front of it
__global__ __launch_bounds__(256) void jpeg_compact_kernel(const uint8_t* __restrict__ out, size_t out_stride,
                                                           const uint32_t* __restrict__ out_bytes, int B, uint8_t* __restrict__ packed,
                                                           size_t packed_cap, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t wsum[4];
    const int f = blockIdx.x;
    uint32_t v = 0;
    for (int i = threadIdx.x; i < f; i += 256) v += out_bytes[i];
    uint32_t off;
    enc_block_scan(v, wsum, &off);
    const uint32_t n = out_bytes[f];
    if (threadIdx.x == 0) {
        offsets[f] = off;
        if (f == B - 1) offsets[B] = off + n;
    }
    if ((size_t)off + n > packed_cap) return;
    const uint8_t* src = out + (size_t)f * out_stride;
    uint8_t* dst = packed + off;
    for (uint32_t i = 4 * threadIdx.x; i < n; i += 1024) {
        if (i + 4 <= n) {
            uint32_t t;
            __builtin_memcpy(&t, src + i, 4);
            __builtin_memcpy(dst + i, &t, 4);
        } else {
            for (uint32_t k = i; k < n; ++k) dst[k] = src[k];
        }
    }
}

static bool enc_sizes_ok(int H, int W) {
    if (H <= 0 || W <= 0 || H > ORBIT_RESIZE_MAX_SIZE || W > ORBIT_RESIZE_MAX_SIZE) return false;
    const EncGeom g = enc_geom(H, W, 0);
    return (uint64_t)g.blocks * ENC_BLOCK_WORDS * 32 < ((uint64_t)1 << 32);  // bit offsets are 32-bit
}

}  // namespace orbit

using namespace orbit;

extern "C" {

int orbit_jpeg_encode_params(int quality, int restart_rows, orbit_jpeg_enc_t* p, size_t p_bytes) {
    ORBIT_REQUIRE(p, "jpeg_encode_params: null pointer");
    ORBIT_REQUIRE(p_bytes == sizeof(orbit_jpeg_enc_t), "jpeg_encode_params: the parameter block is %zu bytes, the caller's p_bytes %zu",
                  sizeof(orbit_jpeg_enc_t), p_bytes);
    ORBIT_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode_params: quality %d outside 1 .. 100", quality);
    ORBIT_REQUIRE(restart_rows >= 0, "jpeg_encode_params: negative restart_rows (%d)", restart_rows);
    enc_params(quality, restart_rows, p);
    return ORBIT_OK;
}

int orbit_jpeg_encode_header(const orbit_jpeg_enc_t* p, int H, int W, const uint8_t* comment, size_t comment_bytes, uint8_t* out,
                             size_t cap) {
    ORBIT_REQUIRE(p && out && (comment || comment_bytes == 0), "jpeg_encode_header: null pointer");
    ORBIT_REQUIRE(H > 0 && W > 0 && H <= 65535 && W <= 65535 && p->restart_rows >= 0, "jpeg_encode_header: bad sizes");
    ORBIT_REQUIRE(comment_bytes <= (size_t)ENC_MAX_COMMENT, "jpeg_encode_header: a comment of %zu bytes, a COM segment holds %d",
                  comment_bytes, ENC_MAX_COMMENT);
    ORBIT_REQUIRE(enc_geom(H, W, p->restart_rows).interval <= 65535, "jpeg_encode_header: a restart interval of %d MCUs exceeds 65535",
                  enc_geom(H, W, p->restart_rows).interval);
    const size_t n = enc_header_bytes(p->restart_rows, comment_bytes);
    ORBIT_REQUIRE(cap >= n, "jpeg_encode_header: out holds %zu bytes, the header has %zu", cap, n);
    size_t k = enc_header_head(out);
    if (comment_bytes) {
        out[k++] = 0xFF, out[k++] = 0xFE, out[k++] = (uint8_t)((comment_bytes + 2) >> 8), out[k++] = (uint8_t)(comment_bytes + 2);
        memcpy(out + k, comment, comment_bytes);
        k += comment_bytes;
    }
    k += enc_header_tail(p, H, W, out + k);
    return (int)k;
}

size_t orbit_jpeg_encode_bound(int H, int W, int restart_rows, size_t comment_bytes) {
    if (!enc_sizes_ok(H, W) || restart_rows < 0 || comment_bytes > (size_t)ENC_MAX_COMMENT) return 0;
    return enc_bound(H, W, restart_rows, comment_bytes);
}

size_t orbit_jpeg_encode_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || !enc_sizes_ok(H, W)) return 0;
    return (size_t)B * enc_layout(H, W).total;
}

int orbit_frames_to_jpeg(const uint8_t* frames_u8_hwc, int B, int H, int W, const orbit_jpeg_enc_t* params, const uint8_t* comments,
                         const uint32_t* comment_offsets, uint8_t* out, size_t out_stride, uint32_t* out_bytes, void* workspace,
                         size_t workspace_bytes, orbit_stream_t stream) {
    ORBIT_REQUIRE(frames_u8_hwc && params && out && out_bytes && workspace, "frames_to_jpeg: null pointer");
    ORBIT_REQUIRE((comments == nullptr) == (comment_offsets == nullptr), "frames_to_jpeg: null pointer (comments and comment_offsets go together)");
    ORBIT_REQUIRE(B > 0 && H > 0 && W > 0, "frames_to_jpeg: bad sizes");
    ORBIT_REQUIRE(enc_sizes_ok(H, W) && H <= 65535 && W <= 65535, "frames_to_jpeg: %dx%d exceeds the encoder's limit (%d pixels per side, 2^32 bits per frame)",
                  H, W, ORBIT_RESIZE_MAX_SIZE);
    ORBIT_REQUIRE(params->quality >= 1 && params->quality <= 100 && params->restart_rows >= 0, "frames_to_jpeg: params were not filled by orbit_jpeg_encode_params");
    const EncGeom g = enc_geom(H, W, params->restart_rows);
    ORBIT_REQUIRE(g.interval <= 65535, "frames_to_jpeg: a restart interval of %d MCUs exceeds 65535", g.interval);
    size_t longest = 0;
    if (comment_offsets)
        for (int b = 0; b < B; ++b) {
            ORBIT_REQUIRE(comment_offsets[b + 1] >= comment_offsets[b], "frames_to_jpeg: comment_offsets decrease at frame %d", b);
            longest = std::max<size_t>(longest, comment_offsets[b + 1] - comment_offsets[b]);
        }
    ORBIT_REQUIRE(longest <= (size_t)ENC_MAX_COMMENT, "frames_to_jpeg: a comment of %zu bytes, a COM segment holds %d", longest, ENC_MAX_COMMENT);
    const size_t bound = enc_bound(H, W, params->restart_rows, longest);
    ORBIT_REQUIRE(out_stride >= bound, "frames_to_jpeg: out_stride of %zu bytes, a %dx%d frame may need %zu", out_stride, H, W, bound);
    ORBIT_REQUIRE(((uintptr_t)workspace & 15) == 0, "frames_to_jpeg: workspace must be 16-byte aligned");
    const EncLayout l = enc_layout(H, W);
    ORBIT_REQUIRE(workspace_bytes >= l.total, "frames_to_jpeg: workspace of %zu bytes, one %dx%d frame needs %zu", workspace_bytes, H, W, l.total);

    EncQuantArg qa;
    EncHuffArg ha;
    EncHeadArg head;
    for (int t = 0; t < 2; ++t) {
        for (int i = 0; i < 64; ++i) qa.q[t][i] = params->qt[t][i], qa.recip[t][i] = params->qrecip[t][i];
        memcpy(ha.dc[t], params->dc[t], sizeof(ha.dc[t]));
        memcpy(ha.ac[t], params->ac[t], sizeof(ha.ac[t]));
    }
    enc_header_head(head.head);
    head.tail_len = (uint32_t)enc_header_tail(params, H, W, head.tail);

    uint8_t* ws = (uint8_t*)workspace;
    const size_t strips = (size_t)2 * g.mcux * 8 * g.mcuy;  // threads per frame of the colour kernel, the widest launch
    const size_t by_threads = std::max<size_t>(1, ((size_t)1 << 30) / strips);
    const int chunk = (int)std::min<size_t>(std::min<size_t>(std::min(workspace_bytes / l.total, by_threads), (size_t)ENC_MAX_FRAMES), (size_t)B);
    const unsigned chunk_blocks = (unsigned)((enc_unstuffed_cap(g.blocks) / ENC_CHUNK + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    int rc = ORBIT_OK;
    for (int b0 = 0; b0 < B && rc == ORBIT_OK; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        for (int b = 0; b <= nb; ++b) head.com_off[b] = comment_offsets ? comment_offsets[b0 + b] : 0u;
        const size_t px = (size_t)nb * H * W, blocks = (size_t)nb * g.blocks;
        const size_t n_color = (size_t)nb * strips;
        int rec = prof_start("jpeg_enc_color", 0.0, (double)px * 3 + (double)nb * g.mcus * 384, s);
        enc_color_kernel<<<(unsigned)((n_color + 255) / 256), 256, 0, s>>>(frames_u8_hwc + (size_t)b0 * H * W * 3, g, n_color, ws, l);
        prof_stop(rec, s);
        rec = prof_start("jpeg_enc_dct", 0.0, (double)nb * g.mcus * 384 + (double)blocks * 128, s);
        enc_dct_kernel<<<(unsigned)((blocks + 255) / 256), 256, 0, s>>>(g, blocks, ws, l, qa);
        prof_stop(rec, s);
        rec = prof_start("jpeg_enc_size", 0.0, (double)blocks * 132, s);
        enc_size_kernel<<<(unsigned)((blocks + 255) / 256), 256, 0, s>>>(g, blocks, ws, l, ha);
        prof_stop(rec, s);
        rec = prof_start("jpeg_enc_scan", 0.0, (double)blocks * 8, s);
        enc_scan_kernel<<<nb, 256, 0, s>>>(g, ws, l);
        prof_stop(rec, s);
        rec = prof_start("jpeg_enc_pack", 0.0, (double)blocks * 132, s);
        enc_pack_kernel<<<(unsigned)((blocks + 255) / 256), 256, 0, s>>>(g, blocks, ws, l, ha);
        prof_stop(rec, s);
        rec = prof_start("jpeg_enc_ff", 0.0, 0.0, s);
        enc_ff_kernel<<<nb, 256, 0, s>>>(g, ws, l);
        prof_stop(rec, s);
        rec = prof_start("jpeg_enc_assemble", 0.0, 0.0, s);
        enc_assemble_kernel<<<dim3(1 + chunk_blocks, nb), 256, 0, s>>>(g, ws, l, head, comments, out + (size_t)b0 * out_stride, out_stride,
                                                                       out_bytes + b0);
        prof_stop(rec, s);
        if (hipGetLastError() != hipSuccess) rc = set_err(ORBIT_ERR_HIP, "frames_to_jpeg: kernel launch failed");
    }
    return rc;
}

int orbit_jpeg_compact(const uint8_t* out, size_t out_stride, const uint32_t* out_bytes, int B, uint8_t* packed, size_t packed_cap,
                       uint32_t* offsets, orbit_stream_t stream) {
    ORBIT_REQUIRE(out && out_bytes && packed && offsets, "jpeg_compact: null pointer");
    ORBIT_REQUIRE(B > 0 && out_stride > 0, "jpeg_compact: bad sizes");
    ORBIT_REQUIRE((uint64_t)B * out_stride < ((uint64_t)1 << 32), "jpeg_compact: %d slices of %zu bytes exceed 32-bit offsets", B, out_stride);
    hipStream_t s = (hipStream_t)stream;
    const int rec = prof_start("jpeg_compact", 0.0, 0.0, s);
    jpeg_compact_kernel<<<B, 256, 0, s>>>(out, out_stride, out_bytes, B, packed, packed_cap, offsets);
    prof_stop(rec, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

}  // extern "C"
