// Baseline JPEG encoding as plain integer code that compiles for the host and for the device: what Pillow's
// Image.save(quality=q) writes for an RGB image - 3-component YCbCr, SOF0, 8 bit, 4:2:0, one interleaved scan, the Annex-K
// Huffman tables - restated from the JPEG standard (ITU T.81) and from the arithmetic of libjpeg's default compression path
// (jcparam.c, jccolor.c, jcsample.c, jccoefct.c, jfdctint.c, jcdctmgr.c, jchuff.c, jcmarker.c). csrc/jpeg_enc.hip wraps the
// per-strip, per-block and per-chunk functions in kernels; tools/jpeg_enc_host_check.cpp runs the very same functions
// serially on the CPU under the sanitizers, where their output is compared with Pillow's bytes.
//
// Padding order (it matters; 18 x 22 tells the variants apart). Luma: the last column is replicated to a multiple of 8, then
// the last row. Chroma, at full resolution: the last row is replicated to an even row count and the last column to the MCU
// grid; then 2 x 2 boxes are averaged with bias 1 on even output columns and 2 on odd ones; only then is the last
// DOWNSAMPLED row replicated to the block grid. Every one of these is a clamp of an index, so nothing is materialised:
// enc_quad reads the pixels a 2 x 2 box of the padded grid stands for.
//
// A block of an MCU that lies wholly right of or below its component's block grid (luma only: the chroma grids equal the MCU
// grid) is a dummy block: all AC coefficients zero, the DC that of the block before it in the MCU (Y00 Y01 Y10 Y11 Cb Cr).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "jpeg_core.h"  // ORBIT_JPEG_NATURAL_ORDER

#if defined(__HIPCC__)
#define ENC_HD __host__ __device__ __forceinline__
#else
#define ENC_HD inline
#endif

namespace orbit_jpegenc {

constexpr int ENC_BLOCK_MAX_BITS = 22 + 63 * 26;  // DC: 11-bit code + 11 value bits; every AC: 16-bit code + 10 value bits
constexpr int ENC_BLOCK_WORDS = 52;               // 32-bit words of the unstuffed bit buffer per block: 1664 >= 1660 bits
constexpr int ENC_CHUNK = 32;                     // bytes of the unstuffed stream one thread stuffs
constexpr int ENC_MAX_COMMENT = 65533;
constexpr int ENC_HEADER_MAX = 20 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14;  // everything but the COM segment

// ---- geometry ------------------------------------------------------------------------------------------------------------------
// Blocks are numbered in scan order: MCU-major, six per MCU. A restart interval (`interval` MCUs, 0 = none) is a segment of
// the scan; nseg of them make a frame.
struct EncGeom {
    int H, W, mcux, mcuy, mcus, blocks, interval, nseg;
};

ENC_HD EncGeom enc_geom(int H, int W, int restart_rows) {
    EncGeom g;
    g.H = H, g.W = W;
    g.mcux = (W + 15) / 16, g.mcuy = (H + 15) / 16;
    g.mcus = g.mcux * g.mcuy;
    g.blocks = 6 * g.mcus;
    g.interval = restart_rows * g.mcux;
    g.nseg = g.interval > 0 ? (g.mcus + g.interval - 1) / g.interval : 1;
    return g;
}
ENC_HD int enc_seg_first_block(const EncGeom& g, int s) { return 6 * s * g.interval; }
ENC_HD int enc_seg_end_block(const EncGeom& g, int s) { return s + 1 < g.nseg ? 6 * (s + 1) * g.interval : g.blocks; }
ENC_HD int enc_block_seg(const EncGeom& g, int blk) { return g.interval > 0 ? blk / (6 * g.interval) : 0; }

// A frame's slice of the workspace, every part at a multiple of 16 bytes:
//   Y plane [16 mcuy][16 mcux], Cb and Cr planes [8 mcuy][8 mcux]; coefficients [blocks][64] int16, zigzag order;
//   sums [blocks] uint32: a block's bit count, then the inclusive sum of them over the frame; seg [nseg + 2] uint32: first
//   byte of every segment in the unstuffed stream, seg[nseg] = its length, seg[nseg + 1] = the FF bytes in it; the unstuffed bit buffer, ENC_BLOCK_WORDS words
//   per block; ff [chunks] uint32: the number of FF bytes in front of every ENC_CHUNK bytes of it.
struct EncLayout {
    size_t y, cb, cr, coef, sums, seg, bits, ff, total;
};
ENC_HD size_t enc_up16(size_t v) { return (v + 15) / 16 * 16; }
ENC_HD size_t enc_unstuffed_cap(int blocks) { return (size_t)blocks * ENC_BLOCK_WORDS * 4; }
ENC_HD EncLayout enc_layout(int H, int W) {
    // sized for the most segments a frame can have (restart_rows = 1), so that the workspace is a function of B, H, W alone
    const EncGeom g = enc_geom(H, W, 1);
    EncLayout l;
    l.y = 0;
    l.cb = l.y + (size_t)g.mcus * 256;
    l.cr = l.cb + (size_t)g.mcus * 64;
    l.coef = l.cr + (size_t)g.mcus * 64;
    l.sums = l.coef + (size_t)g.blocks * 128;
    l.seg = l.sums + enc_up16((size_t)g.blocks * 4);
    l.bits = l.seg + enc_up16((size_t)(g.nseg + 2) * 4);
    l.ff = l.bits + enc_unstuffed_cap(g.blocks);
    l.total = l.ff + enc_up16(enc_unstuffed_cap(g.blocks) / ENC_CHUNK * 4);
    return l;
}

// ---- Annex K tables -------------------------------------------------------------------------------------------------------------
#define ORBIT_JPEG_ENC_QT_LUMA                                                                                                 \
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,                   \
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,                   \
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99}
#define ORBIT_JPEG_ENC_QT_CHROMA                                                                                               \
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, \
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}

// code counts per length 1 .. 16, then the symbols in code order; table 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma
struct EncHuffSpec {
    uint8_t counts[16];
    int nvals;
    const uint8_t* vals;
};
inline EncHuffSpec enc_huff_spec(int t) {
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t ac_luma[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
        0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
        0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
        0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
        0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
        0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
        0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
        0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    static const uint8_t ac_chroma[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
        0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
        0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
        0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
        0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
        0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
        0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
        0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    static const EncHuffSpec specs[4] = {
        {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, dc_vals},
        {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, ac_luma},
        {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, dc_vals},
        {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, ac_chroma}};
    return specs[t & 3];
}

// ---- parameters (host) ---------------------------------------------------------------------------------------------------------
// jpeg_set_quality with force_baseline; a table entry of the code tables is code << 5 | length, 0 where the symbol has no code
inline void enc_params(int quality, int restart_rows, orbit_jpeg_enc_t* p) {
    static const uint8_t base[2][64] = {ORBIT_JPEG_ENC_QT_LUMA, ORBIT_JPEG_ENC_QT_CHROMA};
    p->quality = quality, p->restart_rows = restart_rows;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            int v = (base[t][i] * scale + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            p->qt[t][i] = (uint16_t)v;
            // ceil(2^32 / d), d = 8 v <= 2040: floor(n / d) == (n * m) >> 32 for every n < 2^21, because m d - 2^32 < d < 2^11
            // and so n (m d - 2^32) < 2^32; the numerators are below 2^15 (enc_quantise)
            const uint64_t d = 8u * (uint32_t)v;
            p->qrecip[t][i] = (uint32_t)((((uint64_t)1 << 32) + d - 1) / d);
        }
    for (int t = 0; t < 4; ++t) {
        const EncHuffSpec s = enc_huff_spec(t);
        uint32_t* dst = (t & 1) ? p->ac[t >> 1] : p->dc[t >> 1];
        const int n = (t & 1) ? 256 : 16;
        for (int i = 0; i < n; ++i) dst[i] = 0;
        uint32_t code = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < s.counts[l - 1]; ++i, ++k, ++code) dst[s.vals[k] & (n - 1)] = (code << 5) | (uint32_t)l;
            code <<= 1;
        }
    }
}

// ---- header (host) -------------------------------------------------------------------------------------------------------------
// SOI, APP0 - the part in front of the COM segment - is 20 bytes; enc_header_tail writes what follows it, DQT .. SOS.
inline size_t enc_header_head(uint8_t* o) {
    static const uint8_t head[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 20; ++i) o[i] = head[i];
    return 20;
}
inline size_t enc_header_tail(const orbit_jpeg_enc_t* p, int H, int W, uint8_t* o) {
    static const uint8_t natural[64] = ORBIT_JPEG_NATURAL_ORDER;
    size_t n = 0;
    for (int t = 0; t < 2; ++t) {
        o[n++] = 0xFF, o[n++] = 0xDB, o[n++] = 0, o[n++] = 67, o[n++] = (uint8_t)t;
        for (int k = 0; k < 64; ++k) o[n++] = (uint8_t)p->qt[t][natural[k]];
    }
    const uint8_t sof[19] = {0xFF, 0xC0, 0, 17, 8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, 3,
                             1,    0x22, 0, 2,  0x11, 1, 3, 0x11, 1};
    for (int i = 0; i < 19; ++i) o[n++] = sof[i];
    static const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        const EncHuffSpec s = enc_huff_spec(t);
        const int len = 2 + 1 + 16 + s.nvals;
        o[n++] = 0xFF, o[n++] = 0xC4, o[n++] = (uint8_t)(len >> 8), o[n++] = (uint8_t)len, o[n++] = ids[t];
        for (int i = 0; i < 16; ++i) o[n++] = s.counts[i];
        for (int i = 0; i < s.nvals; ++i) o[n++] = s.vals[i];
    }
    const EncGeom g = enc_geom(H, W, p->restart_rows);
    if (g.interval > 0) {
        o[n++] = 0xFF, o[n++] = 0xDD, o[n++] = 0, o[n++] = 4, o[n++] = (uint8_t)(g.interval >> 8), o[n++] = (uint8_t)g.interval;
    }
    static const uint8_t sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0};
    for (int i = 0; i < 14; ++i) o[n++] = sos[i];
    return n;
}
ENC_HD size_t enc_header_bytes(int restart_rows, size_t comment_bytes) {
    return (size_t)ENC_HEADER_MAX - (restart_rows > 0 ? 0 : 6) + (comment_bytes ? 4 + comment_bytes : 0);
}

// A slice size no frame can overflow: a block codes to at most ENC_BLOCK_MAX_BITS = 1660 bits, the bit buffer gives it
// ENC_BLOCK_WORDS * 32 = 1664, which also covers the up to 7 fill bits at the end of every interval (an interval has at least 6
// blocks); stuffing at most doubles those bytes; an interval adds its 2-byte marker (3 are counted); header and EOI.
ENC_HD size_t enc_bound(int H, int W, int restart_rows, size_t comment_bytes) {
    const EncGeom g = enc_geom(H, W, restart_rows);
    return enc_header_bytes(restart_rows, comment_bytes) + 2 * enc_unstuffed_cap(g.blocks) + 3 * (size_t)g.nseg + 2;
}

// ---- colour conversion + chroma downsampling (jccolor.c rgb_ycc_convert, jcsample.c h2v2_downsample) ------------------------------
ENC_HD void enc_ycc(int r, int g, int b, int& y, int& cb, int& cr) {
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
ENC_HD int enc_imin(int a, int b) { return a < b ? a : b; }

// The 2 x 2 box (qx, qy) of the padded grid of frame rgb [H][W][3]: its four luma samples (row-major) and its chroma pair.
// Reads only pixels of the frame.
ENC_HD void enc_quad(const uint8_t* rgb, int H, int W, int qx, int qy, uint8_t yv[4], uint8_t& cbv, uint8_t& crv) {
    const int x[2] = {enc_imin(2 * qx, W - 1), enc_imin(2 * qx + 1, W - 1)};
    const int cq = enc_imin(qy, (H + 1) / 2 - 1);  // the downsampled row this one replicates
    const int bias = (qx & 1) ? 2 : 1;
    int scb = bias, scr = bias;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ly = enc_imin(2 * qy + j, H - 1), cy = enc_imin(2 * cq + j, H - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint8_t* p = rgb + ((size_t)ly * W + x[i]) * 3;
            int y, cb, cr;
            enc_ycc(p[0], p[1], p[2], y, cb, cr);
            yv[2 * j + i] = (uint8_t)y;
            if (cy != ly) {
                const uint8_t* c = rgb + ((size_t)cy * W + x[i]) * 3;
                enc_ycc(c[0], c[1], c[2], y, cb, cr);
            }
            scb += cb, scr += cr;
        }
    }
    cbv = (uint8_t)(scb >> 2), crv = (uint8_t)(scr >> 2);
}

// The same for four boxes side by side that lie wholly inside the frame, from two rows of 8 pixels held as six little-endian
// words each: ylo / yhi = the 8 luma samples of the upper / lower row, cb4 / cr4 = the four chroma samples, packed likewise.
// q0 = index of the first box (its parity sets the bias).
ENC_HD uint32_t enc_byte(const uint32_t* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }
ENC_HD void enc_strip(const uint32_t r0[6], const uint32_t r1[6], int q0, uint32_t ylo[2], uint32_t yhi[2], uint32_t& cb4,
                      uint32_t& cr4) {
    ylo[0] = ylo[1] = yhi[0] = yhi[1] = 0, cb4 = cr4 = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int bias = ((q0 + q) & 1) ? 2 : 1;
        int scb = bias, scr = bias;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int px = 2 * q + i;
            int y, cb, cr;
            enc_ycc((int)enc_byte(r0, 3 * px), (int)enc_byte(r0, 3 * px + 1), (int)enc_byte(r0, 3 * px + 2), y, cb, cr);
            ylo[px >> 2] |= (uint32_t)y << (8 * (px & 3));
            scb += cb, scr += cr;
            enc_ycc((int)enc_byte(r1, 3 * px), (int)enc_byte(r1, 3 * px + 1), (int)enc_byte(r1, 3 * px + 2), y, cb, cr);
            yhi[px >> 2] |= (uint32_t)y << (8 * (px & 3));
            scb += cb, scr += cr;
        }
        cb4 |= (uint32_t)(scb >> 2) << (8 * q), cr4 |= (uint32_t)(scr >> 2) << (8 * q);
    }
}

// Strip (sx, qy) of the padded grid - boxes 4 sx .. 4 sx + 3 of box row qy - wherever it lies: 4-byte loads of its 2 x 24 bytes
// where all of it is inside the frame, enc_quad box by box at the right and bottom edges.
ENC_HD void enc_strip_at(const uint8_t* rgb, int H, int W, int sx, int qy, uint32_t ylo[2], uint32_t yhi[2], uint32_t& cb4,
                         uint32_t& cr4) {
    if (8 * sx + 8 <= W && 2 * qy + 2 <= H) {
        uint32_t r0[6], r1[6];
        const uint8_t* p = rgb + ((size_t)(2 * qy) * W + 8 * sx) * 3;
        __builtin_memcpy(r0, p, 24);
        __builtin_memcpy(r1, p + (size_t)W * 3, 24);
        enc_strip(r0, r1, 4 * sx, ylo, yhi, cb4, cr4);
        return;
    }
    ylo[0] = ylo[1] = yhi[0] = yhi[1] = 0, cb4 = cr4 = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint8_t yv[4], cb, cr;
        enc_quad(rgb, H, W, 4 * sx + q, qy, yv, cb, cr);
        ylo[q >> 1] |= ((uint32_t)yv[0] | (uint32_t)yv[1] << 8) << (16 * (q & 1));
        yhi[q >> 1] |= ((uint32_t)yv[2] | (uint32_t)yv[3] << 8) << (16 * (q & 1));
        cb4 |= (uint32_t)cb << (8 * q), cr4 |= (uint32_t)cr << (8 * q);
    }
}

// ---- forward DCT + quantisation (jfdctint.c jpeg_fdct_islow, jcdctmgr.c forward_DCT) -----------------------------------------------
// 13 fractional bits, 2 extra bits after the first pass; the output is 8 times the DCT, which the quantiser divides out.
ENC_HD int32_t enc_descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }

// first = true: the row pass (results up-scaled by 4); false: the column pass
ENC_HD void enc_fdct_1d(const int32_t d[8], bool first, int32_t o[8]) {
    int32_t tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int32_t tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int sh = first ? 11 : 15;
    o[0] = first ? (tmp10 + tmp11) * 4 : enc_descale(tmp10 + tmp11, 2);
    o[4] = first ? (tmp10 - tmp11) * 4 : enc_descale(tmp10 - tmp11, 2);
    int32_t z1 = (tmp12 + tmp13) * 4433;
    o[2] = enc_descale(z1 + tmp13 * 6270, sh);
    o[6] = enc_descale(z1 + tmp12 * -15137, sh);
    z1 = tmp4 + tmp7;
    int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int32_t z5 = (z3 + z4) * 9633;
    tmp4 *= 2446, tmp5 *= 16819, tmp6 *= 25172, tmp7 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
    z3 += z5, z4 += z5;
    o[7] = enc_descale(tmp4 + z1 + z3, sh);
    o[5] = enc_descale(tmp5 + z2 + z4, sh);
    o[3] = enc_descale(tmp6 + z2 + z3, sh);
    o[1] = enc_descale(tmp7 + z1 + z4, sh);
}

// |x| < 2^15: the DC of 64 samples of magnitude 128 is 8192, no AC output of the transform exceeds 1.5 times that, and half a
// divisor (<= 1020) is added
ENC_HD int enc_quantise(int32_t x, uint32_t q, uint32_t recip) {
    const uint32_t a = (uint32_t)(x < 0 ? -x : x) + ((8u * q) >> 1);
    const int v = (int)(((uint64_t)a * recip) >> 32);
    return x < 0 ? -v : v;
}

// One block: 8 x 8 samples at `in` (rows `pitch` apart) -> 64 quantised coefficients in zigzag order. q / recip: the
// component's table in natural order. Fully unrolled, every index a constant: the block lives in registers.
ENC_HD void enc_fdct_block(const uint8_t* in, size_t pitch, const uint32_t* q, const uint32_t* recip, int16_t* zz) {
    constexpr uint8_t natural[64] = ORBIT_JPEG_NATURAL_ORDER;
    int32_t ws[64];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        uint32_t w[2];
        __builtin_memcpy(w, in + y * pitch, 8);  // (rows of a plane start at multiples of 8)
        int32_t d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int32_t)enc_byte(w, k) - 128;
        enc_fdct_1d(d, true, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[8 * y + k] = o[k];
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        int32_t d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = ws[8 * k + x];
        enc_fdct_1d(d, false, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[8 * k + x] = o[k];
    }
#pragma unroll
    for (int k = 0; k < 64; ++k) zz[k] = (int16_t)enc_quantise(ws[natural[k]], q[natural[k]], recip[natural[k]]);
}

// Block `blk` of the scan: which component, where its samples lie, whether it is a dummy block.
struct EncBlockPos {
    int comp;      // 0 Y, 1 Cb, 2 Cr
    int bx, by;    // block coordinates in the component's padded plane
    bool dummy;
};
ENC_HD EncBlockPos enc_block_pos(const EncGeom& g, int blk) {
    const int m = blk / 6, k = blk - 6 * m;
    const int my = m / g.mcux, mx = m - my * g.mcux;
    EncBlockPos p;
    if (k < 4) {
        p.comp = 0, p.bx = 2 * mx + (k & 1), p.by = 2 * my + (k >> 1);
        p.dummy = p.bx >= (g.W + 7) / 8 || p.by >= (g.H + 7) / 8;
    } else {
        p.comp = k - 3, p.bx = mx, p.by = my, p.dummy = false;
    }
    return p;
}

// The block whose DC predicts block blk's: the previous block of the same component in scan order, -1 at the first MCU of
// the frame and of every restart interval.
ENC_HD int enc_dc_pred_block(const EncGeom& g, int blk) {
    const int m = blk / 6, k = blk - 6 * m;
    if (k >= 1 && k <= 3) return blk - 1;
    if (m == 0 || (g.interval > 0 && m % g.interval == 0)) return -1;
    return k == 0 ? blk - 3 : blk - 6;
}

// ---- entropy coding (jchuff.c encode_one_block) -------------------------------------------------------------------------------------
ENC_HD int enc_nbits(int v) {  // bit length of |v|
    uint32_t a = (uint32_t)(v < 0 ? -v : v);
    int n = 0;
    while (a) ++n, a >>= 1;
    return n;
}

// The codes of one block go to sink.put(bits, length), length <= 16, most significant first. zz: zigzag coefficients; diff:
// the DC difference; dct / act: the component's code tables (code << 5 | length). A counting sink gives the block's size,
// a writing sink its bits: one walk serves both, so the two cannot disagree.
template <class Sink>
ENC_HD void enc_block_codes(const int16_t* zz, int diff, const uint32_t* dct, const uint32_t* act, Sink& sink) {
    int n = enc_nbits(diff);
    uint32_t e = dct[n & 15];
    sink.put(e >> 5, (int)(e & 31));
    if (n) sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
    int r = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) {
            ++r;
            continue;
        }
        while (r > 15) {
            e = act[0xF0];
            sink.put(e >> 5, (int)(e & 31));
            r -= 16;
        }
        n = enc_nbits(v);
        e = act[((r << 4) | n) & 255];
        sink.put(e >> 5, (int)(e & 31));
        sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
        r = 0;
    }
    if (r > 0) {
        e = act[0];
        sink.put(e >> 5, (int)(e & 31));
    }
}

struct EncCountSink {
    uint32_t bits;
    ENC_HD void put(uint32_t, int len) { bits += (uint32_t)len; }
};

ENC_HD uint32_t enc_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// Writes a block's bits at bit offset `start` of the unstuffed buffer (words in memory order, so every word is byte-swapped
// on its way out). The first and the last word of a block are shared with its neighbours: they are OR-ed into the zeroed
// buffer (Mem::or_word), the words between belong to the block alone and are stored (Mem::set_word).
template <class Mem>
struct EncBitSink {
    Mem mem;
    uint64_t acc;
    int n;
    uint32_t word;
    bool first;
    ENC_HD void begin(uint32_t start) { acc = 0, n = (int)(start & 31u), word = start >> 5, first = true; }
    ENC_HD void put(uint32_t bits, int len) {
        if (len == 0) return;
        acc |= (uint64_t)bits << (64 - n - len);  // n < 32, len <= 16
        n += len;
        if (n >= 32) {
            const uint32_t w = enc_bswap((uint32_t)(acc >> 32));
            if (first) mem.or_word(word, w);
            else mem.set_word(word, w);
            first = false, ++word, acc <<= 32, n -= 32;
        }
    }
    ENC_HD void end() {
        if (n > 0) mem.or_word(word, enc_bswap((uint32_t)(acc >> 32)));
    }
};

// Block blk of a frame, complete: DC prediction, codes, and behind the last block of a restart interval (or of the frame)
// the 1 bits that fill its last byte. sums: inclusive bit sums of the frame's blocks; seg: first byte of every segment.
template <class Mem>
ENC_HD void enc_pack_block(const EncGeom& g, int blk, const int16_t* coef, const uint32_t* sums, const uint32_t* seg,
                           const uint32_t* dc_tab, const uint32_t* ac_tab, Mem mem) {
    const int s = enc_block_seg(g, blk), first = enc_seg_first_block(g, s);
    const uint32_t before = blk > 0 ? sums[blk - 1] : 0, seg_before = first > 0 ? sums[first - 1] : 0;
    const uint32_t start = 8u * seg[s] + (before - seg_before);
    const int pred = enc_dc_pred_block(g, blk), t = blk % 6 >= 4 ? 1 : 0;
    const int16_t* zz = coef + (size_t)blk * 64;
    const int diff = (int)zz[0] - (pred >= 0 ? (int)coef[(size_t)pred * 64] : 0);
    EncBitSink<Mem> sink{mem, 0, 0, 0, true};
    sink.begin(start);
    enc_block_codes(zz, diff, dc_tab + 16 * t, ac_tab + 256 * t, sink);
    if (blk + 1 == enc_seg_end_block(g, s)) {
        const int pad = (int)((0u - (start + (sums[blk] - before))) & 7u);
        sink.put((1u << pad) - 1u, pad);
    }
    sink.end();
}

ENC_HD uint32_t enc_block_bits(const EncGeom& g, int blk, const int16_t* coef, const uint32_t* dc_tab, const uint32_t* ac_tab) {
    const int pred = enc_dc_pred_block(g, blk), t = blk % 6 >= 4 ? 1 : 0;
    const int16_t* zz = coef + (size_t)blk * 64;
    const int diff = (int)zz[0] - (pred >= 0 ? (int)coef[(size_t)pred * 64] : 0);
    EncCountSink sink{0};
    enc_block_codes(zz, diff, dc_tab + 16 * t, ac_tab + 256 * t, sink);
    return sink.bits;
}

// From the inclusive sums: seg[s] = first byte of segment s in the unstuffed stream, every segment rounded up to whole bytes;
// seg[nseg] = the stream's length. (Serial; the kernel scans the same quantities in parallel.)
ENC_HD uint32_t enc_seg_bytes(const EncGeom& g, const uint32_t* sums, int s) {
    const int a = enc_seg_first_block(g, s), b = enc_seg_end_block(g, s);
    return (sums[b - 1] - (a > 0 ? sums[a - 1] : 0) + 7u) >> 3;
}

// ---- byte stuffing + restart markers -------------------------------------------------------------------------------------------------
ENC_HD uint32_t enc_count_ff(const uint8_t* src, uint32_t c0, uint32_t c1) {
    uint32_t n = 0;
    for (uint32_t i = c0; i < c1; ++i) n += src[i] == 0xFF;
    return n;
}

// Bytes [c0, c1) of the unstuffed stream -> the scan at dst: byte i of segment s lands at i + (FF bytes in front of it) + 2 s;
// the marker in front of segment s >= 1 is written by whoever writes the segment's first byte. ff_before: FF bytes in [0, c0).
ENC_HD void enc_stuff_chunk(const uint8_t* src, uint32_t c0, uint32_t c1, uint32_t ff_before, const uint32_t* seg, int nseg,
                            uint8_t* dst) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= c0) lo = mid;
        else hi = mid - 1;
    }
    int s = lo;
    size_t o = (size_t)c0 + ff_before + 2 * (size_t)s;
    uint32_t next = seg[s] == c0 ? c0 : (s + 1 < nseg ? seg[s + 1] : 0xFFFFFFFFu);
    if (seg[s] == c0) --s, o -= 2;  // the loop below re-enters the segment and writes its marker
    for (uint32_t i = c0; i < c1; ++i) {
        if (i == next) {
            ++s, o += 2;
            if (s > 0) dst[o - 2] = 0xFF, dst[o - 1] = (uint8_t)(0xD0 + ((s - 1) & 7));
            next = s + 1 < nseg ? seg[s + 1] : 0xFFFFFFFFu;
        }
        const uint8_t b = src[i];
        dst[o++] = b;
        if (b == 0xFF) dst[o++] = 0;
    }
}

}  // namespace orbit_jpegenc
