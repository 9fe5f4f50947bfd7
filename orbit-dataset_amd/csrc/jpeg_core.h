// Baseline JPEG decoding as plain integer code that compiles for the host and for the device: the header parser (host only),
// the entropy walker (bit reader, Huffman symbol decode, block decode), libjpeg's "islow" inverse DCT, and its chroma
// upsampling + YCbCr -> RGB conversion per pixel. csrc/jpeg.hip wraps the last three in kernels; tools/jpeg_host_check.cpp
// (tools/jpeg_par_host_check.cpp for the walk of one restart interval per lane, tools/jpeg_sub_host_check.cpp for the walk of
// one subsequence of a marker-free stream per lane) runs the very same functions on the CPU
// under the sanitizers, which is where their behaviour on damaged files is established. Restated from the JPEG standard
// (ITU T.81) and from the arithmetic of libjpeg's default decode path (jdhuff.c, jidctint.c, jdsample.c, jdcolor.c): the
// output equals Pillow's for every file the parser accepts and the walker finishes with status 0.
//
// Bounds: the walker reads the stream only through Src::at(pos) with pos < len, writes coefficients only at block indices
// below JpegGeom::total_blocks, and indexes every table with a masked or checked index, so no content of a file can make
// it touch memory outside its own slices.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "orbit_hip.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

namespace orbit_jpeg {

// zigzag position -> natural (row-major) position
#define ORBIT_JPEG_NATURAL_ORDER                                                                                              \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// ---- geometry ----------------------------------------------------------------------------------------------------------------
// Coefficients and samples are kept per component as a plane of whole blocks, wb x hb of them, in raster order; the planes
// follow each other, component c's first block being number base[c].
struct JpegGeom {
    int mcux, mcuy, total_blocks;
    int wb[3], hb[3], base[3];
};

// the largest block count of an H x W frame over the samplings in scope (every one fits 3 planes of 2 * ceil(./16) blocks a side)
JPEG_HD size_t jpeg_cap_blocks(int H, int W) { return 3 * (size_t)(2 * ((W + 15) / 16)) * (size_t)(2 * ((H + 15) / 16)); }

// false when the descriptor is not one the parser would have written for a file in scope
JPEG_HD bool jpeg_geom(const orbit_jpeg_desc_t& d, JpegGeom& g) {
    if (d.width < 1 || d.height < 1 || d.width > ORBIT_RESIZE_MAX_SIZE || d.height > ORBIT_RESIZE_MAX_SIZE) return false;
    if (d.ncomp != 1 && d.ncomp != 3) return false;
    if (d.restart_interval < 0) return false;
    int hmax = 1, vmax = 1;
    if (d.ncomp == 3) {
        hmax = d.hs[0], vmax = d.vs[0];
        if (!((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2))) return false;
        if (d.hs[1] != 1 || d.vs[1] != 1 || d.hs[2] != 1 || d.vs[2] != 1) return false;
    } else if (d.hs[0] != 1 || d.vs[0] != 1) {
        return false;
    }
    g.mcux = (d.width + 8 * hmax - 1) / (8 * hmax);
    g.mcuy = (d.height + 8 * vmax - 1) / (8 * vmax);
    int total = 0;
    for (int c = 0; c < 3; ++c) {
        const bool on = c < d.ncomp;
        if (on && ((unsigned)d.dc_slot[c] > 1u || (unsigned)d.ac_slot[c] > 1u)) return false;
        g.wb[c] = on ? g.mcux * (c == 0 ? hmax : 1) : 0;
        g.hb[c] = on ? g.mcuy * (c == 0 ? vmax : 1) : 0;
        g.base[c] = total;
        total += g.wb[c] * g.hb[c];
    }
    g.total_blocks = total;
    return true;
}

// ---- bit reader --------------------------------------------------------------------------------------------------------------
// acc holds n valid bits, right-aligned. FF 00 is the data byte FF; FF FF .. is fill; any other FF xx is a marker: the reader
// stops in front of it (marker = xx, pos behind it) and hands out no more bits. The end of the segment counts as marker -1.
struct JpegBits {
    uint64_t acc;
    int n;
    uint32_t pos, len;
    int marker;
};

template <class Src>
JPEG_HD void jpeg_fill(JpegBits& b, const Src& s) {
    while (b.n <= 56 && b.marker == 0) {
        if (b.pos >= b.len) {
            b.marker = -1;
            break;
        }
        int c = s.at(b.pos++);
        if (c == 0xFF) {
            int c2 = -1;
            while (b.pos < b.len) {
                c2 = s.at(b.pos++);
                if (c2 != 0xFF) break;
                c2 = -1;
            }
            if (c2 != 0) {
                b.marker = c2;
                break;
            }
        }
        b.acc = (b.acc << 8) | (uint64_t)c;
        b.n += 8;
    }
}

struct JpegWalk {
    JpegBits bits;
    int mcu;            // next MCU
    int to_restart;     // MCUs until the next restart marker (restart_interval > 0)
    int next_rst;       // number of that marker, 0 .. 7
    int dc[3];
    int status;
    int done;
};

JPEG_HD void jpeg_walk_init(JpegWalk& w, const orbit_jpeg_desc_t& d) {
    w.bits.acc = 0, w.bits.n = 0, w.bits.pos = 0, w.bits.len = d.ecs_bytes, w.bits.marker = 0;
    w.mcu = 0, w.to_restart = d.restart_interval, w.next_rst = 0;
    w.dc[0] = w.dc[1] = w.dc[2] = 0;
    w.status = 0, w.done = 0;
}

// k bits, 1 <= k <= 16; past the end: zero, with the status set
template <class Src>
JPEG_HD int jpeg_get_bits(JpegWalk& w, const Src& s, int k) {
    JpegBits& b = w.bits;
    if (b.n < k) jpeg_fill(b, s);
    if (b.n < k) {
        w.status |= ORBIT_JPEG_ST_OVERRUN;
        return 0;
    }
    b.n -= k;
    return (int)((b.acc >> b.n) & ((1u << k) - 1u));
}

// one Huffman symbol, or -1 with the status set
template <class Src>
JPEG_HD int jpeg_symbol(JpegWalk& w, const Src& s, const orbit_jpeg_huff_t& t) {
    JpegBits& b = w.bits;
    if (b.n < 16) jpeg_fill(b, s);
    int l = 1;
    if (b.n >= 8) {
        const int e = t.look[(b.acc >> (b.n - 8)) & 255u];
        if (e != 0) {
            b.n -= e >> 8;
            return e & 255;
        }
        l = 9;
    }
    for (; l <= 16; ++l) {
        if (b.n < l) {
            w.status |= ORBIT_JPEG_ST_OVERRUN;
            return -1;
        }
        const int code = (int)((b.acc >> (b.n - l)) & ((1u << l) - 1u));
        if (code <= t.maxcode[l]) {
            b.n -= l;
            return t.huffval[(t.valptr[l] + code) & 255];
        }
    }
    w.status |= ORBIT_JPEG_ST_CODE;
    return -1;
}

JPEG_HD int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One block: the non-zero quantised coefficients go to coef[natural position]; the block was zeroed by the caller. A
// dequantised value must fit 16 bits, the range in which libjpeg's scalar and vector inverse DCTs compute the same.
template <class Src>
JPEG_HD void jpeg_block(JpegWalk& w, const Src& s, const orbit_jpeg_desc_t& d, const uint8_t* natural, int c, int16_t* coef) {
    const orbit_jpeg_huff_t& dct = d.huff[d.dc_slot[c] & 1];
    const orbit_jpeg_huff_t& act = d.huff[2 + (d.ac_slot[c] & 1)];
    const uint16_t* q = d.qt[c];
    int sym = jpeg_symbol(w, s, dct);
    if (sym < 0) return;
    sym &= 15;
    if (sym) {
        const int v = jpeg_get_bits(w, s, sym);
        if (w.status) return;
        w.dc[c] += jpeg_extend(v, sym);
    }
    const int dcv = w.dc[c];
    if (dcv < -32768 || dcv > 32767 || dcv * (int)q[0] < -32768 || dcv * (int)q[0] > 32767) {
        w.status |= ORBIT_JPEG_ST_RANGE;
        return;
    }
    coef[0] = (int16_t)dcv;
    for (int k = 1; k < 64;) {
        const int rs = jpeg_symbol(w, s, act);
        if (rs < 0) return;
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) break;
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) {
            w.status |= ORBIT_JPEG_ST_INDEX;
            return;
        }
        const int raw = jpeg_get_bits(w, s, sz);
        if (w.status) return;
        const int v = jpeg_extend(raw, sz);
        const int pos = natural[k] & 63;
        const int dq = v * (int)q[pos];
        if (dq < -32768 || dq > 32767) {
            w.status |= ORBIT_JPEG_ST_RANGE;
            return;
        }
        coef[pos] = (int16_t)v;
        ++k;
    }
}

// The marker between two restart intervals, or EOI behind the last MCU (expect = 0xD0 + n or 0xD9): the pad bits of the last
// byte are dropped; whole bytes left in the reader, bytes in front of the marker or another marker set the status.
template <class Src>
JPEG_HD void jpeg_expect_marker(JpegWalk& w, const Src& s, int expect, int flag) {
    JpegBits& b = w.bits;
    if (b.n >= 8) {
        w.status |= flag;
        return;
    }
    b.n = 0, b.acc = 0;
    if (b.marker == 0) jpeg_fill(b, s);  // reads the marker, or a data byte that should not be there
    if (b.n != 0 || b.marker != expect) {
        w.status |= flag;
        return;
    }
    b.marker = 0;
}

// Decodes MCUs until the reader has passed stop_pos, the image is complete (done = 1) or the status is set (done = 1).
// coef: the frame's coefficient planes, zeroed.
template <class Src>
JPEG_HD void jpeg_walk(JpegWalk& w, const Src& s, const orbit_jpeg_desc_t& d, const JpegGeom& g, const uint8_t* natural,
                       int16_t* coef, uint32_t stop_pos) {
    const int mcus = g.mcux * g.mcuy;
    const int hs0 = d.ncomp == 3 ? d.hs[0] : 1, vs0 = d.ncomp == 3 ? d.vs[0] : 1;
    while (!w.done && w.bits.pos <= stop_pos) {
        if (w.mcu >= mcus) {
            jpeg_expect_marker(w, s, 0xD9, ORBIT_JPEG_ST_TRAILING);
            w.done = 1;
            break;
        }
        if (d.restart_interval > 0 && w.to_restart == 0) {
            jpeg_expect_marker(w, s, 0xD0 + w.next_rst, ORBIT_JPEG_ST_RESTART);
            if (w.status) {
                w.done = 1;
                break;
            }
            w.next_rst = (w.next_rst + 1) & 7;
            w.to_restart = d.restart_interval;
            w.dc[0] = w.dc[1] = w.dc[2] = 0;
        }
        const int mx = w.mcu % g.mcux, my = w.mcu / g.mcux;
#pragma unroll
        for (int c = 0; c < 3; ++c) {  // (unrolled: the per-component arrays stay in registers)
            if (c >= d.ncomp) continue;
            const int h = c == 0 ? hs0 : 1, v = c == 0 ? vs0 : 1;
            for (int by = 0; by < v && !w.status; ++by)
                for (int bx = 0; bx < h && !w.status; ++bx) {
                    const int blk = g.base[c] + (my * v + by) * g.wb[c] + mx * h + bx;  // < total_blocks by jpeg_geom
                    jpeg_block(w, s, d, natural, c, coef + (size_t)blk * 64);
                }
        }
        if (w.status) {
            w.done = 1;
            break;
        }
        ++w.mcu;
        if (d.restart_interval > 0) --w.to_restart;
    }
}

// ---- one restart interval per walker (the interval-parallel form) ---------------------------------------------------------------
// Every restart interval starts byte-aligned with the DC predictors reset, so a frame whose markers are all where its
// geometry puts them can be walked interval by interval, in any order or side by side. Three pieces: the marker scan over a
// lane's slice of the segment, the rule that turns the markers of a frame into the table of interval ends, and the walk of
// one interval. A frame takes this form only when the rule holds; when any interval then reports a status, the caller zeroes
// the frame's coefficients and runs jpeg_walk over it, so status and coefficients of a damaged file are jpeg_walk's.
#define JPEG_PAR_MAX_INTERVALS 1024  // the table is 4 KB of LDS

// byte j (0 .. 15) of four little-endian words (by value: an array indexed by j would live in private memory on the device)
JPEG_HD int jpeg_slice_byte(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int j) {
    const uint32_t w = j < 8 ? (j < 4 ? v0 : v1) : (j < 12 ? v2 : v3);
    return (int)((w >> (8 * (j & 3))) & 255u);
}

// The markers of the slice [o, o + n) of the segment, n <= 16, whose bytes are the words v0 .. v3: bit j is set when byte
// o + j is the FF of a marker, FF xx with xx neither 00 (a stuffed data byte) nor FF (fill: the marker's FF is the last one).
// next is the byte at o + n, which decides about an FF at the end of the slice, or -1 behind the segment: an FF that ends the
// segment is no marker.
JPEG_HD uint32_t jpeg_scan_slice(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int n, int next) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = jpeg_slice_byte(v0, v1, v2, v3, j);
        const int c2 = j + 1 < n ? jpeg_slice_byte(v0, v1, v2, v3, (j + 1) & 15) : next;
        if (j < n && c == 0xFF && c2 > 0 && c2 != 0xFF) m |= 1u << j;
    }
    return m;
}

// intervals of the frame by its geometry, or 0 when the frame is walked serially: no restart interval, a single interval, or
// more than the table holds
JPEG_HD int jpeg_par_intervals(const orbit_jpeg_desc_t& d, const JpegGeom& g) {
    const int R = d.restart_interval, mcus = g.mcux * g.mcuy;
    if (R <= 0) return 0;
    const int nseg = mcus / R + (mcus % R != 0);
    return nseg >= 2 && nseg <= JPEG_PAR_MAX_INTERVALS ? nseg : 0;
}

// whether the k-th marker of the segment (k = 0, 1, .. in stream order) may have this code: RST(k mod 8) between the
// intervals, then EOI; what follows EOI is nobody's business
JPEG_HD bool jpeg_par_marker_ok(int k, int code, int nseg) {
    return k < nseg - 1 ? code == 0xD0 + (k & 7) : (k == nseg - 1 ? code == 0xD9 : true);
}

// The byte stream as the walker of one interval sees it: 16 bytes of the segment in two registers, reloaded in words when the
// reader leaves them (it moves forward, so that is one load per 16 bytes). No load touches a byte at or behind `end`; the
// last, partial window of an interval is put together from single bytes.
struct JpegWinSrc {
    const uint8_t* mem;  // the segment's first byte
    uint32_t end;
    mutable uint32_t base;
    mutable uint64_t lo, hi;
    JPEG_HD void load(uint32_t pos) const {
        base = pos, lo = 0, hi = 0;
        if ((uint64_t)pos + 16 <= end) {
            uint64_t a, b;  // (unaligned-safe: the compiler picks the loads)
            __builtin_memcpy(&a, mem + pos, 8);
            __builtin_memcpy(&b, mem + pos + 8, 8);
            lo = a, hi = b;
        } else {
            for (int j = 0; j < 8; ++j) {
                if ((uint64_t)pos + j < end) lo |= (uint64_t)mem[pos + j] << (8 * j);
                if ((uint64_t)pos + 8 + j < end) hi |= (uint64_t)mem[pos + 8 + j] << (8 * j);
            }
        }
    }
    JPEG_HD uint8_t at(uint32_t pos) const {
        uint32_t i = pos - base;
        if (i >= 16u) load(pos), i = 0;
        return (uint8_t)(((i & 8u) ? hi : lo) >> (8 * (i & 7u)));
    }
};

// Interval k of nseg: the MCUs k * R .. of the frame, read from the bytes between marker k - 1 and marker k (ends[k] is the
// position of marker k's FF in the segment, for k < nseg - 1; the last interval runs to the end of the segment and has to
// meet EOI). Returns the interval's status. coef: the frame's coefficient planes, zeroed; the blocks written are those
// jpeg_walk writes for the same MCUs. mem: the segment's first byte.
JPEG_HD int jpeg_walk_interval(int k, int nseg, const uint32_t* ends, const uint8_t* mem, const orbit_jpeg_desc_t& d, const JpegGeom& g,
                               const uint8_t* natural, int16_t* coef) {
    const int R = d.restart_interval, mcus = g.mcux * g.mcuy;
    const int hs0 = d.ncomp == 3 ? d.hs[0] : 1, vs0 = d.ncomp == 3 ? d.vs[0] : 1;
    JpegWalk w;
    uint32_t len = d.ecs_bytes, pos = 0;
    if (k + 1 < nseg && ends[k] < len) len = ends[k];
    if (k > 0) pos = ends[k - 1] + 2;  // (a marker has both its bytes inside the segment)
    if (pos > len) pos = len;
    w.bits.acc = 0, w.bits.n = 0, w.bits.pos = pos, w.bits.len = len, w.bits.marker = 0;
    w.mcu = k * R, w.to_restart = 0, w.next_rst = 0;
    w.dc[0] = w.dc[1] = w.dc[2] = 0;
    w.status = 0, w.done = 0;
    JpegWinSrc s;
    s.mem = mem, s.end = len;
    s.load(pos);
    const int stop = w.mcu + R < mcus ? w.mcu + R : mcus;
    for (; w.mcu < stop && !w.status; ++w.mcu) {
        const int mx = w.mcu % g.mcux, my = w.mcu / g.mcux;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= d.ncomp) continue;
            const int h = c == 0 ? hs0 : 1, v = c == 0 ? vs0 : 1;
            for (int by = 0; by < v && !w.status; ++by)
                for (int bx = 0; bx < h && !w.status; ++bx) {
                    const int blk = g.base[c] + (my * v + by) * g.wb[c] + mx * h + bx;  // < total_blocks by jpeg_geom
                    jpeg_block(w, s, d, natural, c, coef + (size_t)blk * 64);
                }
        }
    }
    if (w.status) return w.status;
    // fewer than 8 bits left, then nothing but the end of the sub-stream (which is where the scan found the next marker)
    if (k + 1 == nseg) jpeg_expect_marker(w, s, 0xD9, ORBIT_JPEG_ST_TRAILING);
    else jpeg_expect_marker(w, s, -1, ORBIT_JPEG_ST_RESTART);
    return w.status;
}

// ---- one subsequence of the segment per walker (the subsequence-parallel form, files without restart markers) --------------------
// The segment is cut into N = ceil(ecs_bytes / S) subsequences of S raw bytes; a subsequence owns the symbols that START in
// it. The state of the walk at a symbol start is (position of the next unread bit, block inside the MCU, zig-zag index, ended)
// - JpegSubState. Subsequence 0 enters with the true state; every other one with a guess (its first byte, block 0, DC next).
// A round walks every subsequence whose entry changed from that entry to the first symbol start at or behind the next
// boundary, writing nothing but its exit state, the blocks it STARTED (a DC symbol starts a block) and the sum of the DC
// differences per component; then every exit that differs from the next entry replaces it (entries are read from the round
// before: the result and the number of rounds do not depend on the order or the timing of the walkers).
// Exactness: a walk from a true state reads the symbols jpeg_walk reads there - same tables, same reader arithmetic - so by
// induction from entry 0 every entry of the fixed point (exit i == entry i + 1 for all i) is a state of the serial walk.
// Termination: entry 0 is true from the start, so exit 0 is final after round 1, entry i after round i: at most N rounds, and
// N is the loop bound. A Huffman stream self-synchronises - a walk from a wrong state falls into step with the true one
// after some symbols - which is why far fewer rounds are needed in practice. A walk from a wrong state may meet an
// invalid code or an index past 63: it then leaves through the next boundary at (block 0, DC next) with JPEG_SUB_ERROR set.
// With the entries final, an exclusive scan over blocks and DC sums gives every subsequence the ordinal of its first block and
// its DC predictors, and jpeg_sub_walk<true> decodes it once more, writing the coefficients jpeg_block writes to the blocks
// jpeg_walk puts them in. The caller checks (jpeg_sub_row_ok, the block total, jpeg_sub_last_ok, no error bit, no status of
// the write pass); when anything fails it zeroes the frame's coefficients and runs jpeg_walk over it, as the interval form does.
#define JPEG_SUB_MAX 1024          // subsequences per frame: the table is 32 KB of LDS
#define JPEG_SUB_BYTES 128         // S of the production rule, doubled until N <= JPEG_SUB_PER_ROUND
#define JPEG_SUB_PER_ROUND 256     // the threads of the kernel's block: a round then walks one subsequence per thread at most
#define JPEG_SUB_MIN_BYTES 512     // a shorter segment is walked serially (fewer than four subsequences)
#define JPEG_SUB_MIN_MCUS 64       // so is a frame of fewer MCUs: measured slower at 16 MCUs and below, faster from 64 on

#define JPEG_SUB_ENDED 0x1000u     // a marker or the end of the segment follows: nothing more to read
#define JPEG_SUB_ERROR 0x2000u     // (exit only) the walk met an invalid code, an index past 63 or ran into the end
#define JPEG_SUB_CHANGED 0x4000u   // (entry only) replaced since this subsequence was last walked
#define JPEG_SUB_STATE 0x1FFFu     // the bits two states are compared by

// pos: raw offset in the segment of the byte that holds the next unread bit - never the 00 of a stuffed FF 00 - or of the FF
// of the marker the walk ended at. st: bit inside that byte (0 = its MSB) | block inside the MCU << 3 | zig-zag index << 6 | flags
struct JpegSubState {
    uint32_t pos, st;
};
// one row of the table (32 bytes): entry, exit, and what the walk from entry to exit counted. After the scan blocks / dc0..2
// hold the sums over the subsequences before this one (unsigned: a walk from a wrong state may sum anything).
struct JpegSubRow {
    JpegSubState entry, exit;
    uint32_t blocks, dc0, dc1, dc2;
};

// S for this frame, or 0 when it does not take the form. forced: 0 = the production rule, >= 4 = that S
JPEG_HD uint32_t jpeg_sub_size(const orbit_jpeg_desc_t& d, int forced) {
    if (d.restart_interval != 0 || forced < 0) return 0;
    uint32_t S = (uint32_t)forced;
    if (forced == 0) {
        const int h = d.ncomp == 3 && d.hs[0] == 2 ? 2 : 1, v = d.ncomp == 3 && d.vs[0] == 2 ? 2 : 1;  // (as jpeg_geom, for any descriptor)
        const int64_t mcus = (int64_t)((d.width + 8 * h - 1) / (8 * h)) * ((d.height + 8 * v - 1) / (8 * v));
        if (d.ecs_bytes < JPEG_SUB_MIN_BYTES || mcus < JPEG_SUB_MIN_MCUS) return 0;
        S = JPEG_SUB_BYTES;
        while ((d.ecs_bytes - 1) / S + 1 > JPEG_SUB_PER_ROUND) S *= 2;  // (ecs_bytes < 2^31: S stays below 2^24)
    }
    if (S < 4) return 0;
    const uint32_t n = d.ecs_bytes / S + (d.ecs_bytes % S != 0);
    return n >= 2 && n <= JPEG_SUB_MAX ? S : 0;
}
JPEG_HD int jpeg_sub_count(const orbit_jpeg_desc_t& d, uint32_t S) { return (int)(d.ecs_bytes / S + (d.ecs_bytes % S != 0)); }
JPEG_HD int jpeg_sub_blocks_per_mcu(const orbit_jpeg_desc_t& d) { return d.ncomp == 3 ? d.hs[0] * d.vs[0] + 2 : 1; }

// the guessed entry of subsequence i > 0 (i = 0: the true one). mem: the segment's first byte
JPEG_HD JpegSubState jpeg_sub_guess(const uint8_t* mem, uint32_t len, uint32_t S, int i) {
    JpegSubState e;
    e.pos = (uint32_t)i * S, e.st = JPEG_SUB_CHANGED;
    if (i > 0 && e.pos < len && mem[e.pos] == 0 && mem[e.pos - 1] == 0xFF) ++e.pos;  // the 00 of FF 00 belongs to the byte before
    return e;
}

// The reader of this form: as jpeg_fill, but an FF that is not followed by 00 - a marker, fill bytes in front of one, the end of
// the segment - ends the stream with pos left ON that FF, so that the bytes in the accumulator account for every raw byte
// between the position of the next unread bit and pos. jpeg_symbol and jpeg_get_bits find either 57 bits or the end here and
// never call jpeg_fill themselves.
template <class Src>
JPEG_HD void jpeg_sub_fill(JpegBits& b, const Src& s) {
    while (b.n <= 56 && b.marker == 0) {
        if (b.pos >= b.len) {
            b.marker = -1;
            break;
        }
        const int c = s.at(b.pos);
        if (c == 0xFF) {
            const int c2 = b.pos + 1 < b.len ? s.at(b.pos + 1) : -1;
            if (c2 != 0) {
                b.marker = c2;
                break;
            }
            ++b.pos;
        }
        ++b.pos;
        b.acc = (b.acc << 8) | (uint64_t)c;
        b.n += 8;
    }
}

// The position of the next unread bit: the accumulator's last ceil(n / 8) bytes are unread (the oldest of them in part), each
// took one raw byte, two when it is FF.
JPEG_HD JpegSubState jpeg_sub_position(const JpegBits& b) {
    const int m = (b.n + 7) >> 3;
    uint64_t x = m >= 8 ? b.acc : (b.acc & ((1ull << (8 * m)) - 1ull));
    x &= x >> 1, x &= x >> 2, x &= x >> 4;  // bit 0 of every byte: the byte is FF
    x &= 0x0101010101010101ull;
    x = (x * 0x0101010101010101ull) >> 56;  // the count of those bytes
    JpegSubState p;
    p.pos = b.pos - (uint32_t)m - (uint32_t)x;
    p.st = (uint32_t)((8 - (b.n & 7)) & 7);
    return p;
}

// The block with ordinal ord in scan order -> its number in the coefficient planes, as jpeg_walk counts
JPEG_HD int jpeg_sub_block_at(const orbit_jpeg_desc_t& d, const JpegGeom& g, uint32_t ord, int& c) {
    const int bpm = jpeg_sub_blocks_per_mcu(d);
    const int mcu = (int)(ord / (uint32_t)bpm), j = (int)(ord % (uint32_t)bpm);
    const int mx = mcu % g.mcux, my = mcu / g.mcux;
    if (d.ncomp != 3) {
        c = 0;
        return g.base[0] + my * g.wb[0] + mx;
    }
    const int h = d.hs[0], v = d.vs[0];
    if (j < h * v) {
        c = 0;
        return g.base[0] + (my * v + j / h) * g.wb[0] + mx * h + j % h;
    }
    c = j - h * v + 1;
    return (c == 1 ? g.base[1] : g.base[2]) + my * g.wb[1] + mx;  // (both chroma planes are mcux x mcuy blocks)
}

// Subsequence i from row.entry to the first symbol start at or behind `limit` = (i + 1) * S. WRITE = false: fills row.exit,
// row.blocks and row.dc0..2 and returns 0. WRITE = true: row.blocks / dc0..2 are the scanned sums in front of the
// subsequence (row is not written); the coefficients go to coef, zeroed by the caller; returns ORBIT_JPEG_ST_* bits (RANGE as
// jpeg_block sets it; anything else means the walk does not repeat the one the entries came from). Every iteration
// consumes at least one bit of a stream that ends, or leaves. mem: the segment's first byte.
template <bool WRITE>
JPEG_HD int jpeg_sub_walk(JpegSubRow& row, uint32_t limit, const uint8_t* mem, const orbit_jpeg_desc_t& d, const JpegGeom& g,
                          const uint8_t* natural, int16_t* coef) {
    const JpegSubState e = row.entry;
    const int bpm = jpeg_sub_blocks_per_mcu(d), nluma = bpm == 1 ? 1 : bpm - 2;
    int blk = (int)((e.st >> 3) & 7u), k = (int)((e.st >> 6) & 63u);
    uint32_t blocks = 0, s0 = 0, s1 = 0, s2 = 0;
    uint32_t ord = 0;            // WRITE: ordinal of the block the next symbol belongs to
    int p0 = 0, p1 = 0, p2 = 0;  // WRITE: DC predictors
    int16_t* out = coef;         // WRITE: that block's coefficients
    int c = 0;                   // component of block blk
    if (WRITE) {
        ord = row.blocks - (k != 0 ? 1u : 0u);  // a block in progress was started by a subsequence before
        p0 = (int)row.dc0, p1 = (int)row.dc1, p2 = (int)row.dc2;
    }
    JpegSubState x;
    x.pos = e.pos, x.st = e.st & JPEG_SUB_STATE;
    if (!(e.st & JPEG_SUB_ENDED) && blk < bpm) {
        JpegWalk w;
        w.bits.acc = 0, w.bits.n = 0, w.bits.pos = e.pos, w.bits.len = d.ecs_bytes, w.bits.marker = 0;
        w.status = 0;
        JpegWinSrc s;
        s.mem = mem, s.end = d.ecs_bytes;
        s.load(e.pos < d.ecs_bytes ? e.pos : d.ecs_bytes);
        jpeg_sub_fill(w.bits, s);
        const int skip = (int)(e.st & 7u);
        bool fail = w.bits.n < skip, ended = false;
        if (!fail) w.bits.n -= skip;
        if (WRITE && k != 0 && !fail) {
            int cc;
            if (ord >= (uint32_t)g.total_blocks) fail = true;
            else out = coef + (size_t)jpeg_sub_block_at(d, g, ord, cc) * 64;
        }
        c = blk < nluma ? 0 : blk - nluma + 1;
        while (!fail) {
            jpeg_sub_fill(w.bits, s);
            // fewer than 8 bits, then a marker: the last symbols of the stream, or the pad bits (ones, which are no code)
            const bool tail = w.bits.marker != 0 && w.bits.n < 8;
            if (w.bits.pos - (uint32_t)((w.bits.n + 7) >> 3) >= limit) {  // (an upper bound of the position: rarely true)
                const JpegSubState p = jpeg_sub_position(w.bits);
                if (p.pos >= limit) {
                    x.pos = p.pos, x.st = p.st | ((uint32_t)blk << 3) | ((uint32_t)k << 6);
                    break;
                }
            }
            if (k == 0) {
                int sym = jpeg_symbol(w, s, d.huff[d.dc_slot[c] & 1]);
                if (sym < 0) {
                    ended = tail && w.status == ORBIT_JPEG_ST_OVERRUN;
                    break;
                }
                sym &= 15;
                int diff = 0;
                if (sym) {
                    const int v = jpeg_get_bits(w, s, sym);
                    if (w.status) break;
                    diff = jpeg_extend(v, sym);
                }
                ++blocks;
                if (c == 0) s0 += (uint32_t)diff;
                else if (c == 1) s1 += (uint32_t)diff;
                else s2 += (uint32_t)diff;
                if (WRITE) {
                    if (ord >= (uint32_t)g.total_blocks) {
                        w.status |= ORBIT_JPEG_ST_DESC;
                        break;
                    }
                    const int dcv = (int)((uint32_t)(c == 0 ? p0 : (c == 1 ? p1 : p2)) + (uint32_t)diff);  // (wraps on a damaged file)
                    if (c == 0) p0 = dcv;
                    else if (c == 1) p1 = dcv;
                    else p2 = dcv;
                    const int q0 = (int)d.qt[c][0];
                    if (dcv < -32768 || dcv > 32767 || dcv * q0 < -32768 || dcv * q0 > 32767) {
                        w.status |= ORBIT_JPEG_ST_RANGE;
                        break;
                    }
                    int cc;
                    out = coef + (size_t)jpeg_sub_block_at(d, g, ord, cc) * 64;
                    out[0] = (int16_t)dcv;
                }
                k = 1;
            } else {
                const int rs = jpeg_symbol(w, s, d.huff[2 + (d.ac_slot[c] & 1)]);
                if (rs < 0) {
                    ended = tail && w.status == ORBIT_JPEG_ST_OVERRUN;
                    break;
                }
                const int r = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                    k = r == 15 ? k + 16 : 64;
                } else {
                    k += r;
                    if (k > 63) {
                        w.status |= ORBIT_JPEG_ST_INDEX;
                        break;
                    }
                    const int raw = jpeg_get_bits(w, s, sz);
                    if (w.status) break;
                    if (WRITE) {
                        const int v = jpeg_extend(raw, sz);
                        const int pos = natural[k] & 63;
                        const int dq = v * (int)d.qt[c][pos];
                        if (dq < -32768 || dq > 32767) {
                            w.status |= ORBIT_JPEG_ST_RANGE;
                            break;
                        }
                        out[pos] = (int16_t)v;
                    }
                    ++k;
                }
            }
            if (k >= 64) {
                k = 0;
                blk = blk + 1 == bpm ? 0 : blk + 1;
                c = blk < nluma ? 0 : blk - nluma + 1;
                ++ord;
            }
        }
        if (ended) {  // in front of the marker: no symbol starts in the bits that are left
            x.pos = w.bits.pos, x.st = ((uint32_t)blk << 3) | ((uint32_t)k << 6) | JPEG_SUB_ENDED;
        } else if (fail || w.status) {
            if (WRITE) return w.status ? w.status : ORBIT_JPEG_ST_OVERRUN;
            x.pos = limit, x.st = JPEG_SUB_ERROR;
        }
    } else if (blk >= bpm) {
        x.pos = limit, x.st = JPEG_SUB_ERROR;
    }
    if (!WRITE) {
        row.exit = x;
        row.blocks = blocks, row.dc0 = s0, row.dc1 = s1, row.dc2 = s2;
    }
    return 0;
}

// after a round: exit i replaces entry i + 1 where they differ. True when it did.
JPEG_HD bool jpeg_sub_hand_over(const JpegSubRow& from, JpegSubRow& to) {
    const uint32_t st = from.exit.st & JPEG_SUB_STATE;
    if (from.exit.pos == to.entry.pos && st == (to.entry.st & JPEG_SUB_STATE)) return false;
    to.entry.pos = from.exit.pos, to.entry.st = st | JPEG_SUB_CHANGED;
    return true;
}

// row i with the sums scanned: no error bit, and the ordinal of the block its entry is in agrees with the entry's block index
JPEG_HD bool jpeg_sub_row_ok(const JpegSubRow& r, int bpm) {
    if (r.exit.st & JPEG_SUB_ERROR) return false;
    const uint32_t in_block = (r.entry.st >> 6) & 63u ? 1u : 0u;
    if (r.blocks < in_block) return false;
    return (r.blocks - in_block) % (uint32_t)bpm == ((r.entry.st >> 3) & 7u);
}

// the last exit: ended between two MCUs, and the marker there is EOI (fill bytes in front of it are allowed, as jpeg_fill has it)
JPEG_HD bool jpeg_sub_last_ok(const JpegSubState& x, const uint8_t* mem, uint32_t len) {
    if ((x.st & (JPEG_SUB_STATE | JPEG_SUB_ERROR)) != JPEG_SUB_ENDED) return false;  // (block 0, DC next, bit 0)
    uint32_t p = x.pos;
    if (p >= len || mem[p] != 0xFF) return false;
    while (p < len && mem[p] == 0xFF) ++p;
    return p < len && mem[p] == 0xD9;
}

// ---- dequantisation + inverse DCT (libjpeg jidctint.c jpeg_idct_islow) -----------------------------------------------------------
// 13 fractional bits, 2 extra bits between the passes. The arithmetic is done in uint32_t (it wraps where an int would
// overflow on a damaged file) and read as int32_t for the arithmetic shifts, which is what the hardware does either way.
JPEG_HD int32_t jpeg_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

// 1-D pass over 8 values; shift 11 for the columns, 18 for the rows
JPEG_HD void jpeg_idct_1d(const int32_t in[8], int shift, int32_t out[8]) {
    typedef uint32_t U;
    U z2 = (U)in[2], z3 = (U)in[6];
    U z1 = (z2 + z3) * 4433u;
    U tmp2 = z1 - z3 * 15137u;
    U tmp3 = z1 + z2 * 6270u;
    z2 = (U)in[0], z3 = (U)in[4];
    U tmp0 = (z2 + z3) * 8192u;
    U tmp1 = (z2 - z3) * 8192u;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)in[7], tmp1 = (U)in[5], tmp2 = (U)in[3], tmp3 = (U)in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
    z1 *= (U)-7373, z2 *= (U)-20995, z3 *= (U)-16069, z4 *= (U)-3196;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    out[0] = jpeg_descale(tmp10 + tmp3, shift), out[7] = jpeg_descale(tmp10 - tmp3, shift);
    out[1] = jpeg_descale(tmp11 + tmp2, shift), out[6] = jpeg_descale(tmp11 - tmp2, shift);
    out[2] = jpeg_descale(tmp12 + tmp1, shift), out[5] = jpeg_descale(tmp12 - tmp1, shift);
    out[3] = jpeg_descale(tmp13 + tmp0, shift), out[4] = jpeg_descale(tmp13 - tmp0, shift);
}

// libjpeg's range-limit table as arithmetic: index v & 1023 -> sample
JPEG_HD uint8_t jpeg_range_limit(int32_t v) {
    v &= 1023;
    return (uint8_t)(v < 128 ? v + 128 : (v < 512 ? 255 : (v < 896 ? 0 : v - 896)));
}

// One block: coef (natural order) * q -> 8 x 8 samples at out (rows `pitch` apart). Returns 0, or ORBIT_JPEG_ST_RANGE when
// a value between the passes leaves 16 bits or a result leaves [-512, 511]: there libjpeg's scalar code (whose table wraps)
// and its vector code (which saturates) part ways, so neither is "the" answer.
JPEG_HD int jpeg_idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, size_t pitch) {
    int32_t ws[64];
    int flag = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        int32_t in[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = (int32_t)coef[8 * k + x] * (int32_t)q[8 * k + x];
        jpeg_idct_1d(in, 11, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            ws[8 * k + x] = o[k];
            if (o[k] < -32768 || o[k] > 32767) flag = ORBIT_JPEG_ST_RANGE;
        }
    }
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int32_t o[8];
        jpeg_idct_1d(ws + 8 * y, 18, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (o[k] < -512 || o[k] > 511) flag = ORBIT_JPEG_ST_RANGE;
            out[y * pitch + k] = jpeg_range_limit(o[k]);
        }
    }
    return flag;
}

// ---- chroma upsampling + colour conversion (libjpeg jdsample.c fancy upsampling, jdcolor.c) --------------------------------------
JPEG_HD int jpeg_imin(int a, int b) { return a < b ? a : b; }
JPEG_HD int jpeg_imax(int a, int b) { return a > b ? a : b; }
JPEG_HD uint8_t jpeg_clamp8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// chroma sample of component plane p (rows `pitch` apart) at luma position (x, y). The real plane is cw x ch samples: the
// neighbours are clamped there, not at the padded block edge. A plane at most 2 samples wide is replicated, not filtered.
JPEG_HD int jpeg_chroma_at(const uint8_t* p, size_t pitch, int hs, int vs, int cw, int ch, int x, int y) {
    if (hs == 1) return p[(size_t)y * pitch + x];
    const int cx = x >> 1;
    if (vs == 1) {
        const uint8_t* row = p + (size_t)y * pitch;
        if (cw <= 2) return row[cx];
        return (x & 1) ? (3 * row[cx] + row[jpeg_imin(cx + 1, cw - 1)] + 2) >> 2 : (3 * row[cx] + row[jpeg_imax(cx - 1, 0)] + 1) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* near = p + (size_t)cy * pitch;
    if (cw <= 2) return near[cx];
    const uint8_t* far = p + (size_t)((y & 1) ? jpeg_imin(cy + 1, ch - 1) : jpeg_imax(cy - 1, 0)) * pitch;
    const int t = 3 * near[cx] + far[cx];
    if (x & 1) {
        const int r = jpeg_imin(cx + 1, cw - 1);
        return (3 * t + 3 * near[r] + far[r] + 7) >> 4;
    }
    const int l = jpeg_imax(cx - 1, 0);
    return (3 * t + 3 * near[l] + far[l] + 8) >> 4;
}

// RGB of pixel (x, y) from the frame's sample planes
JPEG_HD void jpeg_rgb_at(const orbit_jpeg_desc_t& d, const JpegGeom& g, const uint8_t* planes, int x, int y, uint8_t* rgb) {
    const int Y = planes[(size_t)g.base[0] * 64 + (size_t)y * (g.wb[0] * 8) + x];
    if (d.ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;
        return;
    }
    const int hs = d.hs[0], vs = d.vs[0];
    const int cw = hs == 2 ? (d.width + 1) / 2 : d.width, ch = vs == 2 ? (d.height + 1) / 2 : d.height;
    const int cb = jpeg_chroma_at(planes + (size_t)g.base[1] * 64, (size_t)g.wb[1] * 8, hs, vs, cw, ch, x, y) - 128;
    const int cr = jpeg_chroma_at(planes + (size_t)g.base[2] * 64, (size_t)g.wb[2] * 8, hs, vs, cw, ch, x, y) - 128;
    rgb[0] = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
    rgb[1] = jpeg_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
}

// ---- header parser (host) ----------------------------------------------------------------------------------------------------------
// Decode form of one DHT table (T.81 annex C / F.2.2.3). false: the code lengths do not form a prefix code, or a DC symbol
// exceeds 15.
inline bool jpeg_build_huff(const uint8_t counts[16], const uint8_t* vals, int nvals, bool is_dc, orbit_jpeg_huff_t& t) {
    for (int i = 0; i < 18; ++i) t.maxcode[i] = -1;
    for (int i = 0; i < 17; ++i) t.valptr[i] = 0;
    for (int i = 0; i < 256; ++i) t.huffval[i] = 0, t.look[i] = 0;
    for (int i = 0; i < nvals; ++i) {
        if (is_dc && vals[i] > 15) return false;
        t.huffval[i] = vals[i];
    }
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        if (n) {
            if (code + n >= (1 << l)) return false;  // (libjpeg refuses the all-ones code too)
            t.valptr[l] = p - code;
            for (int i = 0; i < n; ++i, ++p, ++code) {
                if (l <= 8)
                    for (int f = 0; f < (1 << (8 - l)); ++f) t.look[(code << (8 - l)) | f] = (uint16_t)((l << 8) | vals[p]);
            }
            t.maxcode[l] = code - 1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0xFFFFF;
    return true;
}

// The body of orbit_jpeg_parse. msg (of msg_bytes) receives the reason when the result is ORBIT_ERR_ARG.
inline int jpeg_parse(const uint8_t* data, size_t bytes, orbit_jpeg_desc_t* d, char* msg, size_t msg_bytes) {
    auto fail = [&](const char* why) {
        if (msg && msg_bytes) {
            size_t i = 0;
            for (; why[i] && i + 1 < msg_bytes; ++i) msg[i] = why[i];
            msg[i] = 0;
        }
        return ORBIT_ERR_ARG;
    };
    {
        uint8_t* raw = reinterpret_cast<uint8_t*>(d);
        for (size_t i = 0; i < sizeof(*d); ++i) raw[i] = 0;
    }
    if (!data || bytes < 4) return fail("jpeg_parse: not a JPEG file (shorter than 4 bytes)");
    if (bytes >= 0x7FFFFFFFu) return fail("jpeg_parse: file of 2 GB or more");
    if (data[0] != 0xFF || data[1] != 0xD8) return fail("jpeg_parse: not a JPEG file (no SOI marker)");
    static const uint8_t natural[64] = ORBIT_JPEG_NATURAL_ORDER;
    struct Dht {
        bool set;
        uint8_t counts[16], vals[256];
        int n;
    };
    Dht dht[2][4];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 4; ++b) dht[a][b].set = false;
    uint16_t qt[4][64];
    int qt_set[4] = {0, 0, 0, 0};  // 1: 8-bit, 2: 16-bit
    int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    bool have_sof = false, jfif = false, adobe = false;
    int verdict = 0;  // first out-of-scope reason met in the headers
    size_t pos = 2;
    for (;;) {
        if (pos >= bytes) return fail("jpeg_parse: the headers run past the end of the file (no scan)");
        if (data[pos] != 0xFF) return fail("jpeg_parse: not a JPEG file (no marker where one is due)");
        while (pos < bytes && data[pos] == 0xFF) ++pos;
        if (pos >= bytes) return fail("jpeg_parse: the headers run past the end of the file");
        const int m = data[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // stand-alone markers
        if (m == 0x00) return fail("jpeg_parse: not a JPEG file (FF 00 among the headers)");
        if (m == 0xD8) continue;
        if (m == 0xD9) return fail("jpeg_parse: the file ends before any scan");
        if (pos + 2 > bytes) return fail("jpeg_parse: a header runs past the end of the file");
        const size_t len = ((size_t)data[pos] << 8) | data[pos + 1];
        if (len < 2 || pos + len > bytes) return fail("jpeg_parse: a header runs past the end of the file");
        const uint8_t* seg = data + pos + 2;
        const size_t n = len - 2;
        pos += len;
        if (m == 0xE0) {
            if (n >= 14 && seg[0] == 'J' && seg[1] == 'F' && seg[2] == 'I' && seg[3] == 'F' && seg[4] == 0) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && seg[0] == 'A' && seg[1] == 'd' && seg[2] == 'o' && seg[3] == 'b' && seg[4] == 'e') adobe = true;
        } else if (m == 0xDB) {
            for (size_t i = 0; i < n;) {
                const int pq = seg[i] >> 4, tq = seg[i] & 15;
                if (tq > 3 || pq > 1) return fail("jpeg_parse: malformed quantisation table header");
                const size_t need = pq ? 128 : 64;
                if (i + 1 + need > n) return fail("jpeg_parse: a quantisation table runs past its segment");
                for (int k = 0; k < 64; ++k)
                    qt[tq][natural[k]] = pq ? (uint16_t)((seg[i + 1 + 2 * k] << 8) | seg[i + 2 + 2 * k]) : seg[i + 1 + k];
                qt_set[tq] = pq ? 2 : 1;
                i += 1 + need;
            }
        } else if (m == 0xC4) {
            for (size_t i = 0; i < n;) {
                const int tc = seg[i] >> 4, th = seg[i] & 15;
                if (tc > 1 || th > 3) return fail("jpeg_parse: malformed Huffman table header");
                if (i + 17 > n) return fail("jpeg_parse: a Huffman table runs past its segment");
                Dht& t = dht[tc][th];
                int total = 0;
                for (int k = 0; k < 16; ++k) t.counts[k] = seg[i + 1 + k], total += seg[i + 1 + k];
                if (total > 256 || i + 17 + (size_t)total > n) return fail("jpeg_parse: a Huffman table runs past its segment");
                for (int k = 0; k < total; ++k) t.vals[k] = seg[i + 17 + k];
                t.n = total, t.set = true;
                i += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {
            if (n < 2) return fail("jpeg_parse: malformed restart interval");
            d->restart_interval = (seg[0] << 8) | seg[1];
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {  // (C4 was handled above)
            if (have_sof) return fail("jpeg_parse: two frame headers");
            if (n < 6) return fail("jpeg_parse: the frame header runs past its segment");
            const int nc = seg[5];
            if (n < 6 + 3 * (size_t)nc) return fail("jpeg_parse: the frame header runs past its segment");
            have_sof = true;
            d->height = (seg[1] << 8) | seg[2];
            d->width = (seg[3] << 8) | seg[4];
            d->ncomp = nc;
            if (m == 0xC2) verdict = verdict ? verdict : ORBIT_JPEG_PROGRESSIVE;
            else if (m >= 0xC9) verdict = verdict ? verdict : ORBIT_JPEG_ARITHMETIC;
            else if (m != 0xC0) verdict = verdict ? verdict : ORBIT_JPEG_SOF_OTHER;
            if (seg[0] != 8) verdict = verdict ? verdict : ORBIT_JPEG_PRECISION;
            if (nc != 1 && nc != 3) verdict = verdict ? verdict : ORBIT_JPEG_COMPONENTS;
            if (d->width < 1 || d->height < 1 || d->width > ORBIT_RESIZE_MAX_SIZE || d->height > ORBIT_RESIZE_MAX_SIZE)
                verdict = verdict ? verdict : ORBIT_JPEG_SIZE;
            for (int c = 0; c < nc && c < 3; ++c) {
                comp_id[c] = seg[6 + 3 * c];
                d->hs[c] = seg[7 + 3 * c] >> 4, d->vs[c] = seg[7 + 3 * c] & 15;
                comp_tq[c] = seg[8 + 3 * c];
            }
        } else if (m == 0xDA) {
            if (!have_sof) return fail("jpeg_parse: a scan before the frame header");
            if (n < 1 || n < 4 + 2 * (size_t)seg[0]) return fail("jpeg_parse: the scan header runs past its segment");
            d->ecs_offset = (uint32_t)pos;
            d->ecs_bytes = (uint32_t)(bytes - pos);
            if (verdict) return d->status = verdict;
            const int nc = d->ncomp, ns = seg[0];
            if (nc == 3) {
                if (adobe && !jfif) return d->status = ORBIT_JPEG_COLORSPACE;
                if (!jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return d->status = ORBIT_JPEG_COLORSPACE;
                const int h = d->hs[0], v = d->vs[0];
                if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2)) || d->hs[1] != 1 || d->vs[1] != 1 ||
                    d->hs[2] != 1 || d->vs[2] != 1)
                    return d->status = ORBIT_JPEG_SAMPLING;
            } else if (d->hs[0] != 1 || d->vs[0] != 1) {
                return d->status = ORBIT_JPEG_SAMPLING;
            }
            if (ns != nc) return d->status = ORBIT_JPEG_MULTISCAN;
            if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return d->status = ORBIT_JPEG_MULTISCAN;
            int dc_ids[2] = {-1, -1}, ac_ids[2] = {-1, -1};
            for (int c = 0; c < nc; ++c) {
                if (seg[1 + 2 * c] != comp_id[c]) return d->status = ORBIT_JPEG_MULTISCAN;
                const int td = seg[2 + 2 * c] >> 4, ta = seg[2 + 2 * c] & 15;
                if (td > 3 || ta > 3 || !dht[0][td].set || !dht[1][ta].set) return d->status = ORBIT_JPEG_TABLES;
                if (comp_tq[c] > 3 || !qt_set[comp_tq[c]]) return d->status = ORBIT_JPEG_TABLES;
                if (qt_set[comp_tq[c]] == 2) return d->status = ORBIT_JPEG_DQT16;
                for (int k = 0; k < 64; ++k) d->qt[c][k] = qt[comp_tq[c]][k];
                int sd = -1, sa = -1;
                for (int k = 0; k < 2 && sd < 0; ++k)
                    if (dc_ids[k] == td || dc_ids[k] < 0) dc_ids[k] = td, sd = k;
                for (int k = 0; k < 2 && sa < 0; ++k)
                    if (ac_ids[k] == ta || ac_ids[k] < 0) ac_ids[k] = ta, sa = k;
                if (sd < 0 || sa < 0) return d->status = ORBIT_JPEG_TABLES;
                d->dc_slot[c] = sd, d->ac_slot[c] = sa;
            }
            for (int k = 0; k < 2; ++k) {
                if (dc_ids[k] >= 0) {
                    const Dht& t = dht[0][dc_ids[k]];
                    if (!jpeg_build_huff(t.counts, t.vals, t.n, true, d->huff[k])) return d->status = ORBIT_JPEG_TABLES;
                }
                if (ac_ids[k] >= 0) {
                    const Dht& t = dht[1][ac_ids[k]];
                    if (!jpeg_build_huff(t.counts, t.vals, t.n, false, d->huff[2 + k])) return d->status = ORBIT_JPEG_TABLES;
                }
            }
            return d->status = 0;
        }
        // every other segment (APPn, COM, DNL ..) is skipped by its length
    }
}

}  // namespace orbit_jpeg
