// The device JPEG encoder's code on the CPU: encodes one raw RGB frame with the functions of csrc/jpeg_enc_core.h that the
// kernels of csrc/jpeg_enc.hip call - colour conversion + downsampling per strip, forward DCT + quantisation per block, the
// code walk per block (once counting, once writing), byte stuffing per chunk - in the kernels' order, serially.
// Built with -fsanitize=address,undefined by tests/test_jpeg_enc_host.py and compared with Pillow's bytes: every buffer is a
// heap allocation of exactly the size the device gives it, so a read or write outside it is reported.
//   jpeg_enc_host_check IN.rgb H W quality restart_rows [comment] OUT.jpg   ->   prints "bytes N bound M"; exit code 0 unless
//                                                                                an argument is bad or a file cannot be read
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "jpeg_enc_core.h"

using namespace orbit_jpegenc;

struct HostMem {
    uint32_t* buf;
    void or_word(uint32_t i, uint32_t v) const { buf[i] |= v; }
    void set_word(uint32_t i, uint32_t v) const { buf[i] = v; }
};

int main(int argc, char** argv) {
    if (argc != 7 && argc != 8) {
        fprintf(stderr, "usage: %s IN.rgb H W quality restart_rows [comment] OUT.jpg\n", argv[0]);
        return 2;
    }
    const int H = atoi(argv[2]), W = atoi(argv[3]), quality = atoi(argv[4]), rows = atoi(argv[5]);
    const char* comment = argc == 8 ? argv[6] : "";
    const size_t clen = strlen(comment);
    if (H < 1 || W < 1 || H > 16384 || W > 16384 || quality < 1 || quality > 100 || rows < 0 || clen > (size_t)ENC_MAX_COMMENT) return 2;
    const size_t in_bytes = (size_t)H * W * 3;
    uint8_t* rgb = (uint8_t*)malloc(in_bytes);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(rgb, 1, in_bytes, f) != in_bytes) return 2;
    fclose(f);

    orbit_jpeg_enc_t* p = (orbit_jpeg_enc_t*)malloc(sizeof(orbit_jpeg_enc_t));
    enc_params(quality, rows, p);
    const EncGeom g = enc_geom(H, W, rows);
    if (g.interval > 65535) return 2;
    const size_t ypitch = 16 * (size_t)g.mcux, cpitch = 8 * (size_t)g.mcux, cap = enc_unstuffed_cap(g.blocks);
    uint8_t* yp = (uint8_t*)malloc((size_t)g.mcus * 256);
    uint8_t* cbp = (uint8_t*)malloc((size_t)g.mcus * 64);
    uint8_t* crp = (uint8_t*)malloc((size_t)g.mcus * 64);
    int16_t* coef = (int16_t*)malloc((size_t)g.blocks * 128);
    uint32_t* sums = (uint32_t*)malloc((size_t)g.blocks * 4);
    uint32_t* seg = (uint32_t*)malloc((size_t)(g.nseg + 2) * 4);
    uint32_t* bits = (uint32_t*)malloc(cap);
    uint32_t* ff = (uint32_t*)malloc(cap / ENC_CHUNK * 4);
    const size_t bound = enc_bound(H, W, rows, clen);
    uint8_t* out = (uint8_t*)malloc(bound);

    // enc_color_kernel: one strip of 8 x 2 pixels per step
    for (int qy = 0; qy < 8 * g.mcuy; ++qy)
        for (int sx = 0; sx < 2 * g.mcux; ++sx) {
            uint32_t ylo[2], yhi[2], cb4, cr4;
            enc_strip_at(rgb, H, W, sx, qy, ylo, yhi, cb4, cr4);
            memcpy(yp + (size_t)(2 * qy) * ypitch + 8 * sx, ylo, 8);
            memcpy(yp + (size_t)(2 * qy + 1) * ypitch + 8 * sx, yhi, 8);
            memcpy(cbp + (size_t)qy * cpitch + 4 * sx, &cb4, 4);
            memcpy(crp + (size_t)qy * cpitch + 4 * sx, &cr4, 4);
        }
    // enc_dct_kernel
    uint32_t q32[2][64], r32[2][64];
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) q32[t][i] = p->qt[t][i], r32[t][i] = p->qrecip[t][i];
    for (int blk = 0; blk < g.blocks; ++blk) {
        EncBlockPos pos = enc_block_pos(g, blk);
        const bool dummy = pos.dummy;
        for (int b = blk; pos.dummy;) pos = enc_block_pos(g, --b);
        const size_t pitch = pos.comp == 0 ? ypitch : cpitch;
        const uint8_t* in = (pos.comp == 0 ? yp : (pos.comp == 1 ? cbp : crp)) + (size_t)pos.by * 8 * pitch + (size_t)pos.bx * 8;
        int16_t* zz = coef + (size_t)blk * 64;
        enc_fdct_block(in, pitch, q32[pos.comp ? 1 : 0], r32[pos.comp ? 1 : 0], zz);
        if (dummy)
            for (int k = 1; k < 64; ++k) zz[k] = 0;
    }
    // enc_size_kernel, enc_scan_kernel
    for (int blk = 0; blk < g.blocks; ++blk) sums[blk] = enc_block_bits(g, blk, coef, &p->dc[0][0], &p->ac[0][0]);
    for (int blk = 1; blk < g.blocks; ++blk) sums[blk] += sums[blk - 1];
    seg[0] = 0;
    for (int s = 0; s < g.nseg; ++s) seg[s + 1] = seg[s] + enc_seg_bytes(g, sums, s);
    const uint32_t total = seg[g.nseg];
    {
        const size_t words = total / 4 + 1 < cap / 4 ? total / 4 + 1 : cap / 4;
        memset(bits, 0, words * 4);
    }
    // enc_pack_kernel
    for (int blk = 0; blk < g.blocks; ++blk) enc_pack_block(g, blk, coef, sums, seg, &p->dc[0][0], &p->ac[0][0], HostMem{bits});
    // enc_ff_kernel
    const uint8_t* stream = (const uint8_t*)bits;
    uint32_t nff = 0;
    for (uint32_t c0 = 0; c0 < total; c0 += ENC_CHUNK) {
        ff[c0 / ENC_CHUNK] = nff;
        nff += enc_count_ff(stream, c0, c0 + ENC_CHUNK < total ? c0 + ENC_CHUNK : total);
    }
    seg[g.nseg + 1] = nff;
    // enc_assemble_kernel
    size_t hlen = enc_header_head(out);
    if (clen) {
        out[hlen++] = 0xFF, out[hlen++] = 0xFE, out[hlen++] = (uint8_t)((clen + 2) >> 8), out[hlen++] = (uint8_t)(clen + 2);
        memcpy(out + hlen, comment, clen);
        hlen += clen;
    }
    hlen += enc_header_tail(p, H, W, out + hlen);
    for (uint32_t c0 = 0; c0 < total; c0 += ENC_CHUNK)
        enc_stuff_chunk(stream, c0, c0 + ENC_CHUNK < total ? c0 + ENC_CHUNK : total, ff[c0 / ENC_CHUNK], seg, g.nseg, out + hlen);
    const size_t n = hlen + total + seg[g.nseg + 1] + 2 * (size_t)(g.nseg - 1) + 2;
    out[n - 2] = 0xFF, out[n - 1] = 0xD9;

    FILE* o = fopen(argv[argc - 1], "wb");
    if (!o || fwrite(out, 1, n, o) != n) return 2;
    fclose(o);
    printf("bytes %zu bound %zu\n", n, bound);
    free(out), free(ff), free(bits), free(seg), free(sums), free(coef), free(crp), free(cbp), free(yp), free(p), free(rgb);
    return 0;
}
