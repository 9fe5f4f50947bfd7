// The subsequence-parallel form of the device JPEG decoder on the CPU: parses one file, walks it serially with jpeg_walk as
// the reference, and then runs the model of what jpeg_entropy_sub_kernel of csrc/jpeg.hip does with a frame without restart
// markers, from the same functions of csrc/jpeg_core.h - the rule that admits a frame, the guessed entries, the Jacobi rounds
// of jpeg_sub_walk<false> with the lanes emulated in order (every walk of a round first, then every hand-over, so a round reads
// the entries of the round before), the exclusive scan, the checks, jpeg_sub_walk<true> for every subsequence (in DESCENDING
// order: the write pass of one may not depend on another's), and the serial walk again when anything fails. Built with
// -fsanitize=address,undefined by tests/test_jpeg_sub_host.py; every buffer is a heap allocation of exactly the size the
// device gives it - the table has N rows - so a read or write outside it is reported.
//   jpeg_sub_host_check IN.jpg OUT.rgb SUB_BYTES
//       prints "parse P serial S sub Q taken T equal E n N rounds R decodes D idct I width W height H"; writes the H * W * 3
//       bytes decoded from the model's coefficients when P == 0 and Q == 0 and I == 0; exit code 0 unless a file cannot be read
//       or written or SUB_BYTES is neither 0 (the production rule) nor >= 4
// taken: 0 serial, 1 the frame is the interval form's by its geometry (its markers are not looked at here), 3 one walker per subsequence, 4 that was tried
// and the frame walked serially again. equal: 1 when the model's coefficients are the serial walk's. decodes: walks of all rounds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "jpeg_core.h"

using namespace orbit_jpeg;

struct HostSrc {
    const uint8_t* p;
    uint8_t at(uint32_t pos) const { return p[pos]; }
};

static int serial_walk(const orbit_jpeg_desc_t& d, const JpegGeom& g, const uint8_t* natural, const uint8_t* ecs, int16_t* coef) {
    JpegWalk w;
    jpeg_walk_init(w, d);
    HostSrc src{ecs};
    for (uint32_t stop = ORBIT_JPEG_STAGE_BYTES - 1; !w.done; stop += ORBIT_JPEG_STAGE_BYTES) jpeg_walk(w, src, d, g, natural, coef, stop);
    return w.status;
}

// true: the frame's coefficients are in coef and its status is 0
static bool sub_frame(const orbit_jpeg_desc_t& d, const JpegGeom& g, const uint8_t* natural, const uint8_t* ecs, uint32_t S, int n,
                      int16_t* coef, int& rounds, long& decodes) {
    const uint32_t len = d.ecs_bytes;
    JpegSubRow* rows = (JpegSubRow*)malloc((size_t)n * sizeof(JpegSubRow));
    for (int i = 0; i < n; ++i) {
        rows[i].entry = jpeg_sub_guess(ecs, len, S, i);
        rows[i].exit.pos = 0, rows[i].exit.st = 0;
        rows[i].blocks = rows[i].dc0 = rows[i].dc1 = rows[i].dc2 = 0;
    }
    rounds = 0, decodes = 0;
    while (rounds < n) {
        int walked = 0;
        for (int i = 0; i < n; ++i)
            if (rows[i].entry.st & JPEG_SUB_CHANGED) {
                rows[i].entry.st &= ~JPEG_SUB_CHANGED;
                jpeg_sub_walk<false>(rows[i], (uint32_t)(i + 1) * S, ecs, d, g, natural, nullptr);
                ++walked;
            }
        if (!walked) break;
        ++rounds, decodes += walked;
        for (int i = 0; i + 1 < n; ++i) jpeg_sub_hand_over(rows[i], rows[i + 1]);
    }
    uint32_t blocks = 0, s0 = 0, s1 = 0, s2 = 0;
    for (int i = 0; i < n; ++i) {
        const JpegSubRow r = rows[i];
        rows[i].blocks = blocks, rows[i].dc0 = s0, rows[i].dc1 = s1, rows[i].dc2 = s2;
        blocks += r.blocks, s0 += r.dc0, s1 += r.dc1, s2 += r.dc2;
    }
    bool ok = blocks == (uint32_t)g.total_blocks && jpeg_sub_last_ok(rows[n - 1].exit, ecs, len);
    const int bpm = jpeg_sub_blocks_per_mcu(d);
    for (int i = 0; i < n; ++i) ok = ok && jpeg_sub_row_ok(rows[i], bpm);
    if (ok) {
        int st = 0;
        for (int i = n - 1; i >= 0; --i) st |= jpeg_sub_walk<true>(rows[i], (uint32_t)(i + 1) * S, ecs, d, g, natural, coef);
        ok = st == 0;
    }
    free(rows);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s IN.jpg OUT.rgb SUB_BYTES\n", argv[0]);
        return 2;
    }
    const int sub_bytes = atoi(argv[3]);
    if (sub_bytes != 0 && sub_bytes < 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* file = (uint8_t*)malloc(size > 0 ? (size_t)size : 1);
    if (size > 0 && fread(file, 1, (size_t)size, f) != (size_t)size) return 2;
    fclose(f);

    orbit_jpeg_desc_t* d = (orbit_jpeg_desc_t*)malloc(sizeof(orbit_jpeg_desc_t));
    char msg[160] = "";
    const int parse = jpeg_parse(file, (size_t)size, d, msg, sizeof(msg));
    int serial = 0, sub = 0, taken = 0, equal = 0, n = 0, rounds = 0, idct = 0;
    long decodes = 0;
    if (parse == 0) {
        JpegGeom g;
        if (!jpeg_geom(*d, g) || (size_t)g.total_blocks > jpeg_cap_blocks(d->height, d->width)) {
            serial = sub = ORBIT_JPEG_ST_DESC;
        } else {
            static const uint8_t natural[64] = ORBIT_JPEG_NATURAL_ORDER;
            const size_t ncoef = (size_t)g.total_blocks * 64;
            // the entropy-coded segment as its own allocation: no walker may read in front of it or behind it
            uint8_t* ecs = (uint8_t*)malloc(d->ecs_bytes ? d->ecs_bytes : 1);
            memcpy(ecs, file + d->ecs_offset, d->ecs_bytes);
            int16_t* ref = (int16_t*)calloc(ncoef, sizeof(int16_t));
            serial = serial_walk(*d, g, natural, ecs, ref);

            int16_t* coef = (int16_t*)calloc(ncoef, sizeof(int16_t));
            const uint32_t S = jpeg_sub_size(*d, sub_bytes);
            if (jpeg_par_intervals(*d, g) != 0) {
                taken = 1;  // (the interval form's: tools/jpeg_par_host_check.cpp is its model)
            } else if (S != 0) {
                n = jpeg_sub_count(*d, S);
                taken = 3;
                if (!sub_frame(*d, g, natural, ecs, S, n, coef, rounds, decodes)) {
                    taken = 4;
                    memset(coef, 0, ncoef * sizeof(int16_t));
                }
            }
            if (taken != 3) sub = serial_walk(*d, g, natural, ecs, coef);
            equal = memcmp(ref, coef, ncoef * sizeof(int16_t)) == 0;

            int status = sub;  // (from here on with the bits of the inverse DCT, printed as "idct")
            uint8_t* planes = (uint8_t*)malloc(ncoef);
            if (status == 0) {
                for (int c = 0; c < d->ncomp; ++c)
                    for (int by = 0; by < g.hb[c]; ++by)
                        for (int bx = 0; bx < g.wb[c]; ++bx) {
                            const size_t blk = (size_t)g.base[c] + (size_t)by * g.wb[c] + bx;
                            const size_t pitch = (size_t)g.wb[c] * 8;
                            status |= jpeg_idct_block(coef + blk * 64, d->qt[c], planes + (size_t)g.base[c] * 64 + (size_t)by * 8 * pitch + (size_t)bx * 8,
                                                      pitch);
                        }
            }
            idct = status & ~sub;
            if (status == 0) {
                std::vector<uint8_t> rgb((size_t)d->width * d->height * 3);
                for (int y = 0; y < d->height; ++y)
                    for (int x = 0; x < d->width; ++x) jpeg_rgb_at(*d, g, planes, x, y, &rgb[((size_t)y * d->width + x) * 3]);
                FILE* o = fopen(argv[2], "wb");
                if (!o || fwrite(rgb.data(), 1, rgb.size(), o) != rgb.size()) return 2;
                fclose(o);
            }
            free(planes);
            free(coef);
            free(ref);
            free(ecs);
        }
    }
    printf("parse %d serial %d sub %d taken %d equal %d n %d rounds %d decodes %ld idct %d width %d height %d%s%s\n", parse, serial, sub, taken,
           equal, n, rounds, decodes, idct, d->width, d->height, msg[0] ? " : " : "", msg);
    free(d);
    free(file);
    return 0;
}
