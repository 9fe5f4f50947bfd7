// The interval-parallel form of the device JPEG decoder on the CPU: parses one file, walks it serially with jpeg_walk as the
// reference, and then runs the model of what the entropy kernel of csrc/jpeg.hip does with a restart-marked frame, from the
// same functions of csrc/jpeg_core.h - the marker scan in 16-byte lane slices of 1 KB tiles, the rule that admits a frame,
// jpeg_walk_interval for every interval (in DESCENDING order: no interval may depend on one before it), and the serial walk
// again when an interval reports a status. Built with -fsanitize=address,undefined by tests/test_jpeg_par_host.py; every
// buffer is a heap allocation of exactly the size the device gives it, so a read or write outside it is reported.
//   jpeg_par_host_check IN.jpg OUT.rgb   ->   prints "parse P serial S parallel Q taken T equal E nseg N idct I width W height H";
//                                             writes the H * W * 3 bytes decoded from the model's coefficients when P == 0
//                                             and Q == 0 and I == 0; exit code 0 unless a file cannot be read or written
// taken: 0 serial, 1 one walker per interval, 2 that was tried and the frame walked serially again. equal: 1 when the
// model's coefficients are the serial walk's.
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

// the scan as the wave runs it: tile by tile, lane by lane, markers appended in stream order
static bool scan_markers(const uint8_t* ecs, uint32_t len, int nseg, uint32_t* ends) {
    const uint32_t T = ORBIT_JPEG_STAGE_BYTES;
    int count = 0;
    bool bad = false;
    for (uint32_t t = 0; t < (len + T - 1) / T && count < nseg; ++t)
        for (int lane = 0; lane < 64; ++lane) {
            const uint32_t o = t * T + 16u * lane;
            const int n = o >= len ? 0 : (len - o < 16u ? (int)(len - o) : 16);
            uint32_t v[4] = {0, 0, 0, 0};
            for (int j = 0; j < n; ++j) v[j >> 2] |= (uint32_t)ecs[o + j] << (8 * (j & 3));
            const int next = (n == 16 && o + 16 < len) ? ecs[o + 16] : -1;
            const uint32_t m = jpeg_scan_slice(v[0], v[1], v[2], v[3], n, next);
            for (int j = 0; j < 16; ++j) {
                if (!((m >> j) & 1u)) continue;
                if (count < nseg) {
                    const int code = j < 15 ? jpeg_slice_byte(v[0], v[1], v[2], v[3], j + 1) : next;
                    if (!jpeg_par_marker_ok(count, code, nseg)) bad = true;
                    ends[count] = o + (uint32_t)j;
                }
                ++count;
            }
        }
    return !bad && count >= nseg;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN.jpg OUT.rgb\n", argv[0]);
        return 2;
    }
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
    int serial = 0, parallel = 0, taken = 0, equal = 0, nseg = 0, idct = 0;
    if (parse == 0) {
        JpegGeom g;
        if (!jpeg_geom(*d, g) || (size_t)g.total_blocks > jpeg_cap_blocks(d->height, d->width)) {
            serial = parallel = ORBIT_JPEG_ST_DESC;
        } else {
            static const uint8_t natural[64] = ORBIT_JPEG_NATURAL_ORDER;
            const size_t ncoef = (size_t)g.total_blocks * 64;
            // the entropy-coded segment as its own allocation: no walker may read in front of it or behind it
            uint8_t* ecs = (uint8_t*)malloc(d->ecs_bytes ? d->ecs_bytes : 1);
            memcpy(ecs, file + d->ecs_offset, d->ecs_bytes);
            int16_t* ref = (int16_t*)calloc(ncoef, sizeof(int16_t));
            serial = serial_walk(*d, g, natural, ecs, ref);

            int16_t* coef = (int16_t*)calloc(ncoef, sizeof(int16_t));
            uint32_t* ends = (uint32_t*)malloc(JPEG_PAR_MAX_INTERVALS * sizeof(uint32_t));
            nseg = jpeg_par_intervals(*d, g);
            if (nseg != 0 && scan_markers(ecs, d->ecs_bytes, nseg, ends)) {
                taken = 1;
                for (int k = nseg - 1; k >= 0; --k) parallel |= jpeg_walk_interval(k, nseg, ends, ecs, *d, g, natural, coef);
                if (parallel != 0) {
                    taken = 2;
                    memset(coef, 0, ncoef * sizeof(int16_t));
                }
            }
            if (taken != 1) parallel = serial_walk(*d, g, natural, ecs, coef);
            equal = memcmp(ref, coef, ncoef * sizeof(int16_t)) == 0;

            int status = parallel;  // (from here on with the bits of the inverse DCT, printed as "idct")
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
            idct = status & ~parallel;
            if (status == 0) {
                std::vector<uint8_t> rgb((size_t)d->width * d->height * 3);
                for (int y = 0; y < d->height; ++y)
                    for (int x = 0; x < d->width; ++x) jpeg_rgb_at(*d, g, planes, x, y, &rgb[((size_t)y * d->width + x) * 3]);
                FILE* o = fopen(argv[2], "wb");
                if (!o || fwrite(rgb.data(), 1, rgb.size(), o) != rgb.size()) return 2;
                fclose(o);
            }
            free(planes);
            free(ends);
            free(coef);
            free(ref);
            free(ecs);
        }
    }
    printf("parse %d serial %d parallel %d taken %d equal %d nseg %d idct %d width %d height %d%s%s\n", parse, serial, parallel, taken, equal, nseg, idct,
           d->width, d->height, msg[0] ? " : " : "", msg);
    free(d);
    free(file);
    return 0;
}
