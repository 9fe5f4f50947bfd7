// The device JPEG decoder's code on the CPU: parses one file with the host parser and decodes it with the functions of
// csrc/jpeg_core.h that the kernels of csrc/jpeg.hip call - entropy walker, inverse DCT, upsampling + colour conversion.
// Built with -fsanitize=address,undefined by tests/test_jpeg_host.py and run on valid and on damaged files: every buffer is
// a heap allocation of exactly the size the device gives it, so a read or write outside it is reported.
//   jpeg_host_check IN.jpg OUT.rgb   ->   prints "parse P status S width W height H ncomp N", writes H * W * 3 bytes when
//                                         P == 0 and S == 0; exit code 0 unless a file cannot be read or written
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
    int status = 0;
    if (parse == 0) {
        JpegGeom g;
        if (!jpeg_geom(*d, g) || (size_t)g.total_blocks > jpeg_cap_blocks(d->height, d->width)) {
            status = ORBIT_JPEG_ST_DESC;
        } else {
            static const uint8_t natural[64] = ORBIT_JPEG_NATURAL_ORDER;
            // the entropy-coded segment as its own allocation: the walker may not read in front of it or behind it
            uint8_t* ecs = (uint8_t*)malloc(d->ecs_bytes ? d->ecs_bytes : 1);
            memcpy(ecs, file + d->ecs_offset, d->ecs_bytes);
            int16_t* coef = (int16_t*)calloc((size_t)g.total_blocks * 64, sizeof(int16_t));
            uint8_t* planes = (uint8_t*)malloc((size_t)g.total_blocks * 64);
            JpegWalk w;
            jpeg_walk_init(w, *d);
            HostSrc src{ecs};
            // in slices of one staging tile, as the kernel resumes the walker
            for (uint32_t stop = ORBIT_JPEG_STAGE_BYTES - 1; !w.done; stop += ORBIT_JPEG_STAGE_BYTES)
                jpeg_walk(w, src, *d, g, natural, coef, stop);
            status = w.status;
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
            free(ecs);
        }
    }
    printf("parse %d status %d width %d height %d ncomp %d%s%s\n", parse, status, d->width, d->height, d->ncomp, msg[0] ? " : " : "", msg);
    free(d);
    free(file);
    return 0;
}
