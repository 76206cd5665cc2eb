// Stand-alone checker of the scaled reconstruction's host twin for sanitizer builds (host only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread jpeg_host.cpp jpeg_scale_check_main.cpp -o jpeg_scale_check
//   jpeg_scale_check FILE.jpg ...
//
// For every file and every scale 2, 4, 8: the coefficients of the intact file go through jpeg_reconstruct_scaled_host and, two
// frames on two threads, through the C entry, with the coefficients, the tables, the plane workspace and the picture in heap
// blocks of exactly the sizes the geometry states, so that an access one byte outside is seen by AddressSanitizer.  A geometry
// that is not covered at a scale must be refused by the entry with the picture untouched.  Prints one line per file and scale:
// the size and the FNV-1a hash of the picture, for the caller to hold against another decoder's.  Exit status 1 when a file does
// not decode, the two ways differ or a refusal writes.
#include "jpeg_host.h"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace tstar {
void set_error(const std::string&) {}
}  // namespace tstar

extern "C" {
int tstar_jpeg_sizes_scaled(int W, int H, int ncomp, int hs, int vs, int scale, size_t* out4);
int tstar_jpeg_reconstruct_scaled_host(const int16_t* coef, const uint16_t* quant, int n, int W, int H, int ncomp, int hs, int vs,
                                       int scale, uint8_t* rgb, int threads);
}

using namespace tstar;

static uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        std::vector<uint8_t> d;
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + got);
        fclose(f);
        char msg[160];
        JpegGeom g;
        if (jpeg_probe(d.data(), d.size(), &g, msg, sizeof(msg)) != JPEG_OK) { printf("%s probe: %s\n", argv[a], msg); bad = 1; continue; }
        const size_t per = g.blocks() * 64;
        std::vector<int16_t> coef(2 * per);                                 // two frames: the same picture twice
        std::vector<uint16_t> quant(2 * 192);
        if (jpeg_entropy(d.data(), d.size(), g, coef.data(), quant.data(), msg, sizeof(msg)) != JPEG_OK) {
            printf("%s entropy: %s\n", argv[a], msg);
            bad = 1;
            continue;
        }
        memcpy(coef.data() + per, coef.data(), per * sizeof(int16_t));
        memcpy(quant.data() + 192, quant.data(), 192 * sizeof(uint16_t));
        for (int scale = 2; scale <= 8; scale *= 2) {
            const JpegScaledGeom sg{g, scale};
            size_t out4[4] = {0, 0, 0, 0};
            if (tstar_jpeg_sizes_scaled(g.W, g.H, g.ncomp, g.hs, g.vs, scale, out4) != 0 || out4[0] != (size_t)sg.ow() ||
                out4[1] != (size_t)sg.oh() || out4[2] != sg.plane_bytes() || out4[3] != (size_t)sg.covered()) {
                printf("%s scale=%d: the sizes entry disagrees with the geometry\n", argv[a], scale);
                bad = 1;
                continue;
            }
            const size_t frame = (size_t)sg.ow() * sg.oh() * 3;
            std::vector<uint8_t> two(2 * frame, 0xA5);
            const int rc = tstar_jpeg_reconstruct_scaled_host(coef.data(), quant.data(), 2, g.W, g.H, g.ncomp, g.hs, g.vs, scale, two.data(), 2);
            if (!sg.covered()) {
                bool untouched = rc != 0;
                for (uint8_t v : two) untouched = untouched && v == 0xA5;
                if (!untouched) bad = 1;
                printf("%s scale=%d covered=0 refused=%d\n", argv[a], scale, (int)untouched);
                continue;
            }
            std::vector<uint8_t> scratch(sg.plane_bytes(), 0xEE), rgb(frame, 0xA5);
            jpeg_reconstruct_scaled_host(sg, coef.data(), quant.data(), scratch.data(), rgb.data());
            const bool same = rc == 0 && memcmp(two.data(), rgb.data(), frame) == 0 && memcmp(two.data() + frame, rgb.data(), frame) == 0;
            if (!same) bad = 1;
            printf("%s scale=%d covered=1 size=%dx%d same=%d fnv=%016llx\n", argv[a], scale, sg.ow(), sg.oh(), (int)same,
                   (unsigned long long)fnv1a(rgb.data(), frame));
        }
    }
    return bad;
}
