// Stand-alone checker of the JPEG host stage for sanitizer builds (host only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread jpeg_host.cpp jpeg_check_main.cpp -o jpeg_check
//   jpeg_check FILE.jpg ...
//
// For every file: the intact bytes must decode; then the decoder is driven over the file truncated at every 97th offset,
// over single flipped bytes in the entropy data and over every header byte overwritten in three ways.  Each buffer is an
// exact-size heap copy, so that a read one byte past the input is seen by AddressSanitizer.  Prints one line per file;
// exit status 1 when an intact file fails or a truncated one decodes.
#include "jpeg_host.h"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace tstar {
void set_error(const std::string&) {}
}  // namespace tstar

using namespace tstar;

// decode an exact-size copy of [d, d + n) -> status
static int run(const uint8_t* d, size_t n, std::vector<int16_t>& coef, std::vector<uint8_t>& scratch, std::vector<uint8_t>& rgb) {
    std::vector<uint8_t> copy(d, d + n);                 // heap block of exactly n bytes (redzones on both sides)
    char msg[160];
    JpegGeom g;
    int rc = jpeg_probe(copy.data(), n, &g, msg, sizeof(msg));
    if (rc != JPEG_OK) return rc;
    if ((size_t)g.W * g.H > (size_t)1 << 24) return JPEG_UNCOVERED;          // a mutated SOF asking for a huge picture: not this tool's business
    coef.assign(g.blocks() * 64, 0);
    uint16_t quant[192];
    rc = jpeg_entropy(copy.data(), n, g, coef.data(), quant, msg, sizeof(msg));
    if (rc != JPEG_OK) return rc;
    scratch.assign(g.plane_bytes(), 0);
    rgb.assign((size_t)g.W * g.H * 3, 0);
    jpeg_reconstruct_host(g, coef.data(), quant, scratch.data(), rgb.data());
    jpeg_frame_end(copy.data(), n, 0);
    return JPEG_OK;
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
        std::vector<int16_t> coef;
        std::vector<uint8_t> scratch, rgb;
        const int intact = run(d.data(), d.size(), coef, scratch, rgb);
        // start of the entropy data: after the first SOS segment
        size_t sos = 0;
        for (size_t p = 2; p + 4 <= d.size();) {
            if (d[p] != 0xFF) break;
            const int m = d[p + 1];
            const size_t L = ((size_t)d[p + 2] << 8) | d[p + 3];
            if (m == 0xDA) { sos = p + 2 + L; break; }
            p += 2 + L;
        }
        int trunc_ok = 0, trunc_n = 0, flip_err = 0, flip_n = 0, hdr_n = 0;
        for (size_t n = 0; n < d.size(); n += 97) {
            ++trunc_n;
            if (run(d.data(), n, coef, scratch, rgb) == JPEG_OK) ++trunc_ok;
        }
        if (sos && sos < d.size()) {
            const size_t span = d.size() - 2 - sos, step = span / 64 + 1;
            std::vector<uint8_t> m(d);
            for (size_t p = sos; p < d.size() - 2; p += step) {
                m[p] ^= 0xFF;
                ++flip_n;
                if (run(m.data(), m.size(), coef, scratch, rgb) != JPEG_OK) ++flip_err;
                m[p] ^= 0xFF;
            }
            const uint8_t over[3] = {0x00, 0xFF, 0x80};
            for (size_t p = 2; p < sos; ++p)
                for (int k = 0; k < 3; ++k) {
                    const uint8_t keep = m[p];
                    m[p] = k == 2 ? (uint8_t)(keep ^ 0x80) : over[k];
                    ++hdr_n;
                    run(m.data(), m.size(), coef, scratch, rgb);
                    m[p] = keep;
                }
        }
        printf("%s intact=%d truncated_decoded=%d/%d flips_rejected=%d/%d header_mutations=%d\n", argv[a], intact, trunc_ok, trunc_n,
               flip_err, flip_n, hdr_n);
        if (intact != JPEG_OK || trunc_ok) bad = 1;
    }
    return bad;
}
