// Stand-alone checker of the JPEG encoder's host twin for sanitizer builds (host only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread
//       jpeg_enc_host.cpp jpeg_host.cpp jpeg_enc_check_main.cpp -o jpeg_enc_check
//   jpeg_enc_check CASE ...
//
// A case file: five little-endian int32 {W, H, quality, hs, vs}, then the frame, W * H * 3 bytes of RGB.  (jpeg_host.cpp is
// linked for jpeg_thread_allowance only.)  For every case the frame, the coefficients and every output live in heap blocks of
// EXACT size, so that AddressSanitizer sees a read or write one byte outside them.  The whole-frame entry runs at the exact
// capacity (must succeed), one byte less (must report a short slot), zero, and with two frames on the thread pool; the two
// stages and the header writer run separately and must give the same bytes.  Prints one line per case; exit status 1 when
// a result is not what it must be.
#include "../../include/tstar_hip.h"
#include "jpeg_enc_host.h"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace tstar {
void set_error(const std::string&) {}
}  // namespace tstar

using namespace tstar;

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        int32_t h5[5];
        if (fread(h5, sizeof(int32_t), 5, f) != 5) { fprintf(stderr, "%s: short case header\n", argv[a]); return 2; }
        const int W = h5[0], H = h5[1], quality = h5[2], hs = h5[3], vs = h5[4];
        const JpegGeom g{W, H, 3, hs, vs};
        if (!jpeg_enc_geom_ok(g) || (size_t)W * H > (size_t)1 << 22) { fprintf(stderr, "%s: bad case geometry\n", argv[a]); return 2; }
        std::vector<uint8_t> frame((size_t)W * H * 3);
        if (fread(frame.data(), 1, frame.size(), f) != frame.size()) { fprintf(stderr, "%s: short frame\n", argv[a]); return 2; }
        fclose(f);
        const int32_t idx1[1] = {0}, idx2[2] = {0, 0};
        uint32_t len[2] = {0, 0};
        int32_t st[2] = {-1, -1};
        uint64_t counters[JPEG_ENC_N_COUNTERS] = {0, 0, 0, 0, 0};
        // generous capacity -> the reference bytes and their length
        std::vector<uint8_t> full(kJpegEncHeaderBytes + jpeg_enc_max_scan_bytes(g));
        int ok = tstar_jpeg_encode_host(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, full.data(), full.size(), len, st, 1, counters) == 0 &&
                 st[0] == JPEG_ENC_OK && len[0] > (uint32_t)kJpegEncHeaderBytes;
        const size_t L = len[0];
        // exact capacity
        std::vector<uint8_t> exact(L);
        ok = ok && tstar_jpeg_encode_host(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, exact.data(), L, len, st, 1, nullptr) == 0 &&
             st[0] == JPEG_ENC_OK && len[0] == L && memcmp(exact.data(), full.data(), L) == 0;
        // one byte short: a status, the length it would have taken, and not a byte written
        std::vector<uint8_t> shorter(L - 1, 0xA5);
        ok = ok && tstar_jpeg_encode_host(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, shorter.data(), L - 1, len, st, 1, nullptr) == 0 &&
             st[0] == JPEG_ENC_SHORT && len[0] == L;
        for (uint8_t b : shorter) ok = ok && b == 0xA5;
        // zero capacity (a one-byte block the call must not touch)
        std::vector<uint8_t> none(1, 0xA5);
        ok = ok && tstar_jpeg_encode_host(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, none.data(), 0, len, st, 1, nullptr) == 0 &&
             st[0] == JPEG_ENC_SHORT && none[0] == 0xA5;
        // two frames on two workers, slots back to back
        std::vector<uint8_t> two(2 * L);
        ok = ok && tstar_jpeg_encode_host(frame.data(), 1, H, W, idx2, 2, quality, hs, vs, two.data(), L, len, st, 2, nullptr) == 0 &&
             st[0] == JPEG_ENC_OK && st[1] == JPEG_ENC_OK && memcmp(two.data(), full.data(), L) == 0 && memcmp(two.data() + L, full.data(), L) == 0;
        // the stages separately: exact-size coefficients, exact-size scan, exact-size header
        std::vector<int16_t> coef(g.blocks() * 64);
        std::vector<uint16_t> quant(192);
        ok = ok && tstar_jpeg_encode_blocks_host(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, coef.data(), quant.data(), 1, nullptr) == 0;
        std::vector<uint8_t> scan(L - kJpegEncHeaderBytes), head(kJpegEncHeaderBytes);
        size_t hl = 0;
        ok = ok && tstar_jpeg_encode_scan_host(coef.data(), 1, W, H, hs, vs, scan.data(), scan.size(), len, st, 1, nullptr) == 0 &&
             st[0] == JPEG_ENC_OK && len[0] == scan.size() && memcmp(scan.data(), full.data() + kJpegEncHeaderBytes, scan.size()) == 0;
        ok = ok && tstar_jpeg_encode_header(W, H, quality, hs, vs, head.data(), head.size(), &hl) == 0 && hl == head.size() &&
             memcmp(head.data(), full.data(), hl) == 0;
        ok = ok && tstar_jpeg_encode_header(W, H, quality, hs, vs, none.data(), 0, &hl) != 0 && none[0] == 0xA5;
        std::vector<uint8_t> scan_short(scan.size() - 1, 0xA5);
        ok = ok && tstar_jpeg_encode_scan_host(coef.data(), 1, W, H, hs, vs, scan_short.data(), scan_short.size(), len, st, 1, nullptr) == 0 &&
             st[0] == JPEG_ENC_SHORT;
        for (uint8_t b : scan_short) ok = ok && b == 0xA5;
        printf("%s %dx%d q%d %dx%d ok=%d bytes=%zu zrl=%llu no_eob=%llu stuffed=%llu\n", argv[a], W, H, quality, hs, vs, ok, L,
               (unsigned long long)counters[JPEG_ENC_N_ZRL], (unsigned long long)counters[JPEG_ENC_N_NO_EOB],
               (unsigned long long)counters[JPEG_ENC_N_STUFFED]);
        if (!ok) bad = 1;
    }
    return bad;
}
