// Stand-alone checker of the JPEG encoder's host twin WITH OPTIMISED HUFFMAN TABLES for sanitizer builds (host only), the
// companion of jpeg_enc_check_main.cpp and jpeg_enc_rst_check_main.cpp and built the same way:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread
//       jpeg_enc_host.cpp jpeg_host.cpp jpeg_enc_opt_check_main.cpp -o jpeg_enc_opt_check
//   jpeg_enc_opt_check
//
// It needs no input: tiny geometries (one MCU, one pixel, dummy blocks right and below, every sampling) times intervals from none to
// beyond the frame, on frames of a fixed pseudo-random sequence at quality 100, and a flat mid-gray frame (four one-symbol tables).  Every
// frame, coefficient array, spec, histogram and output lives in a heap block of EXACT size, so that AddressSanitizer sees a read or
// write one byte outside.  Each case runs the whole-file entry at a generous capacity, the exact one (must succeed), one byte less
// (must report a short slot and write nothing), zero, and two frames on two workers; the scan stage and the header entry alone at
// exact and short capacities; and checks what must hold whatever the picture: four DHT segments that count their symbols, the
// scan stage's bytes behind the header entry's bytes are the whole-file entry's, the histograms sum to the symbols of the tables.
// The last line runs the table procedure on the extreme histograms: one symbol, all 256, equal counts, 1, 2, 3, 5, ... for 18, 30
// and 32 symbols (code sizes above 16: the limiting loop) and for 33 and 40 (code sizes above 32: the overflow status).
// Prints one line per case; exit status 1 when a result is not what it must be.
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

namespace {

struct Case { int W, H, hs, vs, flat; };

bool all_are(const std::vector<uint8_t>& v, uint8_t b) {
    for (uint8_t x : v)
        if (x != b) return false;
    return true;
}

// the four DHT segments behind the 177 bytes in front of them: each counts its symbols; -> the offset behind the last, 0 when not
size_t walk_dhts(const std::vector<uint8_t>& f, size_t* symbols) {
    size_t p = kJpegEncHeaderDhtAt;
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    *symbols = 0;
    for (int t = 0; t < 4; ++t) {
        if (p + 21 > f.size() || f[p] != 0xFF || f[p + 1] != 0xC4 || f[p + 4] != ids[t]) return 0;
        const size_t len = (size_t)f[p + 2] << 8 | f[p + 3];
        size_t n = 0;
        for (int i = 0; i < 16; ++i) n += f[p + 5 + i];
        if (len != 19 + n || n < 1) return 0;
        *symbols += n;
        p += 2 + len;
    }
    return p;
}

// the table procedure on one histogram, everything in exact-size heap blocks
bool table_case(const std::vector<uint32_t>& freq, int want_status, bool want_steps) {
    std::vector<uint8_t> spec(kJpegEncSpecBytes), len(256);
    std::vector<uint16_t> code(256);
    std::vector<int32_t> steps(1, -1);
    if (tstar_jpeg_huff_optimal(freq.data(), spec.data(), code.data(), len.data(), steps.data()) != 0) return false;
    jpegenc::HuffSpecWide s;
    memcpy(&s, spec.data(), sizeof(s));
    if (s.status != want_status) return false;
    size_t present = 0, coded = 0, sum = 0;
    for (int i = 0; i < 256; ++i) { present += freq[i] != 0; coded += len[i] != 0; }
    for (int i = 0; i < 16; ++i) sum += s.bits[i];
    if (want_status != jpegenc::HUFF_OK) return s.nvals == 0 && sum == 0 && coded == 0;
    for (int i = 0; i < 256; ++i)
        if ((freq[i] != 0) != (len[i] != 0) || len[i] > 16) return false;
    return s.nvals == present && sum == present && coded == present && (steps[0] > 0) == want_steps;
}

}  // namespace

int main() {
    const Case cases[] = {{8, 8, 2, 2, 0}, {1, 1, 1, 1, 0}, {40, 24, 2, 2, 0}, {77, 9, 2, 2, 0}, {9, 45, 2, 1, 0}, {33, 31, 2, 1, 1}, {40, 24, 1, 1, 0},
                          {23, 17, 1, 1, 1}};
    const int intervals[] = {0, 1, 3, 65535};
    const int quality = 100;
    int bad = 0;
    uint32_t seed = 12345u;
    for (const Case& cs : cases) {
        const int W = cs.W, H = cs.H, hs = cs.hs, vs = cs.vs;
        const JpegGeom g{W, H, 3, hs, vs};
        std::vector<uint8_t> frame((size_t)W * H * 3);
        for (uint8_t& b : frame) { seed = seed * 1664525u + 1013904223u; b = cs.flat ? 128 : (uint8_t)(seed >> 24); }
        const int32_t idx1[1] = {0}, idx2[2] = {0, 0};
        for (int R : intervals) {
            uint32_t len[2] = {0, 0};
            int32_t st[2] = {-1, -1};
            std::vector<uint8_t> full((size_t)jpeg_enc_header_bytes(R, 1) + jpeg_enc_max_scan_bytes(g, R, 1));
            int ok = tstar_jpeg_encode_host_opt(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, R, full.data(), full.size(), len, st, 1, nullptr,
                                                nullptr) == 0 &&
                     st[0] == JPEG_ENC_OK && len[0] > (uint32_t)kJpegEncHeaderDhtAt;
            const size_t L = len[0];
            full.resize(L);
            size_t symbols = 0;
            const size_t dht_end = walk_dhts(full, &symbols);
            const size_t head = dht_end + (R > 0 ? 6 : 0) + 14;
            ok = ok && dht_end != 0 && head < L && full[head - 14] == 0xFF && full[head - 13] == 0xDA;
            if (cs.flat) ok = ok && symbols == 4 && dht_end == (size_t)kJpegEncHeaderDhtAt + 4 * 22;
            // exact capacity, one byte short, zero
            std::vector<uint8_t> exact(L), shorter(L - 1, 0xA5), none(1, 0xA5);
            ok = ok && tstar_jpeg_encode_host_opt(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, R, exact.data(), L, len, st, 1, nullptr, nullptr) == 0 &&
                 st[0] == JPEG_ENC_OK && len[0] == L && exact == full;
            ok = ok && tstar_jpeg_encode_host_opt(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, R, shorter.data(), L - 1, len, st, 1, nullptr,
                                                  nullptr) == 0 &&
                 st[0] == JPEG_ENC_SHORT && len[0] == L && all_are(shorter, 0xA5);
            ok = ok && tstar_jpeg_encode_host_opt(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, R, none.data(), 0, len, st, 1, nullptr, nullptr) == 0 &&
                 st[0] == JPEG_ENC_SHORT && none[0] == 0xA5;
            // two frames on two workers, slots back to back
            std::vector<uint8_t> two(2 * L);
            ok = ok && tstar_jpeg_encode_host_opt(frame.data(), 1, H, W, idx2, 2, quality, hs, vs, R, two.data(), L, len, st, 2, nullptr, nullptr) == 0 &&
                 st[0] == JPEG_ENC_OK && st[1] == JPEG_ENC_OK && memcmp(two.data(), full.data(), L) == 0 && memcmp(two.data() + L, full.data(), L) == 0;
            // the stages separately: exact-size coefficients, scan, specs, histogram, header; then under-sized ones
            std::vector<int16_t> coef(g.blocks() * 64);
            ok = ok && tstar_jpeg_encode_blocks_host(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, coef.data(), nullptr, 1, nullptr) == 0;
            std::vector<uint8_t> scan(L - head), specs(4 * kJpegEncSpecBytes), hd(head);
            std::vector<uint32_t> hist(4 * jpegenc::kHuffSymbols);
            size_t hl = 0;
            ok = ok && tstar_jpeg_encode_scan_host_opt(coef.data(), 1, W, H, hs, vs, R, scan.data(), scan.size(), len, st, specs.data(), hist.data(), 1,
                                                       nullptr, nullptr) == 0 &&
                 st[0] == JPEG_ENC_OK && len[0] == scan.size() && memcmp(scan.data(), full.data() + head, scan.size()) == 0;
            size_t present = 0, dc = 0;
            for (int t = 0; t < 4; ++t)
                for (int i = 0; i < jpegenc::kHuffSymbols; ++i) {
                    present += hist[t * jpegenc::kHuffSymbols + i] != 0;
                    if (t % 2 == 0) dc += hist[t * jpegenc::kHuffSymbols + i];
                }
            ok = ok && present == symbols && dc == g.blocks();                  // one DC symbol per block, dummy blocks included
            ok = ok && tstar_jpeg_encode_header_opt(W, H, quality, hs, vs, R, specs.data(), hd.data(), hd.size(), &hl) == 0 && hl == head &&
                 memcmp(hd.data(), full.data(), hl) == 0;
            std::vector<uint8_t> hd_short(head - 1, 0xA5);
            ok = ok && tstar_jpeg_encode_header_opt(W, H, quality, hs, vs, R, specs.data(), hd_short.data(), hd_short.size(), &hl) == 4 &&
                 all_are(hd_short, 0xA5);
            for (size_t cut : {(size_t)1, scan.size() / 2, scan.size()}) {
                std::vector<uint8_t> scan_short(scan.size() - cut, 0xA5);
                ok = ok && tstar_jpeg_encode_scan_host_opt(coef.data(), 1, W, H, hs, vs, R, scan_short.data(), scan_short.size(), len, st, specs.data(),
                                                           nullptr, 1, nullptr, nullptr) == 0 &&
                     st[0] == JPEG_ENC_SHORT && len[0] == scan.size() && all_are(scan_short, 0xA5);
            }
            printf("%dx%d %dx%d flat=%d interval=%d bytes=%zu header=%zu symbols=%zu ok=%d\n", W, H, hs, vs, cs.flat, R, L, head, symbols, ok);
            if (!ok) bad = 1;
        }
    }
    // the table procedure alone
    int ok = 1;
    std::vector<uint32_t> f(256, 0);
    f[0xF0] = 7;
    ok = ok && table_case(f, jpegenc::HUFF_OK, false);                         // one symbol
    for (int i = 0; i < 256; ++i) f[i] = 3;
    ok = ok && table_case(f, jpegenc::HUFF_OK, false);                         // all 256, every choice a tie
    for (int i = 0; i < 256; ++i) f[i] = (uint32_t)(i * 2654435761u >> 12) % 1000u + 1000u;          // all 256, no two alike in a row
    ok = ok && table_case(f, jpegenc::HUFF_OK, false);
    for (int n : {18, 30, 32, 33, 40}) {
        std::vector<uint32_t> fib(256, 0);
        uint64_t a = 1, b = 2;
        for (int i = 0; i < n; ++i) {
            fib[i] = (uint32_t)a;                      // 40 of them sum to 433 494 434
            const uint64_t c = a + b;
            a = b;
            b = c;
        }
        ok = ok && table_case(fib, n >= 33 ? jpegenc::HUFF_CLEN_OVERFLOW : jpegenc::HUFF_OK, n < 33);
    }
    std::vector<uint32_t> none(256, 0), big(256, 10000000u);
    ok = ok && table_case(none, jpegenc::HUFF_EMPTY, false);
    std::vector<uint8_t> spec(kJpegEncSpecBytes);
    ok = ok && tstar_jpeg_huff_optimal(big.data(), spec.data(), nullptr, nullptr, nullptr) != 0;
    printf("tables ok=%d\n", ok);
    return bad || !ok;
}
