// Stand-alone checker of the JPEG encoder's host twin WITH RESTART INTERVALS for sanitizer builds (host only), the companion of
// jpeg_enc_check_main.cpp and built the same way:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread
//       jpeg_enc_host.cpp jpeg_host.cpp jpeg_enc_rst_check_main.cpp -o jpeg_enc_rst_check
//   jpeg_enc_rst_check
//
// It needs no input: tiny geometries (one MCU, one MCU row, one MCU column, dummy blocks right and below, every sampling) times
// intervals from 1 MCU to beyond the frame, on frames of a fixed pseudo-random sequence at quality 100 (long scans, 0xFF bytes).
// Every frame, coefficient array and output lives in a heap block of EXACT size, so that AddressSanitizer sees a read or write
// one byte outside.  Each case runs the whole-file entry at a generous capacity, the exact one (must succeed), one byte less
// (must report a short slot and write nothing), zero, and two frames on two workers; the scan stage and the header alone at
// exact and short capacities; and checks what the bytes must hold whatever the picture: DRI in front of SOS, as many RSTn as
// the geometry says, numbered 0..7 in turn, as many as the counter says.  Prints one line per case; exit status 1 when a
// result is not what it must be.
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

struct Case { int W, H, hs, vs; };

bool all_are(const std::vector<uint8_t>& v, uint8_t b) {
    for (uint8_t x : v)
        if (x != b) return false;
    return true;
}

// markers of a scan (stuffed bytes: FF D0..D7 can only be a marker); -1 when they are not numbered 0..7 in turn
long count_markers(const uint8_t* scan, size_t len) {
    long n = 0;
    for (size_t i = 0; i + 1 < len; ++i)
        if (scan[i] == 0xFF && scan[i + 1] >= 0xD0 && scan[i + 1] <= 0xD7) {
            if (scan[i + 1] != 0xD0 + (n & 7)) return -1;
            ++n;
        }
    return n;
}

}  // namespace

int main() {
    const Case cases[] = {{8, 8, 2, 2}, {1, 1, 1, 1}, {40, 24, 2, 2}, {77, 9, 2, 2}, {9, 45, 2, 1}, {33, 31, 2, 1}, {40, 24, 1, 1}, {23, 17, 1, 1}};
    const int intervals[] = {0, 1, 2, 3, 5, 7, 64, 65535};
    const int quality = 100;
    int bad = 0;
    uint32_t seed = 12345u;
    for (const Case& cs : cases) {
        const int W = cs.W, H = cs.H, hs = cs.hs, vs = cs.vs;
        const JpegGeom g{W, H, 3, hs, vs};
        std::vector<uint8_t> frame((size_t)W * H * 3);
        for (uint8_t& b : frame) { seed = seed * 1664525u + 1013904223u; b = (uint8_t)(seed >> 24); }
        const int32_t idx1[1] = {0}, idx2[2] = {0, 0};
        std::vector<uint8_t> plain;                   // the file without an interval, from the entry that takes none
        for (int R : intervals) {
            uint32_t len[2] = {0, 0};
            int32_t st[2] = {-1, -1};
            uint64_t rc[JPEG_ENC_R_COUNTERS] = {0, 0, 0};
            const size_t head = (size_t)jpeg_enc_header_bytes(R);
            const size_t markers = jpeg_enc_restart_markers(g, R);
            std::vector<uint8_t> full(head + jpeg_enc_max_scan_bytes(g, R));
            int ok = tstar_jpeg_encode_host_rst(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, R, full.data(), full.size(), len, st, 1, nullptr,
                                                rc) == 0 &&
                     st[0] == JPEG_ENC_OK && len[0] > head;
            const size_t L = len[0];
            ok = ok && rc[JPEG_ENC_R_RST] == markers && count_markers(full.data() + head, L - head) == (long)markers;
            ok = ok && rc[JPEG_ENC_R_PAD_FREE] <= markers && rc[JPEG_ENC_R_PAD_FF] <= markers - rc[JPEG_ENC_R_PAD_FREE];
            if (R > 0) {
                const uint8_t dri[6] = {0xFF, 0xDD, 0, 4, (uint8_t)(R >> 8), (uint8_t)(R & 255)};
                ok = ok && head == (size_t)kJpegEncHeaderBytes + 6 && memcmp(full.data() + head - 14 - 6, dri, 6) == 0 &&
                     full[head - 14] == 0xFF && full[head - 13] == 0xDA;
            } else {
                plain.assign(L, 0);
                ok = ok && tstar_jpeg_encode_host(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, plain.data(), L, len, st, 1, nullptr) == 0 &&
                     st[0] == JPEG_ENC_OK && len[0] == L && memcmp(plain.data(), full.data(), L) == 0;
            }
            if (R > 0 && markers == 0)                 // DRI and no marker: the plain file with six bytes more
                ok = ok && L == plain.size() + 6 && memcmp(full.data() + head, plain.data() + kJpegEncHeaderBytes, L - head) == 0;
            // exact capacity
            std::vector<uint8_t> exact(L);
            ok = ok && tstar_jpeg_encode_host_rst(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, R, exact.data(), L, len, st, 1, nullptr,
                                                  nullptr) == 0 &&
                 st[0] == JPEG_ENC_OK && len[0] == L && memcmp(exact.data(), full.data(), L) == 0;
            // one byte short, and zero capacity: a status, the length it would have taken, not a byte written
            std::vector<uint8_t> shorter(L - 1, 0xA5), none(1, 0xA5);
            ok = ok && tstar_jpeg_encode_host_rst(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, R, shorter.data(), L - 1, len, st, 1, nullptr,
                                                  nullptr) == 0 &&
                 st[0] == JPEG_ENC_SHORT && len[0] == L && all_are(shorter, 0xA5);
            ok = ok && tstar_jpeg_encode_host_rst(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, R, none.data(), 0, len, st, 1, nullptr,
                                                  nullptr) == 0 &&
                 st[0] == JPEG_ENC_SHORT && none[0] == 0xA5;
            // two frames on two workers, slots back to back; the counters of both are summed
            std::vector<uint8_t> two(2 * L);
            uint64_t rc2[JPEG_ENC_R_COUNTERS] = {0, 0, 0};
            ok = ok && tstar_jpeg_encode_host_rst(frame.data(), 1, H, W, idx2, 2, quality, hs, vs, R, two.data(), L, len, st, 2, nullptr, rc2) == 0 &&
                 st[0] == JPEG_ENC_OK && st[1] == JPEG_ENC_OK && memcmp(two.data(), full.data(), L) == 0 &&
                 memcmp(two.data() + L, full.data(), L) == 0;
            for (int k = 0; k < JPEG_ENC_R_COUNTERS; ++k) ok = ok && rc2[k] == 2 * rc[k];
            // the stages separately: exact-size coefficients, exact-size scan, exact-size header; then under-sized ones
            std::vector<int16_t> coef(g.blocks() * 64);
            ok = ok && tstar_jpeg_encode_blocks_host(frame.data(), 1, H, W, idx1, 1, quality, hs, vs, coef.data(), nullptr, 1, nullptr) == 0;
            std::vector<uint8_t> scan(L - head), hd(head);
            size_t hl = 0;
            uint64_t rc3[JPEG_ENC_R_COUNTERS] = {0, 0, 0};
            ok = ok && tstar_jpeg_encode_scan_host_rst(coef.data(), 1, W, H, hs, vs, R, scan.data(), scan.size(), len, st, 1, nullptr, rc3) == 0 &&
                 st[0] == JPEG_ENC_OK && len[0] == scan.size() && memcmp(scan.data(), full.data() + head, scan.size()) == 0;
            for (int k = 0; k < JPEG_ENC_R_COUNTERS; ++k) ok = ok && rc3[k] == rc[k];
            ok = ok && tstar_jpeg_encode_header_rst(W, H, quality, hs, vs, R, hd.data(), hd.size(), &hl) == 0 && hl == head &&
                 memcmp(hd.data(), full.data(), hl) == 0;
            std::vector<uint8_t> hd_short(head - 1, 0xA5);
            ok = ok && tstar_jpeg_encode_header_rst(W, H, quality, hs, vs, R, hd_short.data(), hd_short.size(), &hl) != 0 && all_are(hd_short, 0xA5);
            for (size_t cut : {(size_t)1, (size_t)2, scan.size() / 2, scan.size()}) {
                if (cut > scan.size()) continue;
                std::vector<uint8_t> scan_short(scan.size() - cut, 0xA5);
                ok = ok && tstar_jpeg_encode_scan_host_rst(coef.data(), 1, W, H, hs, vs, R, scan_short.data(), scan_short.size(), len, st, 1,
                                                           nullptr, nullptr) == 0 &&
                     st[0] == JPEG_ENC_SHORT && len[0] == scan.size() && all_are(scan_short, 0xA5);
            }
            // an interval the DRI segment cannot hold is refused
            ok = ok && tstar_jpeg_encode_scan_host_rst(coef.data(), 1, W, H, hs, vs, 65536, scan.data(), scan.size(), len, st, 1, nullptr, nullptr) != 0;
            ok = ok && tstar_jpeg_encode_scan_host_rst(coef.data(), 1, W, H, hs, vs, -1, scan.data(), scan.size(), len, st, 1, nullptr, nullptr) != 0;
            printf("%dx%d %dx%d interval=%d ok=%d bytes=%zu rst=%llu pad_free=%llu pad_ff=%llu\n", W, H, hs, vs, R, ok, L,
                   (unsigned long long)rc[JPEG_ENC_R_RST], (unsigned long long)rc[JPEG_ENC_R_PAD_FREE], (unsigned long long)rc[JPEG_ENC_R_PAD_FF]);
            if (!ok) bad = 1;
        }
    }
    return bad;
}
