// Stand-alone checker of the split entropy path (jpeg_entropy_split_host: sub-sequences, rounds, scan, write pass, redo)
// on the CPU, for sanitizer builds (host only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread jpeg_host.cpp jpeg_split_check_main.cpp -o jpeg_split_check
//   jpeg_split_check [--exhaustive N] FILE.jpg ...
//
// Every stream goes through jpeg_plan_segments + jpeg_entropy_split_host with sub-sequences of 8, 64 and 128 bytes, every
// segment cut (min_split_bytes = 1), and through jpeg_entropy.  Every buffer, the workspace included, is an exact-size heap
// block.  Required of every device-routed stream: its status equals jpeg_entropy's (so OK <=> OK, and never the UNCOVERED
// that stands for "the write pass refused what one lane accepts"); when that is OK, the coefficients are identical; and
// with max_rounds = 1 (segments abandoned) the result is the same.  The intact file must converge.  Streams: the intact
// file, truncations and flipped bytes spread over the file (of a file above 8 KB only 24 of each, and these without the
// 8-byte sub-sequences, whose thousands of rounds are the intact file's to walk); for the first N files (--exhaustive,
// default 2; meant for small files) EVERY truncation and every single byte of the entropy data corrupted in three ways.
// Prints one line per file; exit status 1 on any difference.
#include "jpeg_check_common.h"

#include <stdlib.h>

namespace tstar {
void set_error(const std::string&) {}
}  // namespace tstar

using namespace jpegcheck;

struct Tally {
    int streams = 0, routed = 0, ok = 0, differ = 0, split = 0, abandoned = 0, rounds_max = 0;
};

static const int kSubs[3] = {8, 64, 128};

// one stream -> false when the split path and the sequential decoder disagree
static bool run(const uint8_t* d, size_t n, const JpegGeom& g, Tally& t, bool must_converge, bool smallest = true) {
    OneFrame f;
    ++t.streams;
    if (!plan_one_frame(d, n, g, &f)) return false;
    const size_t per = g.blocks() * 64;
    std::vector<int16_t> want(per), got(per);
    std::vector<uint16_t> want_q(192);
    char msg[160];
    const int host = jpeg_entropy(f.bytes.data(), n, g, want.data(), want_q.data(), msg, sizeof(msg));
    if (f.route != 0) return host != JPEG_OK;
    ++t.routed;
    const std::vector<JpegSegment>& segs = f.segs;
    const int nseg = (int)segs.size();
    if (nseg == 0 || f.sets.size() != 1) return false;
    bool good = true;
    for (int v = smallest ? 0 : 1; v < 4; ++v) {                    // three sub-sequence sizes, then one round only
        const int sub = kSubs[v % 3], rounds = v == 3 ? 1 : kJpegSplitMaxRounds;
        const size_t wsb = jpeg_split_workspace_bytes(n, nseg, sub);
        if (wsb == 0) return false;
        std::vector<uint64_t> ws((wsb + 7) / 8);
        std::vector<int32_t> status((size_t)nseg, -1), info((size_t)nseg, -7);
        if (!jpeg_entropy_split_host(f.bytes.data(), n, segs.data(), f.sets.data(), 1, &f.frame, 1, nseg, g, sub, 1, rounds, ws.data(), wsb,
                                     got.data(), status.data(), info.data()))
            return false;
        int dev = JPEG_OK;
        for (int i = 0; i < nseg && dev == JPEG_OK; ++i) dev = status[(size_t)i];
        for (int i = 0; i < nseg; ++i) {
            const int32_t r = info[(size_t)i];
            if (r == 0 && segs[(size_t)i].end > segs[(size_t)i].begin) good = false;    // min_split_bytes = 1 cuts every segment that has a byte
            if (r > 0) { ++t.split; if (r > t.rounds_max) t.rounds_max = r; }
            if (r < 0) ++t.abandoned;
            if (must_converge && v < 3 && r <= 0) good = false;
        }
        if (dev != host) good = false;
        if (dev == JPEG_OK && (memcmp(want.data(), got.data(), per * sizeof(int16_t)) != 0 ||
                               memcmp(want_q.data(), f.quant.data(), 192 * sizeof(uint16_t)) != 0))
            good = false;
        if (dev == JPEG_OK && v == 1) ++t.ok;
    }
    return good;
}

int main(int argc, char** argv) {
    int bad = 0, exhaustive = 2, a = 1;
    if (argc > 2 && strcmp(argv[1], "--exhaustive") == 0) { exhaustive = atoi(argv[2]); a = 3; }
    for (int fi = 0; a < argc; ++a, ++fi) {
        std::vector<uint8_t> d;
        if (!read_file(argv[a], &d)) return 2;
        char msg[160];
        JpegGeom g;
        if (jpeg_probe(d.data(), d.size(), &g, msg, sizeof(msg)) != JPEG_OK) { fprintf(stderr, "%s: %s\n", argv[a], msg); return 2; }
        Tally t;
        auto check = [&](const uint8_t* p, size_t n, const char* what, size_t at, bool conv) {
            if (!run(p, n, g, t, conv, conv || d.size() <= 8192)) {
                ++t.differ;
                fprintf(stderr, "%s: %s at %zu: the split path and the sequential decoder disagree\n", argv[a], what, at);
            }
        };
        check(d.data(), d.size(), "intact", 0, true);
        const bool intact = t.ok == 1 && t.differ == 0;
        const size_t sos = entropy_start(d);
        const bool all = fi < exhaustive;
        const bool big = d.size() > 8192;
        for (size_t n = all ? sos : 0; n < d.size(); n += all ? 1 : (big ? d.size() / 24 : 97)) check(d.data(), n, "truncation", n, false);
        if (sos && sos + 2 < d.size()) {
            const size_t span = d.size() - 2 - sos, step = all ? 1 : span / (big ? 24 : 64) + 1;
            std::vector<uint8_t> m(d);
            for (size_t p = sos; p < d.size() - 2; p += step) {
                const uint8_t keep = m[p];
                const uint8_t with[3] = {(uint8_t)(keep ^ 0xFF), (uint8_t)(keep ^ 0x01), (uint8_t)(keep == 0xFF ? 0x7F : 0xFF)};
                for (int k = 0; k < (all ? 3 : 1); ++k) {
                    m[p] = with[k];
                    check(m.data(), m.size(), "corruption", p, false);
                }
                m[p] = keep;
            }
            std::vector<uint8_t> stray(d.begin(), d.end() - 2);
            const uint8_t extra[5] = {0x12, 0x34, 0x56, 0xFF, 0xD9};
            stray.insert(stray.end(), extra, extra + 5);
            check(stray.data(), stray.size(), "stray bytes", d.size() - 2, false);
        }
        printf("%s intact=%d streams=%d routed=%d ok=%d split=%d abandoned=%d rounds_max=%d differ=%d\n", argv[a], intact ? 0 : 1, t.streams,
               t.routed, t.ok, t.split, t.abandoned, t.rounds_max, t.differ);
        if (!intact || t.differ) bad = 1;
    }
    return bad;
}
