// Stand-alone checker of the segment planner and of the device kernel's decode core on the CPU, for sanitizer builds
// (host only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread jpeg_host.cpp jpeg_segments_check_main.cpp -o jpeg_segments_check
//   jpeg_segments_check FILE.jpg ...
//
// For every file, with the intact file's geometry as the batch's: the intact bytes, the file truncated at every 97th
// offset, single flipped bytes in the entropy data, every header byte overwritten in three ways, stray bytes in front of
// EOI and a missing EOI go through jpeg_plan_segments + jpeg_entropy_segments_host and through jpeg_entropy.  Every buffer
// is an exact-size heap block, so a read or write one element outside is seen by AddressSanitizer.  Required of every
// stream: a frame jpeg_entropy accepts takes the device route; a device-routed frame's status (its first segment that is
// not OK) equals jpeg_entropy's; when that is OK, coefficients and quantisation rows are identical.  Prints one line per
// file; exit status 1 on any difference or when the intact file does not decode on the device route.
#include "jpeg_check_common.h"

namespace tstar {
void set_error(const std::string&) {}
}  // namespace tstar

using namespace jpegcheck;

struct Tally {
    int streams = 0, device_routed = 0, device_ok = 0, differ = 0;
};

// one stream, exact-size copies -> false when the two decoders disagree
static bool run(const uint8_t* d, size_t n, const JpegGeom& g, Tally& t, int* device_status) {
    OneFrame f;
    ++t.streams;
    *device_status = -1;
    if (!plan_one_frame(d, n, g, &f)) return false;
    const size_t per = g.blocks() * 64;
    std::vector<int16_t> want(per), got(per);
    std::vector<uint16_t> want_q(192);
    char msg[160];
    const int host = jpeg_entropy(f.bytes.data(), n, g, want.data(), want_q.data(), msg, sizeof(msg));
    if (f.route != 0) return host != JPEG_OK;                       // what the sequential decoder accepts is planned
    ++t.device_routed;
    std::vector<int32_t> status(f.segs.size(), -1);
    if (f.segs.empty() || f.frame.n_segments != (int32_t)f.segs.size() || f.frame.table_set != 0 || f.sets.size() != 1) return false;
    if (!jpeg_entropy_segments_host(f.bytes.data(), n, f.segs.data(), f.sets.data(), 1, &f.frame, 1, (int)f.segs.size(), g, got.data(),
                                    status.data()))
        return false;
    int dev = JPEG_OK;
    for (size_t i = 0; i < status.size() && dev == JPEG_OK; ++i) dev = status[i];
    *device_status = dev;
    if (dev != host) return false;
    if (dev == JPEG_OK) {
        ++t.device_ok;
        if (memcmp(want.data(), got.data(), per * sizeof(int16_t)) != 0 || memcmp(want_q.data(), f.quant.data(), 192 * sizeof(uint16_t)) != 0)
            return false;
    }
    return true;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::vector<uint8_t> d;
        if (!read_file(argv[a], &d)) return 2;
        char msg[160];
        JpegGeom g;
        if (jpeg_probe(d.data(), d.size(), &g, msg, sizeof(msg)) != JPEG_OK) { fprintf(stderr, "%s: %s\n", argv[a], msg); return 2; }
        Tally t;
        int st = -1;
        auto check = [&](const uint8_t* p, size_t n, const char* what, size_t at) {
            if (!run(p, n, g, t, &st)) {
                ++t.differ;
                fprintf(stderr, "%s: %s at %zu: planner / segment decoder and the sequential decoder disagree\n", argv[a], what, at);
            }
        };
        check(d.data(), d.size(), "intact", 0);
        const int intact = st;
        const size_t sos = entropy_start(d);
        for (size_t n = 0; n < d.size(); n += 97) check(d.data(), n, "truncation", n);
        if (sos && sos + 2 < d.size()) {
            const size_t span = d.size() - 2 - sos, step = span / 64 + 1;
            std::vector<uint8_t> m(d);
            for (size_t p = sos; p < d.size() - 2; p += step) {
                m[p] ^= 0xFF;
                check(m.data(), m.size(), "flip", p);
                m[p] ^= 0xFF;
            }
            const uint8_t over[3] = {0x00, 0xFF, 0x80};
            for (size_t p = 2; p < sos; ++p)
                for (int k = 0; k < 3; ++k) {
                    const uint8_t keep = m[p];
                    m[p] = k == 2 ? (uint8_t)(keep ^ 0x80) : over[k];
                    check(m.data(), m.size(), "header byte", p);
                    m[p] = keep;
                }
            std::vector<uint8_t> stray(d.begin(), d.end() - 2);     // bytes between the last block and EOI
            const uint8_t extra[5] = {0x12, 0x34, 0x56, 0xFF, 0xD9};
            stray.insert(stray.end(), extra, extra + 5);
            check(stray.data(), stray.size(), "stray bytes", d.size() - 2);
            check(d.data(), d.size() - 2, "missing EOI", d.size() - 2);
            check(d.data(), d.size() - 1, "half an EOI", d.size() - 1);
        }
        printf("%s intact=%d streams=%d device_routed=%d device_ok=%d differ=%d\n", argv[a], intact, t.streams, t.device_routed,
               t.device_ok, t.differ);
        if (intact != JPEG_OK || t.differ) bad = 1;
    }
    return bad;
}
