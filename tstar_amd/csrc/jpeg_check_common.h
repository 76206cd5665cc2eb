// What the stand-alone checkers of the device entropy core (jpeg_segments_check_main.cpp, jpeg_split_check_main.cpp) share:
// read a file, find the start of its entropy data, plan one frame on exact-size heap copies.
#pragma once
#include "jpeg_entropy_core.h"
#include "jpeg_host.h"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace jpegcheck {

using namespace tstar;

inline bool read_file(const char* path, std::vector<uint8_t>* d) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); return false; }
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) d->insert(d->end(), buf, buf + got);
    fclose(f);
    return true;
}

// start of the entropy data: after the first SOS segment (0: none)
inline size_t entropy_start(const std::vector<uint8_t>& d) {
    for (size_t p = 2; p + 4 <= d.size();) {
        if (d[p] != 0xFF) break;
        const int m = d[p + 1];
        const size_t L = ((size_t)d[p + 2] << 8) | d[p + 3];
        if (m == 0xDA) return p + 2 + L;
        p += 2 + L;
    }
    return 0;
}

// One stream as a batch of one frame.  Every buffer is an exact-size heap block, so a read or write one element outside is
// seen by AddressSanitizer.
struct OneFrame {
    std::vector<uint8_t> bytes;
    std::vector<uint16_t> quant;
    std::vector<JpegSegment> segs;
    std::vector<JpegTableSet> sets;
    JpegFrameDesc frame;
    int32_t route;                                                  // 0: the device route
};

inline bool plan_one_frame(const uint8_t* d, size_t n, const JpegGeom& g, OneFrame* f) {
    f->bytes.assign(d, d + n);
    f->quant.assign(192, 0);
    f->route = -1;
    const uint8_t* datas[1] = {f->bytes.data()};
    const size_t lens[1] = {n};
    const uint64_t offsets[1] = {0};
    std::vector<JpegTableSet> sets;
    std::vector<JpegSegment> segs;
    if (!jpeg_plan_segments(datas, lens, offsets, 1, g, &f->route, &f->frame, f->quant.data(), &sets, &segs)) return false;
    f->segs.assign(segs.begin(), segs.end());                       // exact-size blocks of the records too
    f->sets.assign(sets.begin(), sets.end());
    return true;
}

}  // namespace jpegcheck
