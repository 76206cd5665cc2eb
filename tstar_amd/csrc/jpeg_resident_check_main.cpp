// Stand-alone checker of the gather's host mirror (jpeg_resident_host.cpp), for sanitizer builds (host only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan jpeg_resident_host.cpp jpeg_resident_check_main.cpp -o jpeg_resident_check
//   jpeg_resident_check [SEED]
//
// Builds an arena of frames of lengths 0 .. a few thousand bytes at every misalignment, with segment records inside them, in
// exact-size heap blocks (so a read or write one byte outside is seen by AddressSanitizer), and drives the C entries over
//   good     descriptors of shuffled id lists with repeats and zero-length frames: the batch must equal a plain restatement;
//   refused  out-of-range ids, frames that overlap, leave gaps or start unaligned, a wrong segment prefix, total_bytes that is
//            no multiple of 16 or 2^32, batch capacities one byte short down to zero: the entry must return an error and leave
//            the batch buffer as it was;
//   zeroed   descriptors that pass those checks but disagree with the arena (another length, another segment count), and arenas
//            whose own records point outside them (offset + length beyond the arena, segments beyond the list, negative counts):
//            such a frame must come out as zeros with a record without a table set, everything else as in a good batch.
// Prints one line; exit status 1 on any difference.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/tstar_hip.h"
#include "jpeg_resident_core.h"

namespace tstar {
void set_error(const std::string&) {}
}  // namespace tstar

using namespace tstar;
using namespace tstar::jpegres;

namespace {

uint32_t g_state = 1;
uint32_t rnd() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}

struct TestArena {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<uint16_t> quant;          // call() hands it over in a 16-byte-aligned block
    std::vector<JpegFrameDesc> frames;
    std::vector<JpegSegment> segments;
};

TestArena make_arena() {
    TestArena a;
    const uint32_t lens[] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 1000, 4097, 0, 5};
    uint32_t e = 0;
    for (uint32_t L : lens) {
        a.bytes.resize(a.bytes.size() + (rnd() % 3), 0xEE);         // frames start at every misalignment over the list
        a.off.push_back(a.bytes.size());
        a.len.push_back(L);
        for (uint32_t i = 0; i < L; ++i) a.bytes.push_back((uint8_t)rnd());
        for (int i = 0; i < 192; ++i) a.quant.push_back((uint16_t)(e * 192 + i + 1));
        const int ns = L == 0 ? 0 : 1 + (int)(rnd() % 3);
        a.frames.push_back(JpegFrameDesc{(int32_t)(e % 3), (int32_t)a.segments.size(), ns, 0});
        for (int s = 0; s < ns; ++s) {
            const uint32_t b = L * s / ns, en = L * (s + 1) / ns;
            a.segments.push_back(JpegSegment{e, b, en, (uint32_t)s * 7, 7, s == ns - 1 ? 1u : 0u});
        }
        ++e;
    }
    return a;
}

struct Fetch {
    std::vector<GatherDesc> desc;
    size_t total = 0;
    int n_segments = 0;
};

Fetch describe(const TestArena& a, const std::vector<uint32_t>& ids) {
    Fetch f;
    for (uint32_t id : ids) {
        GatherDesc d{id, (uint32_t)f.total, a.len[id], (uint32_t)f.n_segments, (uint32_t)a.frames[id].n_segments, 0};
        f.desc.push_back(d);
        f.total += (a.len[id] + 15) & ~15u;
        f.n_segments += a.frames[id].n_segments;
    }
    return f;
}

// the batch a fetch must give; zero[j]: frame j is one the mirror has to refuse
std::vector<uint8_t> expect(const TestArena& a, const Fetch& f, const std::vector<bool>& zero) {
    size_t at3[3];
    const size_t nbytes = tstar_jpeg_gather_bytes(f.total, (int)f.desc.size(), f.n_segments, at3);
    std::vector<uint8_t> out(nbytes, 0);
    for (size_t j = 0; j < f.desc.size(); ++j) {
        const GatherDesc& d = f.desc[j];
        JpegFrameDesc fr{-1, 0, 0, 0};
        if (!zero[j]) {
            memcpy(out.data() + d.dst, a.bytes.data() + a.off[d.id], d.len);
            memcpy(out.data() + at3[0] + j * 384, a.quant.data() + (size_t)d.id * 192, 384);
            fr = JpegFrameDesc{a.frames[d.id].table_set, (int32_t)d.first_segment, (int32_t)d.n_segments, 0};
        }
        memcpy(out.data() + at3[1] + j * sizeof(fr), &fr, sizeof(fr));
        for (uint32_t i = 0; i < d.n_segments; ++i) {
            JpegSegment s{0xffffffffu, 0, 0, 0, 0, 0};
            if (!zero[j]) {
                s = a.segments[(size_t)a.frames[d.id].first_segment + i];
                s.frame = (uint32_t)j; s.begin += d.dst; s.end += d.dst;
            }
            memcpy(out.data() + at3[2] + (size_t)(d.first_segment + i) * sizeof(s), &s, sizeof(s));
        }
    }
    return out;
}

// one call on exact-size copies of everything -> the entry's return value; *batch holds the buffer afterwards
int call(const TestArena& a, size_t arena_bytes, const Fetch& f, size_t total, int n_segments, size_t cap, std::vector<uint8_t>* batch) {
    std::vector<uint8_t> bytes(a.bytes);
    std::vector<uint64_t> off(a.off);
    std::vector<uint32_t> len(a.len);
    std::vector<JpegFrameDesc> frames(a.frames);
    std::vector<JpegSegment> segments(a.segments);
    std::vector<GatherDesc> desc(f.desc);
    // a 16-byte-aligned, exact-size batch block
    void* raw = nullptr;
    const size_t alloc = cap ? (cap + 15) & ~(size_t)15 : 16;
    if (posix_memalign(&raw, 16, alloc)) exit(2);
    uint8_t* b = (uint8_t*)raw;
    memset(b, 0xA5, alloc);
    void* qraw = nullptr;
    if (posix_memalign(&qraw, 16, a.quant.size() * 2)) exit(2);
    memcpy(qraw, a.quant.data(), a.quant.size() * 2);
    const int rc = tstar_jpeg_gather_host(bytes.data(), arena_bytes, off.data(), len.data(), (const uint16_t*)qraw, frames.data(),
                                          segments.data(), (int)len.size(), (int)segments.size(), desc.data(), (int)desc.size(), total,
                                          n_segments, b, cap);
    batch->assign(b, b + cap);
    free(raw);
    free(qraw);
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    g_state = argc > 1 ? (uint32_t)atoi(argv[1]) * 2654435761u + 1 : 1;
    const TestArena a = make_arena();
    const uint32_t E = (uint32_t)a.len.size();
    int cases = 0, refused = 0, zeroed = 0, differ = 0;
    std::vector<uint8_t> got;
    auto untouched = [&](const std::vector<uint8_t>& b) {
        for (uint8_t v : b)
            if (v != 0xA5) return false;
        return true;
    };

    // good
    for (int round = 0; round < 40; ++round) {
        std::vector<uint32_t> ids;
        const int n = 1 + (int)(rnd() % 12);
        for (int j = 0; j < n; ++j) ids.push_back(rnd() % E);
        if (round == 0) ids = {0, 14, 0};                            // zero-length frames only
        if (round == 1) { ids.clear(); for (uint32_t e = 0; e < E; ++e) ids.push_back(e); }
        const Fetch f = describe(a, ids);
        const size_t cap = tstar_jpeg_gather_bytes(f.total, (int)ids.size(), f.n_segments, nullptr);
        ++cases;
        const std::vector<uint8_t> want = expect(a, f, std::vector<bool>(ids.size(), false));
        if (call(a, a.bytes.size(), f, f.total, f.n_segments, cap, &got) != 0 || got != want) {
            ++differ;
            fprintf(stderr, "good fetch %d differs\n", round);
        }
    }

    // refused
    {
        const std::vector<uint32_t> ids = {3, 12, 5, 12, 0, 13};
        const Fetch f = describe(a, ids);
        const size_t cap = tstar_jpeg_gather_bytes(f.total, (int)ids.size(), f.n_segments, nullptr);
        auto must_refuse = [&](const Fetch& g, size_t total, int nseg, size_t c, const char* what) {
            ++cases;
            if (call(a, a.bytes.size(), g, total, nseg, c, &got) == 0 || !untouched(got)) {
                ++differ;
                fprintf(stderr, "not refused: %s\n", what);
            } else {
                ++refused;
            }
        };
        Fetch g = f; g.desc[2].id = E;               must_refuse(g, f.total, f.n_segments, cap, "id == n_entries");
        g = f; g.desc[0].id = 0xffffffffu;           must_refuse(g, f.total, f.n_segments, cap, "id 2^32 - 1");
        g = f; g.desc[1].dst -= 16;                  must_refuse(g, f.total, f.n_segments, cap, "overlapping frames");
        g = f; g.desc[1].dst += 16;                  must_refuse(g, f.total, f.n_segments, cap, "a gap");
        g = f; g.desc[1].dst += 1;                   must_refuse(g, f.total, f.n_segments, cap, "unaligned start");
        g = f; g.desc[3].first_segment += 1;         must_refuse(g, f.total, f.n_segments, cap, "segment prefix");
        g = f; g.desc[5].len += 4096;                must_refuse(g, f.total, f.n_segments, cap, "frames beyond total_bytes");
        g = f; g.desc[5].n_segments += 1;            must_refuse(g, f.total, f.n_segments, cap, "segments beyond n_segments");
        must_refuse(f, f.total + 16, f.n_segments, cap + 16, "total_bytes larger than the frames");
        must_refuse(f, f.total - 16, f.n_segments, cap, "total_bytes smaller than the frames");
        must_refuse(f, f.total + 1, f.n_segments, cap + 16, "total_bytes no multiple of 16");
        must_refuse(f, (size_t)1 << 32, f.n_segments, cap, "total_bytes 2^32");
        must_refuse(f, f.total, f.n_segments + 1, cap + 32, "n_segments larger than the frames'");
        must_refuse(f, f.total, f.n_segments - 1, cap, "n_segments smaller than the frames'");
        must_refuse(f, f.total, -1, cap, "negative n_segments");
        for (size_t c : {cap - 1, cap - 16, f.total, (size_t)16, (size_t)0}) must_refuse(f, f.total, f.n_segments, c, "short capacity");
        g = f; g.desc.clear();                       must_refuse(g, 0, 0, cap, "no frames");
    }

    // zeroed
    {
        const std::vector<uint32_t> ids = {13, 4, 12, 9, 13};
        const Fetch f = describe(a, ids);
        auto must_zero = [&](const TestArena& ar, size_t arena_bytes, Fetch g, std::vector<bool> zero, const char* what) {
            // lay the descriptor out again from its own counts, so that it passes the host's checks
            g.total = 0; g.n_segments = 0;
            for (GatherDesc& d : g.desc) {
                d.dst = (uint32_t)g.total; d.first_segment = (uint32_t)g.n_segments;
                g.total += (d.len + 15) & ~15u; g.n_segments += (int)d.n_segments;
            }
            const size_t cap = tstar_jpeg_gather_bytes(g.total, (int)g.desc.size(), g.n_segments, nullptr);
            ++cases;
            const std::vector<uint8_t> want = expect(ar, g, zero);
            if (call(ar, arena_bytes, g, g.total, g.n_segments, cap, &got) != 0 || got != want) {
                ++differ;
                fprintf(stderr, "not zeroed: %s\n", what);
            } else {
                ++zeroed;
            }
        };
        Fetch g = f; g.desc[1].len += 1;             must_zero(a, a.bytes.size(), g, {false, true, false, false, false}, "a longer frame than the arena's");
        g = f; g.desc[2].len -= 1;                   must_zero(a, a.bytes.size(), g, {false, false, true, false, false}, "a shorter frame than the arena's");
        g = f; g.desc[3].n_segments += 2;            must_zero(a, a.bytes.size(), g, {false, false, false, true, false}, "more segments than the arena's");
        g = f; g.desc[0].n_segments = 0;             must_zero(a, a.bytes.size(), g, {true, false, false, false, false}, "no segments where the arena has some");
        must_zero(a, a.off[13], f, {true, false, false, false, true}, "an arena that ends before a frame does");
        TestArena b = a;
        b.off[4] = ~(uint64_t)0 - 3;                 must_zero(b, b.bytes.size(), f, {false, true, false, false, false}, "an offset that wraps");
        b = a; b.frames[12].first_segment = (int32_t)b.segments.size() - 1;
        must_zero(b, b.bytes.size(), f, {false, false, b.frames[12].n_segments > 1, false, false}, "segments beyond the arena's list");
        b = a; b.frames[9].first_segment = -1;       must_zero(b, b.bytes.size(), f, {false, false, false, true, false}, "a negative first segment");
        b = a; b.frames[9].n_segments = -5;          must_zero(b, b.bytes.size(), f, {false, false, false, true, false}, "a negative segment count");
    }
    printf("cases=%d refused=%d zeroed=%d differ=%d\n", cases, refused, zeroed, differ);
    return differ ? 1 : 0;
}
