// Stand-alone checker of the host twin of the re-coding with OPTIMISED tables, for sanitizer builds (host only): the scan stage
// with shared tables (tstar_jpeg_encode_scan_host_grp, jpeg_enc_host.cpp), the header with given quantisation tables AND given
// Huffman tables, and the assembly's mirror with long header rows and without an interval (jpeg_recode_host.cpp).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread
//       jpeg_recode_host.cpp jpeg_enc_host.cpp jpeg_host.cpp jpeg_recode_opt_check_main.cpp -o jpeg_recode_opt_check
//   jpeg_recode_opt_check
//
// It needs no input.  For tiny geometries of every sampling times intervals 0 (none), 1, 3 and 65535 (beyond the frame) it makes
// five frames of a fixed pseudo-random sequence at quality 100, puts frames 0, 1 into group 0, frame 2 into no group and frames
// 3, 4 into group 1, and codes them.  Every buffer is a heap block of EXACT size, so that AddressSanitizer sees a read or write one
// byte outside.  Checked: a group's counts are the sum of its frames' own; its tables are huff_optimal's of that sum; a frame
// without a group has status 3, length 0 and an untouched slot; every coded frame decodes (the planner takes header + scan, with one
// segment per interval, and the record buffer of the assembly is the planner's word on the output); the header entry at exact and
// short capacities and at its largest; counts that overflow keep their group's frames and no other; coefficients of 1024 and
// -32768 give status 2, still count, and touch no bin outside the histogram; groups that are not numbered in order, a pitch that is
// no multiple of 16 and an interval of 0 at the entry without _opt are refused.  Prints one line; exit status 1 on any difference.
#include "../../include/tstar_hip.h"
#include "jpeg_enc_host.h"
#include "jpeg_recode_core.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

namespace tstar {
void set_error(const std::string&) {}
}  // namespace tstar

using namespace tstar;
using namespace tstar::jpegrec;

namespace {

struct Case { int W, H, hs, vs; };
constexpr size_t kH = 4 * jpegenc::kHuffSymbols;

uint32_t g_state = 2463534242u;
uint32_t rnd() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}

struct Aligned {                     // an exact-size block at a 16-byte-aligned address
    uint8_t* p;
    size_t n;
    explicit Aligned(size_t bytes) : p((uint8_t*)aligned_alloc(16, (bytes + 15) / 16 * 16)), n(bytes) { memset(p, 0xEE, (bytes + 15) / 16 * 16); }
    ~Aligned() { free(p); }
    Aligned(const Aligned&) = delete;
};

int fail(const char* what, const Case& c, int restart) {
    printf("FAIL %s (%dx%d %dx%d interval %d)\n", what, c.W, c.H, c.hs, c.vs, restart);
    return 1;
}

int run_case(const Case& cs, int restart) {
    const JpegGeom g{cs.W, cs.H, 3, cs.hs, cs.vs};
    const int m = 5, quality = 100, n_groups = 2;
    const int32_t group[m] = {0, 0, -1, 1, 1};
    const size_t blocks = g.blocks(), per = blocks * 64;
    const int n_mcu = g.mcux() * g.mcuy();
    const uint32_t n_int = recode_intervals((uint32_t)n_mcu, (uint32_t)restart);
    uint16_t quant[192];
    jpeg_enc_quant(quality, quant);
    std::vector<std::vector<uint8_t>> files(m);
    std::vector<int16_t> coef((size_t)m * per);
    const size_t max_std = jpeg_enc_max_scan_bytes(g, 0);
    for (int i = 0; i < m; ++i) {
        std::vector<uint8_t> rgb((size_t)cs.W * cs.H * 3);
        for (uint8_t& v : rgb) v = (uint8_t)rnd();
        jpeg_enc_blocks(rgb.data(), g, quant, coef.data() + (size_t)i * per, nullptr);
        std::vector<uint8_t> f(kJpegEncHeaderBytes + max_std);
        jpeg_enc_header(g, quality, 0, f.data());
        size_t len = 0;
        if (jpeg_enc_scan(coef.data() + (size_t)i * per, g, 0, f.data() + kJpegEncHeaderBytes, max_std, &len, nullptr, nullptr) != JPEG_ENC_OK) return fail("source scan", cs, restart);
        f.resize(kJpegEncHeaderBytes + len);
        files[i] = f;
    }
    // spans
    int32_t span[2 * n_groups];
    if (tstar_jpeg_encode_group_spans(group, m, n_groups, cs.W, cs.H, cs.hs, cs.vs, span) != 0 || span[0] != 0 || span[1] != 2 || span[2] != 3 || span[3] != 5)
        return fail("spans", cs, restart);
    {
        const int32_t gap[m] = {0, 0, -1, 2, 2}, back[m] = {1, 1, -1, 0, 0}, low[m] = {0, 0, -2, 1, 1};
        if (tstar_jpeg_encode_group_spans(gap, m, 3, cs.W, cs.H, cs.hs, cs.vs, span) == 0 || tstar_jpeg_encode_group_spans(back, m, 2, cs.W, cs.H, cs.hs, cs.vs, span) == 0 ||
            tstar_jpeg_encode_group_spans(low, m, 2, cs.W, cs.H, cs.hs, cs.vs, span) == 0 || tstar_jpeg_encode_group_spans(group, m, 3, cs.W, cs.H, cs.hs, cs.vs, span) == 0)
            return fail("bad groups were accepted", cs, restart);
    }
    // the scans with the groups' tables, in slots of exact size
    const size_t slot = (jpeg_enc_max_scan_bytes(g, restart, 1) + 15) / 16 * 16;
    Aligned slots((size_t)m * slot);
    std::vector<uint32_t> scan_len(m), ghist(n_groups * kH);
    std::vector<int32_t> status(m);
    std::vector<uint8_t> specs((size_t)n_groups * 4 * kJpegEncSpecBytes);
    auto code = [&](const int16_t* cf, int stages) {
        return tstar_jpeg_encode_scan_host_grp(cf, m, cs.W, cs.H, cs.hs, cs.vs, restart, group, n_groups, stages, ghist.data(), specs.data(), slots.p, slot,
                                               scan_len.data(), status.data(), 1);
    };
    if (code(coef.data(), 7) != 0) return fail("scan with shared tables", cs, restart);
    std::vector<uint32_t> sum(n_groups * kH, 0), one(kH);
    for (int i = 0; i < m; ++i) {
        if (group[i] < 0) continue;
        jpeg_enc_gather(coef.data() + (size_t)i * per, g, restart, one.data());
        for (size_t k = 0; k < kH; ++k) sum[(size_t)group[i] * kH + k] += one[k];
    }
    if (sum != ghist) return fail("group counts", cs, restart);
    const jpegenc::HuffSpecWide* sp = (const jpegenc::HuffSpecWide*)specs.data();
    for (int q = 0; q < 4 * n_groups; ++q) {
        jpegenc::HuffSpecWide s;
        jpegenc::HuffCodes h;
        jpegenc::huff_optimal(sum.data() + (size_t)q * jpegenc::kHuffSymbols, s, h, nullptr);
        if (memcmp(&s, sp + q, sizeof s) != 0 || s.status != jpegenc::HUFF_OK) return fail("group tables", cs, restart);
    }
    for (int i = 0; i < m; ++i) {
        if (group[i] < 0) {
            if (status[i] != JPEG_ENC_HUFF_OVERFLOW || scan_len[i] != 0) return fail("a frame without a group", cs, restart);
            for (size_t k = 0; k < slot; ++k) if (slots.p[(size_t)i * slot + k] != 0xEE) return fail("a frame without a group was written", cs, restart);
        } else if (status[i] != JPEG_ENC_OK || scan_len[i] < 2) return fail("scan status", cs, restart);
    }
    // headers: one row per group, exact and short capacities, the largest
    const size_t pitch = kHeaderPitchOpt;
    Aligned headers((size_t)n_groups * pitch);
    uint32_t header_len[n_groups];
    for (int q = 0; q < n_groups; ++q) {
        size_t hlen = 0;
        if (tstar_jpeg_encode_header_tables_opt(cs.W, cs.H, quant, cs.hs, cs.vs, restart, specs.data() + (size_t)q * 4 * kJpegEncSpecBytes, headers.p + q * pitch, pitch, &hlen) != 0)
            return fail("header", cs, restart);
        header_len[q] = (uint32_t)hlen;
        std::vector<uint8_t> exact(hlen), ref(kJpegEncHeaderOptMax + kJpegEncDriBytes), shorter(hlen - 1, 0xEE);
        size_t n = 0;
        const size_t rn = jpeg_enc_header_opt(g, quality, restart, sp + 4 * q, ref.data());
        if (tstar_jpeg_encode_header_tables_opt(cs.W, cs.H, quant, cs.hs, cs.vs, restart, (const uint8_t*)(sp + 4 * q), exact.data(), hlen, &n) != 0 || rn != hlen ||
            memcmp(exact.data(), ref.data(), hlen) != 0)
            return fail("exact header", cs, restart);
        if (tstar_jpeg_encode_header_tables_opt(cs.W, cs.H, quant, cs.hs, cs.vs, restart, (const uint8_t*)(sp + 4 * q), shorter.data(), hlen - 1, &n) != 4) return fail("short header", cs, restart);
        for (uint8_t v : shorter) if (v != 0xEE) return fail("short header wrote", cs, restart);
    }
    {
        jpegenc::HuffSpecWide full[4];
        memset(full, 0, sizeof full);
        for (auto& s : full) { s.bits[15] = 255; s.bits[14] = 1; s.nvals = 256; for (int i = 0; i < 256; ++i) s.vals[i] = (uint8_t)i; }
        uint16_t wide[192];
        for (int k = 0; k < 192; ++k) wide[k] = (uint16_t)(256 + (k * 733) % 60000);
        std::vector<uint8_t> big(kJpegEncHeaderTablesOptMax);
        size_t n = 0;
        if (tstar_jpeg_encode_header_tables_opt(cs.W, cs.H, wide, cs.hs, cs.vs, 65535, (const uint8_t*)full, big.data(), big.size(), &n) != 0 || n != big.size() || n > pitch)
            return fail("widest header", cs, restart);
        full[2].status = 1;
        if (tstar_jpeg_encode_header_tables_opt(cs.W, cs.H, wide, cs.hs, cs.vs, 1, (const uint8_t*)full, big.data(), big.size(), &n) != 1) return fail("a table with a status", cs, restart);
    }
    // the source batch and the piece: frame 2 kept
    std::vector<const uint8_t*> ptrs(m);
    std::vector<size_t> lens(m);
    std::vector<uint64_t> offs(m);
    size_t src_total = 0;
    for (int i = 0; i < m; ++i) { ptrs[i] = files[i].data(); lens[i] = files[i].size(); offs[i] = src_total; src_total += lens[i]; }
    std::vector<uint8_t> src(src_total);
    for (int i = 0; i < m; ++i) memcpy(src.data() + offs[i], files[i].data(), lens[i]);
    std::vector<int32_t> route(m);
    std::vector<JpegFrameDesc> sframes(m);
    Aligned squant((size_t)m * 384);
    std::vector<JpegTableSet> ssets(4);
    std::vector<JpegSegment> ssegs(m + 1);
    size_t out5[5];
    if (tstar_jpeg_plan_segments(ptrs.data(), lens.data(), offs.data(), m, cs.W, cs.H, 3, cs.hs, cs.vs, route.data(), sframes.data(),
                                 (uint16_t*)squant.p, ssets.data(), 4, ssegs.data(), m + 1, out5) != 0 || out5[1] != (size_t)m)
        return fail("source plan", cs, restart);
    std::vector<RecodeDesc> desc(m);
    std::vector<std::vector<uint8_t>> want(m);
    uint32_t nseg = 0;
    size_t total = 0;
    for (int j = 0; j < m; ++j) {
        RecodeDesc& d = desc[j];
        memset(&d, 0, sizeof d);
        d.src = (uint32_t)j;
        d.first_segment = nseg;
        if (group[j] < 0) {
            d.kind = RECODE_KEPT; d.src_off = (uint32_t)offs[j]; d.src_len = (uint32_t)lens[j]; d.table_set = 2; d.n_segments = 1;
            want[j] = files[j];
        } else {
            d.kind = RECODE_NEW; d.hdr = (uint32_t)group[j]; d.table_set = group[j]; d.n_segments = n_int;
            want[j].assign(headers.p + d.hdr * pitch, headers.p + d.hdr * pitch + header_len[d.hdr]);
            want[j].insert(want[j].end(), slots.p + (size_t)j * slot, slots.p + (size_t)j * slot + scan_len[j]);
        }
        nseg += d.n_segments;
        total += want[j].size();
    }
    const size_t nrec = tstar_jpeg_recode_layout(m, (int)nseg, out5);
    if (!nrec) return fail("layout", cs, restart);
    Aligned rec(nrec);
    std::vector<uint8_t> out(total, 0xEE);
    auto assemble = [&](size_t row, uint8_t* r, uint8_t* o) {
        return tstar_jpeg_recode_assemble_host_opt(desc.data(), m, (int)nseg, headers.p, row, header_len, n_groups, slots.p, slot, scan_len.data(), restart, n_mcu,
                                                   src.data(), src_total, (const uint16_t*)squant.p, sframes.data(), ssegs.data(), m, m, r, nrec, o, total);
    };
    if (assemble(pitch, rec.p, out.data()) != 0) return fail("assemble", cs, restart);
    Records r;
    recode_layout(m, (int)nseg, &r);
    recode_views(rec.p, &r);
    std::vector<const uint8_t*> optrs(m);
    std::vector<size_t> olens(m);
    std::vector<uint64_t> ooffs(m);
    size_t at = 0;
    for (int j = 0; j < m; ++j) {
        if (r.off[j] != at || r.len[j] != want[j].size() || memcmp(out.data() + at, want[j].data(), want[j].size()) != 0) return fail("output bytes", cs, restart);
        optrs[j] = out.data() + at; olens[j] = want[j].size(); ooffs[j] = at;
        at += want[j].size();
    }
    std::vector<JpegFrameDesc> pframes(m);
    std::vector<uint16_t> pquant((size_t)m * 192);
    std::vector<JpegTableSet> psets(4);
    std::vector<JpegSegment> psegs(nseg + 1);
    if (tstar_jpeg_plan_segments(optrs.data(), olens.data(), ooffs.data(), m, cs.W, cs.H, 3, cs.hs, cs.vs, route.data(), pframes.data(), pquant.data(),
                                 psets.data(), 4, psegs.data(), (int)nseg + 1, out5) != 0 || out5[1] != nseg)
        return fail("plan of the output", cs, restart);
    for (int j = 0; j < m; ++j) if (route[j] != 0) return fail("the planner does not take an output frame", cs, restart);
    if (memcmp(psegs.data(), r.segments, (size_t)nseg * sizeof(JpegSegment)) != 0) return fail("segments", cs, restart);
    if (memcmp(pquant.data(), r.quant, (size_t)m * 384) != 0) return fail("quant rows", cs, restart);
    for (int j = 0; j < m; ++j)
        if (r.frames[j].first_segment != pframes[j].first_segment || r.frames[j].n_segments != pframes[j].n_segments || r.frames[j].table_set != desc[j].table_set)
            return fail("frame records", cs, restart);
    // and the output decodes to the source's coefficients
    {
        std::vector<int16_t> back((size_t)m * per);
        std::vector<int32_t> seg_status(nseg);
        if (tstar_jpeg_entropy_segments_host(out.data(), total, psegs.data(), psets.data(), (int)out5[0], pframes.data(), m, (int)nseg, cs.W, cs.H, 3, cs.hs, cs.vs, back.data(),
                                             seg_status.data()) != 0)
            return fail("decode of the output", cs, restart);
        for (int32_t s : seg_status) if (s != 0) return fail("a segment of the output does not decode", cs, restart);
        if (back != coef) return fail("the output's coefficients are not the source's", cs, restart);
    }
    // refused: a pitch that is no multiple of 16; an interval of 0 at the entry without _opt (both leave the buffers alone)
    {
        std::vector<uint8_t> o3(total, 0xEE);
        Aligned rec3(nrec);
        if (assemble(pitch - 8, rec3.p, o3.data()) == 0) return fail("a pitch of no multiple of 16 was accepted", cs, restart);
        if (restart == 0 && tstar_jpeg_recode_assemble_host(desc.data(), m, (int)nseg, headers.p, header_len, n_groups, slots.p, slot, scan_len.data(), 0, n_mcu, src.data(),
                                                            src_total, (const uint16_t*)squant.p, sframes.data(), ssegs.data(), m, m, rec3.p, nrec, o3.data(), total) == 0)
            return fail("an interval of 0 was accepted without _opt", cs, restart);
        for (uint8_t v : o3) if (v != 0xEE) return fail("a refused call wrote bytes", cs, restart);
        for (size_t i = 0; i < nrec; ++i) if (rec3.p[i] != 0xEE) return fail("a refused call wrote records", cs, restart);
    }
    // counts that overflow (33 symbols with the counts 1, 2, 3, 5, 8, ...: beside the reserved symbol the rarest sits 33 deep) in group 0's first table keep group 0 only
    {
        std::vector<uint32_t> keep = ghist;
        uint32_t a = 1, b = 2;
        for (int i = 0; i < 33; ++i) { ghist[i] = a; const uint32_t c = a + b; a = b; b = c; }
        memset(slots.p, 0xEE, (size_t)m * slot);
        if (code(coef.data(), 6) != 0) return fail("scan with crafted counts", cs, restart);
        if (sp[0].status != jpegenc::HUFF_CLEN_OVERFLOW) return fail("the crafted counts do not overflow", cs, restart);
        for (int i = 0; i < m; ++i) {
            const bool coded = group[i] == 1;
            if (status[i] != (coded ? JPEG_ENC_OK : JPEG_ENC_HUFF_OVERFLOW) || (scan_len[i] != 0) != coded) return fail("overflow status", cs, restart);
            if (!coded)
                for (size_t k = 0; k < slot; ++k) if (slots.p[(size_t)i * slot + k] != 0xEE) return fail("a frame of an overflowing group was written", cs, restart);
        }
        ghist = keep;
    }
    // coefficients without a code: status 2, counted all the same, inside the histogram
    {
        std::vector<int16_t> cf = coef;
        cf[5] = 1024;                                     // frame 0, an AC coefficient of category 11
        cf[(size_t)3 * per + 64 + 9] = -32768;            // frame 3, category 16
        cf[(size_t)4 * per] = -32768;                     // frame 4, a DC difference beyond category 11
        if (code(cf.data(), 7) != 0) return fail("scan with bad coefficients", cs, restart);
        if (status[0] != JPEG_ENC_BAD_COEF || status[3] != JPEG_ENC_BAD_COEF || status[4] != JPEG_ENC_BAD_COEF || status[1] != JPEG_ENC_OK)
            return fail("bad coefficient status", cs, restart);
        uint64_t dc = 0;
        for (int i = 0; i < 12; ++i) dc += ghist[i] + ghist[2 * jpegenc::kHuffSymbols + i];
        if (dc != 2 * blocks) return fail("a frame with a bad coefficient did not count", cs, restart);
    }
    return 0;
}

}  // namespace

int main() {
    const Case cases[] = {{8, 8, 2, 2}, {16, 16, 2, 2}, {17, 9, 2, 2}, {48, 48, 2, 2}, {40, 24, 2, 1}, {24, 40, 1, 1}, {23, 17, 1, 1}};
    const int intervals[] = {0, 1, 3, 65535};
    int bad = 0, n = 0;
    for (const Case& cs : cases)
        for (int restart : intervals) { bad |= run_case(cs, restart); ++n; }
    if (tstar_jpeg_encode_group_frames(1920, 1080, 2, 2) != 1000000000 / (64 * 48960) || tstar_jpeg_encode_group_frames(16384, 16384, 1, 1) != 1) {
        printf("FAIL group_frames\n");
        bad = 1;
    }
    printf("%s: %d cases\n", bad ? "FAILED" : "ok", n);
    return bad;
}
