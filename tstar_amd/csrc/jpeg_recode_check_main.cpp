// Stand-alone checker of the re-code assembly's host mirror (jpeg_recode_host.cpp) and of the header writer with given tables
// (jpeg_enc_host.cpp), for sanitizer builds (host only):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -pthread
//       jpeg_recode_host.cpp jpeg_enc_host.cpp jpeg_host.cpp jpeg_recode_check_main.cpp -o jpeg_recode_check
//   jpeg_recode_check
//
// It needs no input.  For tiny geometries of every sampling times intervals from 1 MCU to beyond the frame it encodes frames of a
// fixed pseudo-random sequence at quality 100 (long scans, 0xFF bytes), takes their coefficients' scans with the interval into
// slots, and assembles pieces in which every third frame is KEPT (its source file as it is).  Slots, headers, the source batch,
// the record buffer and the output live in heap blocks of EXACT size, so that AddressSanitizer sees a read or write one byte
// outside.  Checked: the output is header + scan (or the source file) end to end; the records are what tstar_jpeg_plan_segments
// says about the output; an output capacity one frame short drops that frame whole (no bytes, no table set) and touches nothing
// behind the capacity; descriptors that do not tile, name a header, a source frame or a kind that is not there are refused with
// every buffer left as it was; the header entry at exact and short capacities.  Prints one line; exit status 1 on any difference.
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
    const int m = 5, quality = 100;
    const size_t blocks = g.blocks();
    const int n_mcu = g.mcux() * g.mcuy();
    const uint32_t n_int = recode_intervals((uint32_t)n_mcu, (uint32_t)restart);
    uint16_t quant[192];
    jpeg_enc_quant(quality, quant);
    // the source batch: whole files (without an interval), end to end, planned by the planner
    std::vector<std::vector<uint8_t>> files(m);
    std::vector<int16_t> coef((size_t)m * blocks * 64);
    const size_t max_scan = jpeg_enc_max_scan_bytes(g, restart);
    for (int i = 0; i < m; ++i) {
        std::vector<uint8_t> rgb((size_t)cs.W * cs.H * 3);
        for (uint8_t& v : rgb) v = (uint8_t)rnd();
        jpeg_enc_blocks(rgb.data(), g, quant, coef.data() + (size_t)i * blocks * 64, nullptr);
        std::vector<uint8_t> f(kJpegEncHeaderBytes + max_scan);
        jpeg_enc_header(g, quality, 0, f.data());
        size_t len = 0;
        if (jpeg_enc_scan(coef.data() + (size_t)i * blocks * 64, g, 0, f.data() + kJpegEncHeaderBytes, max_scan, &len, nullptr, nullptr) != JPEG_ENC_OK) return fail("source scan", cs, restart);
        f.resize(kJpegEncHeaderBytes + len);
        files[i] = f;
    }
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
    // the scans with the interval, in slots
    const size_t slot = (max_scan + 15) / 16 * 16;
    Aligned slots((size_t)m * slot);
    std::vector<uint32_t> scan_len(m);
    for (int i = 0; i < m; ++i) {
        size_t len = 0;
        if (jpeg_enc_scan(coef.data() + (size_t)i * blocks * 64, g, restart, slots.p + (size_t)i * slot, slot, &len, nullptr, nullptr) != JPEG_ENC_OK)
            return fail("scan with the interval", cs, restart);
        scan_len[i] = (uint32_t)len;
    }
    // one header row; exact and short capacities of the header entry
    Aligned headers(kHeaderPitch);
    size_t hlen = 0;
    if (tstar_jpeg_encode_header_tables(cs.W, cs.H, quant, cs.hs, cs.vs, restart, headers.p, kHeaderPitch, &hlen) != 0 ||
        hlen != (size_t)jpeg_enc_header_bytes(restart))
        return fail("header", cs, restart);
    {
        std::vector<uint8_t> exact(hlen), ref(hlen), shorter(hlen - 1, 0xEE);
        size_t n = 0;
        jpeg_enc_header(g, quality, restart, ref.data());
        if (tstar_jpeg_encode_header_tables(cs.W, cs.H, quant, cs.hs, cs.vs, restart, exact.data(), hlen, &n) != 0 || exact != ref) return fail("exact header", cs, restart);
        if (tstar_jpeg_encode_header_tables(cs.W, cs.H, quant, cs.hs, cs.vs, restart, shorter.data(), hlen - 1, &n) != 4) return fail("short header", cs, restart);
        for (uint8_t v : shorter) if (v != 0xEE) return fail("short header wrote", cs, restart);
        uint16_t wide[192];
        for (int k = 0; k < 192; ++k) wide[k] = (uint16_t)(1 + (k * 733) % 60000);
        std::vector<uint8_t> big(kJpegEncHeaderTablesMax);
        if (tstar_jpeg_encode_header_tables(cs.W, cs.H, wide, cs.hs, cs.vs, 65535, big.data(), big.size(), &n) != 0 || n != big.size()) return fail("widest header", cs, restart);
        wide[7] = 0;
        if (tstar_jpeg_encode_header_tables(cs.W, cs.H, wide, cs.hs, cs.vs, 1, big.data(), big.size(), &n) != 1) return fail("zero table entry", cs, restart);
    }
    const uint32_t header_len[1] = {(uint32_t)hlen};
    // the piece: every third frame kept
    std::vector<RecodeDesc> desc(m);
    std::vector<std::vector<uint8_t>> want(m);
    uint32_t nseg = 0;
    size_t total = 0;
    for (int j = 0; j < m; ++j) {
        RecodeDesc& d = desc[j];
        memset(&d, 0, sizeof d);
        d.src = (uint32_t)j;
        d.first_segment = nseg;
        if (j % 3 == 1) {
            d.kind = RECODE_KEPT; d.src_off = (uint32_t)offs[j]; d.src_len = (uint32_t)lens[j]; d.table_set = 1; d.n_segments = 1;
            want[j] = files[j];
        } else {
            d.kind = RECODE_NEW; d.hdr = 0; d.table_set = 0; d.n_segments = n_int;
            want[j].assign(headers.p, headers.p + hlen);
            want[j].insert(want[j].end(), slots.p + (size_t)j * slot, slots.p + (size_t)j * slot + scan_len[j]);
        }
        nseg += d.n_segments;
        total += want[j].size();
    }
    const size_t nrec = tstar_jpeg_recode_layout(m, (int)nseg, out5);
    if (!nrec) return fail("layout", cs, restart);
    auto call = [&](const std::vector<RecodeDesc>& dd, uint8_t* rec, uint8_t* out, size_t cap) {
        return tstar_jpeg_recode_assemble_host(dd.data(), m, (int)nseg, headers.p, header_len, 1, slots.p, slot, scan_len.data(), restart, n_mcu,
                                               src.data(), src_total, (const uint16_t*)squant.p, sframes.data(), ssegs.data(), m, m, rec, nrec,
                                               out, cap);
    };
    Aligned rec(nrec);
    std::vector<uint8_t> out(total, 0xEE);
    if (call(desc, rec.p, out.data(), total) != 0) return fail("assemble", cs, restart);
    Records r;
    recode_layout(m, (int)nseg, &r);
    recode_views(rec.p, &r);
    // bytes, and the records against the planner over the output
    std::vector<const uint8_t*> optrs(m);
    std::vector<size_t> olens(m);
    std::vector<uint64_t> ooffs(m);
    size_t at = 0;
    for (int j = 0; j < m; ++j) {
        if (r.off[j] != at || r.len[j] != want[j].size() || memcmp(out.data() + at, want[j].data(), want[j].size()) != 0) return fail("output bytes", cs, restart);
        optrs[j] = out.data() + at; olens[j] = want[j].size(); ooffs[j] = at;
        at += want[j].size();
    }
    if (r.off[m] != total) return fail("total", cs, restart);
    std::vector<JpegFrameDesc> pframes(m);
    std::vector<uint16_t> pquant((size_t)m * 192);
    std::vector<JpegTableSet> psets(4);
    std::vector<JpegSegment> psegs(nseg + 1);
    if (tstar_jpeg_plan_segments(optrs.data(), olens.data(), ooffs.data(), m, cs.W, cs.H, 3, cs.hs, cs.vs, route.data(), pframes.data(), pquant.data(),
                                 psets.data(), 4, psegs.data(), (int)nseg + 1, out5) != 0 || out5[1] != nseg)
        return fail("plan of the output", cs, restart);
    if (memcmp(psegs.data(), r.segments, (size_t)nseg * sizeof(JpegSegment)) != 0) return fail("segments", cs, restart);
    if (memcmp(pquant.data(), r.quant, (size_t)m * 384) != 0) return fail("quant rows", cs, restart);
    for (int j = 0; j < m; ++j)
        if (r.frames[j].first_segment != pframes[j].first_segment || r.frames[j].n_segments != pframes[j].n_segments ||
            r.frames[j].table_set != desc[j].table_set || r.frames[j].reserved != 0)
            return fail("frame records", cs, restart);
    // a capacity one byte short of the last frame: that frame is dropped whole, nothing is written behind the capacity
    {
        const size_t cap = total - 1;
        std::vector<uint8_t> o2(cap, 0xEE);
        Aligned rec2(nrec);
        if (call(desc, rec2.p, o2.data(), cap) != 0) return fail("short output", cs, restart);
        Records r2;
        recode_layout(m, (int)nseg, &r2);
        recode_views(rec2.p, &r2);
        if (r2.frames[m - 1].table_set != -1 || r2.frames[m - 1].n_segments != 0) return fail("short output: last record", cs, restart);
        if (memcmp(o2.data(), out.data(), total - want[m - 1].size()) != 0) return fail("short output: other frames", cs, restart);
        for (size_t i = total - want[m - 1].size(); i < cap; ++i) if (o2[i] != 0xEE) return fail("short output: wrote a dropped frame", cs, restart);
    }
    // refused descriptors leave every buffer as it was
    for (int k = 0; k < 7; ++k) {
        std::vector<RecodeDesc> dd = desc;
        switch (k) {
            case 0: dd[1].first_segment += 1; break;
            case 1: dd[0].n_segments += 1; break;
            case 2: dd[0].hdr = 1; break;
            case 3: dd[2].src = (uint32_t)m; break;
            case 4: dd[2].kind = 2; break;
            case 5: dd[1].src_len = (uint32_t)src_total + 1; break;
            default: dd[0].table_set = -1; break;
        }
        std::vector<uint8_t> o3(total, 0xEE);
        Aligned rec3(nrec);
        if (call(dd, rec3.p, o3.data(), total) == 0) return fail("a bad descriptor was accepted", cs, restart);
        for (uint8_t v : o3) if (v != 0xEE) return fail("a refused call wrote bytes", cs, restart);
        for (size_t i = 0; i < nrec; ++i) if (rec3.p[i] != 0xEE) return fail("a refused call wrote records", cs, restart);
    }
    return 0;
}

}  // namespace

int main() {
    const Case cases[] = {{8, 8, 2, 2}, {16, 16, 2, 2}, {17, 9, 2, 2}, {48, 48, 2, 2}, {40, 24, 2, 1}, {24, 40, 1, 1}, {23, 17, 1, 1}};
    const int intervals[] = {1, 2, 3, 8, 64, 65535};
    int bad = 0, n = 0;
    for (const Case& cs : cases)
        for (int restart : intervals) { bad |= run_case(cs, restart); ++n; }
    printf("%s: %d cases\n", bad ? "FAILED" : "ok", n);
    return bad;
}
