// Baseline JPEG encoder, host half: see jpeg_enc_host.h.  HIP-free; every integer comes from jpeg_enc_math.h, which the
// kernels of jpeg_enc.hip share.
#include "jpeg_enc_host.h"

#include <string.h>

#include <atomic>
#include <initializer_list>
#include <string>
#include <thread>
#include <vector>

namespace tstar {

void set_error(const std::string& msg);          // capi.hip (or the stand-alone checker): thread-local last error

namespace {
constexpr jpegenc::EncTables kTables = jpegenc::make_tables();
}

bool jpeg_enc_geom_ok(const JpegGeom& g) {
    return g.W > 0 && g.H > 0 && g.W <= 16384 && g.H <= 16384 && g.ncomp == 3 &&
           ((g.hs == 1 && g.vs == 1) || (g.hs == 2 && (g.vs == 1 || g.vs == 2)));
}

size_t jpeg_enc_max_scan_bytes(const JpegGeom& g) { return 2 * ((g.blocks() * (size_t)jpegenc::kMaxBlockBits + 7) / 8) + 2; }

size_t jpeg_enc_restart_markers(const JpegGeom& g, int restart) {
    return restart > 0 ? ((size_t)g.mcux() * g.mcuy() - 1) / (size_t)restart : 0;
}
size_t jpeg_enc_max_scan_bytes(const JpegGeom& g, int restart) { return jpeg_enc_max_scan_bytes(g) + 4 * jpeg_enc_restart_markers(g, restart); }
size_t jpeg_enc_max_scan_bytes(const JpegGeom& g, int restart, int optimize) {
    if (!optimize) return jpeg_enc_max_scan_bytes(g, restart);
    return 2 * ((g.blocks() * (size_t)jpegenc::kMaxBlockBitsOpt + 7) / 8) + 2 + 4 * jpeg_enc_restart_markers(g, restart);
}

JpegEncPlan plan_jpeg_encode(const JpegGeom& g, int n, size_t slot_bytes, int restart, int optimize) {
    JpegEncPlan p = {};
    const size_t block_bits = optimize ? (size_t)jpegenc::kMaxBlockBitsOpt : (size_t)jpegenc::kMaxBlockBits;
    if (!jpeg_enc_restart_ok(restart)) { p.error = "restart interval must be in 0..65535 MCUs (DRI holds 16 bits)"; return p; }
    if (!jpeg_enc_geom_ok(g)) { p.error = "unsupported geometry (3 components, sampling 2x2 / 2x1 / 1x1, sides 1..16384)"; return p; }
    if (n < 1 || n > 65535) { p.error = "n must be in 1..65535"; return p; }
    p.blocks = g.blocks();
    p.restart = restart;
    p.markers = jpeg_enc_restart_markers(g, restart);
    if (p.blocks * block_bits + p.markers * (size_t)jpegenc::kRestartBits >= (1ull << 32)) { p.error = "frame too large: a scan's bit offsets would not fit 32 bits"; return p; }
    if (slot_bytes < 2 || slot_bytes >= (1ull << 31)) { p.error = "slot_bytes must be in 2..2^31-1"; return p; }
    p.coef_bytes = p.blocks * 128;
    p.max_scan_bytes = jpeg_enc_max_scan_bytes(g, restart, optimize);
    p.header_bytes = (size_t)jpeg_enc_header_bytes(restart, optimize);
    // with markers the unstuffed stream holds them and the padding in front of them: 3 bytes more per marker at most
    const size_t max_raw = (p.blocks * block_bits + 7) / 8 + 3 * p.markers;
    const size_t raw_cap = slot_bytes < max_raw ? slot_bytes : max_raw;      // unstuffed bytes never exceed the stuffed ones
    p.raw_words = raw_cap / 4 + 1;
    p.ff_chunks = (p.raw_words * 4 + kJpegEncStuffChunk - 1) / kJpegEncStuffChunk;
    auto up = [](size_t v) { return (v + 15) / 16 * 16; };
    p.off_meta = 0;
    p.off_bits = up((size_t)n * 4 * sizeof(uint32_t));
    p.off_raw = p.off_bits + up((size_t)n * p.blocks * sizeof(uint32_t));
    p.off_ff = p.off_raw + up((size_t)n * p.raw_words * sizeof(uint32_t));
    p.workspace_bytes = p.off_ff + up((size_t)n * p.ff_chunks * sizeof(uint32_t));
    if (restart > 0) {
        p.off_seg = p.workspace_bytes;
        p.off_mark = p.off_seg + up((size_t)n * (p.markers + 1) * sizeof(uint32_t));
        p.workspace_bytes = p.off_mark + up((size_t)n * p.markers * sizeof(uint32_t));
    }
    if (optimize) {
        p.optimize = 1;
        p.off_hist = p.workspace_bytes;
        p.off_codes = p.off_hist + up((size_t)n * 4 * jpegenc::kHuffSymbols * sizeof(uint32_t));
        p.workspace_bytes = p.off_codes + up((size_t)n * 4 * sizeof(jpegenc::HuffCodes));
    }
    const size_t total_blocks = (size_t)n * p.blocks;
    if (total_blocks / 32 + 1 >= 0x7fffffffull) { p.error = "chunk too large for one launch"; return p; }
    p.block_wgs = (unsigned)((total_blocks + 31) / 32);
    p.entropy_wgs_x = (unsigned)((p.blocks + 255) / 256);
    p.stuff_wgs_x = (unsigned)((p.ff_chunks + 255) / 256);
    return p;
}

void jpeg_enc_quant(int quality, uint16_t* quant) {
    const int scale = jpegenc::quality_scale(quality);
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) quant[c * 64 + k] = (uint16_t)jpegenc::quant_entry(jpegenc::kStd.q[c ? 1 : 0][k], scale);
}

void jpeg_enc_header(const JpegGeom& g, int quality, int restart, uint8_t* out) {
    uint16_t quant[192];
    jpeg_enc_quant(quality, quant);
    jpeg_enc_header_tables(g, quant, restart, out);
}

namespace {
// SOI .. SOS; specs: the four tables of the DHT segments (null: the Annex K tables)
size_t write_header(const JpegGeom& g, const uint16_t* quant, int restart, const jpegenc::HuffSpecWide* specs, uint8_t* out) {
    uint8_t* p = out;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) *p++ = (uint8_t)b; };
    const int n_tables = memcmp(quant + 64, quant + 128, 128) == 0 ? 2 : 3;       // Cb and Cr share table 1 when their rows are equal
    bool wide = false;
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < n_tables; ++t) {
        const uint16_t* q = quant + t * 64;
        int prec = 0;
        for (int k = 0; k < 64; ++k) prec |= q[k] > 255;
        wide |= prec != 0;
        put({0xFF, 0xDB, 0, 67 + 64 * prec, (prec << 4) | t});
        for (int k = 0; k < 64; ++k) {
            const uint16_t v = q[jpegenc::kStd.zigzag[k]];
            if (prec) *p++ = (uint8_t)(v >> 8);
            *p++ = (uint8_t)v;
        }
    }
    // a 16-bit table is not baseline: libjpeg then writes SOF1 (extended sequential, Huffman)
    put({0xFF, wide ? 0xC1 : 0xC0, 0, 17, 8, g.H >> 8, g.H & 255, g.W >> 8, g.W & 255, 3, 1, (g.hs << 4) | g.vs, 0, 2, 0x11, 1, 3, 0x11,
         n_tables - 1});
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};                // DC 0, AC 0, DC 1, AC 1
    for (int t = 0; t < 4; ++t) {
        const uint8_t* bits = specs ? specs[t].bits : kTables.spec[t].bits;
        const uint8_t* vals = specs ? specs[t].vals : kTables.spec[t].vals;
        const int nvals = specs ? (int)specs[t].nvals : kTables.spec[t].nvals;
        const int len = 2 + 1 + 16 + nvals;
        put({0xFF, 0xC4, len >> 8, len & 255, ids[t]});
        for (int i = 0; i < 16; ++i) *p++ = bits[i];
        for (int i = 0; i < nvals; ++i) *p++ = vals[i];
    }
    if (restart > 0) put({0xFF, 0xDD, 0, 4, restart >> 8, restart & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return (size_t)(p - out);
}
}  // namespace

size_t jpeg_enc_header_tables(const JpegGeom& g, const uint16_t* quant, int restart, uint8_t* out) { return write_header(g, quant, restart, nullptr, out); }

size_t jpeg_enc_header_opt(const JpegGeom& g, int quality, int restart, const jpegenc::HuffSpecWide* specs, uint8_t* out) {
    uint16_t quant[192];
    jpeg_enc_quant(quality, quant);
    return write_header(g, quant, restart, specs, out);
}

size_t jpeg_enc_header_tables_opt(const JpegGeom& g, const uint16_t* quant, int restart, const jpegenc::HuffSpecWide* specs, uint8_t* out) {
    return write_header(g, quant, restart, specs, out);
}

const char* jpeg_enc_groups_check(const int32_t* group, int n, int n_groups, size_t blocks, int32_t* span) {
    if (!group || n < 1 || n_groups < 1 || n_groups > n) return "no group, or more groups than frames";
    const int most = jpeg_enc_group_frames(blocks);
    int last = -1, members = 0;
    for (int f = 0; f < n; ++f) {
        const int g = group[f];
        if (g == -1) continue;
        if (g < 0 || g >= n_groups) return "a frame's group outside -1 .. n_groups - 1";
        if (g != last && g != last + 1) return "the groups are not numbered in frame order without a gap";
        if (g != last) { members = 0; if (span) span[2 * g] = f; }
        if (++members > most) return "a group holds more frames than keep its counts within 1000000000";
        if (span) span[2 * g + 1] = f + 1;
        last = g;
    }
    if (last != n_groups - 1) return "a group without a frame";
    return nullptr;
}

void jpeg_enc_blocks(const uint8_t* rgb, const JpegGeom& g, const uint16_t* quant, int16_t* coef, uint64_t* dummy2) {
    const int real_bw = (g.W + 7) / 8, real_bh = (g.H + 7) / 8;
    for (int c = 0; c < 3; ++c) {
        const int bw = g.bw(c), bh = g.bh(c);
        int16_t* cc = coef + g.block_offset(c) * 64;
        const uint16_t* q = quant + 64 * c;
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx) {
                int16_t* o = cc + ((size_t)by * bw + bx) * 64;
                if (c == 0 && (by >= real_bh || bx >= real_bw)) {       // DC in the second loop below
                    memset(o, 0, 128);
                    continue;
                }
                int32_t ws[64];
                for (int r = 0; r < 8; ++r) {
                    int32_t d[8];
                    for (int i = 0; i < 8; ++i) d[i] = jpegenc::sample_at(rgb, g.W, g.H, g.hs, g.vs, c, by * 8 + r, bx * 8 + i) - 128;
                    jpegenc::fdct8<true>(d, ws + r * 8);
                }
                for (int i = 0; i < 8; ++i) {
                    int32_t d[8], t[8];
                    for (int r = 0; r < 8; ++r) d[r] = ws[r * 8 + i];
                    jpegenc::fdct8<false>(d, t);
                    for (int r = 0; r < 8; ++r) o[r * 8 + i] = (int16_t)jpegenc::quantise(t[r], q[r * 8 + i]);
                }
            }
    }
    const int bw0 = g.bw(0), bh0 = g.bh(0);
    for (int by = 0; by < bh0; ++by)
        for (int bx = 0; bx < bw0; ++bx) {
            int kind = 0;
            const int src = jpegenc::dummy_source(by, bx, real_bw, real_bh, g.hs, bw0, &kind);
            if (src < 0) continue;
            coef[((size_t)by * bw0 + bx) * 64] = coef[(size_t)src * 64];
            if (dummy2) ++dummy2[kind];
        }
}

namespace {

struct ByteSink {                        // MSB-first bit writer with FF -> FF 00
    std::vector<uint8_t> bytes;
    uint64_t acc = 0, stuffed = 0;
    int nb = 0;
    void byte(uint8_t b) {
        bytes.push_back(b);
        if (b == 0xFF) { bytes.push_back(0); ++stuffed; }
    }
    void operator()(unsigned code, int len) {
        acc = (acc << len) | code;
        nb += len;
        while (nb >= 8) {
            byte((uint8_t)(acc >> (nb - 8)));
            nb -= 8;
        }
    }
    // fills the current byte with one-bits (stuffed like any byte when that makes 0xFF); 1 when there was a byte to fill
    int pad(bool* ff) {
        if (!nb) return 0;
        const uint8_t b = (uint8_t)((acc << (8 - nb)) | ((1u << (8 - nb)) - 1u));
        if (ff) *ff = b == 0xFF;
        byte(b);
        nb = 0;
        return 1;
    }
    void marker(int m) {                 // never stuffed
        bytes.push_back(0xFF);
        bytes.push_back((uint8_t)m);
    }
    void finish() {
        pad(nullptr);
        marker(0xD9);
    }
};

}  // namespace

// the whole scan of one frame into sink.bytes; JPEG_ENC_OK or JPEG_ENC_BAD_COEF
static int scan_frame(const int16_t* coef, const JpegGeom& g, int restart, ByteSink& sink, uint64_t* counters, uint64_t* rst_counters,
                      const jpegenc::HuffCodes* codes) {
    const jpegenc::ScanGeom sg = scan_geom(g);
    sink.bytes.reserve(g.blocks() * 16);
    uint64_t zrl = 0, no_eob = 0, rst = 0, pad_free = 0, pad_ff = 0;
    int bad = 0;
    const int nb = sg.blocks(), per = sg.per_mcu();
    for (int k = 0; k < nb; ++k) {
        if (restart > 0 && k > 0 && k % per == 0 && (k / per) % restart == 0) {
            bool ff = false;
            if (!sink.pad(&ff)) ++pad_free;
            pad_ff += ff;
            sink.marker(0xD0 + (int)(rst++ & 7));
        }
        int c, b, pb;
        jpegenc::scan_block(sg, k, restart, &c, &b, &pb);
        const int pred = pb < 0 ? 0 : coef[(size_t)pb * 64];
        const jpegenc::BlockEvents ev = jpegenc::encode_block(coef + (size_t)b * 64, pred, codes[c ? 2 : 0], codes[c ? 3 : 1], jpegenc::kStd.zigzag, sink);
        zrl += (uint64_t)ev.zrl;
        no_eob += (uint64_t)ev.no_eob;
        bad |= ev.bad;
    }
    sink.finish();
    if (counters) {
        counters[JPEG_ENC_N_ZRL] += zrl;
        counters[JPEG_ENC_N_NO_EOB] += no_eob;
        counters[JPEG_ENC_N_STUFFED] += sink.stuffed;
    }
    if (rst_counters) {
        rst_counters[JPEG_ENC_R_RST] += rst;
        rst_counters[JPEG_ENC_R_PAD_FREE] += pad_free;
        rst_counters[JPEG_ENC_R_PAD_FF] += pad_ff;
    }
    return bad ? JPEG_ENC_BAD_COEF : JPEG_ENC_OK;
}

// One frame's scan, coded with `codes`, into `out` when it fits `cap` (out is not touched otherwise) -> the status; *len: the scan's
// bytes; with JPEG_ENC_BAD_COEF 0 (the scan entries) or, `walked`, the bytes the walk made (the whole-file entries).  Every caller's
// tail: what it adds is its own precedence of the tables' status.
static int emit_scan(const int16_t* coef, const JpegGeom& g, int restart, const jpegenc::HuffCodes* codes, uint8_t* out, size_t cap, size_t* len,
                     uint64_t* counters, uint64_t* rst_counters, bool walked = false) {
    ByteSink sink;
    const int rc = scan_frame(coef, g, restart, sink, counters, rst_counters, codes);
    *len = rc == JPEG_ENC_OK || walked ? sink.bytes.size() : 0;
    if (rc != JPEG_ENC_OK) return JPEG_ENC_BAD_COEF;
    if (sink.bytes.size() > cap) return JPEG_ENC_SHORT;
    memcpy(out, sink.bytes.data(), sink.bytes.size());
    return JPEG_ENC_OK;
}

// emit_scan behind the `head` bytes of `header`, for the whole-file entries: the scan goes behind the header only when the whole file
// fits, so a short slot is left as it was.  *length: header and walked bytes, whatever the status.  cnt: a worker's counters.
static int emit_file(const int16_t* coef, const JpegGeom& g, int restart, const jpegenc::HuffCodes* codes, const uint8_t* header, size_t head,
                     uint8_t* slot, size_t slot_bytes, uint32_t* length, uint64_t* cnt) {
    const bool room = slot_bytes >= head;
    size_t len = 0;
    const int rc = emit_scan(coef, g, restart, codes, room ? slot + head : nullptr, room ? slot_bytes - head : 0, &len, cnt, cnt + JPEG_ENC_N_COUNTERS, true);
    *length = (uint32_t)(head + len);
    if (rc == JPEG_ENC_OK) memcpy(slot, header, head);     // OK means room: without it cap is 0, and a scan holds its EOI at least
    return rc;
}

int jpeg_enc_scan(const int16_t* coef, const JpegGeom& g, int restart, uint8_t* out, size_t cap, size_t* len, uint64_t* counters,
                  uint64_t* rst_counters) {
    return emit_scan(coef, g, restart, kTables.codes, out, cap, len, counters, rst_counters);
}

int jpeg_enc_gather(const int16_t* coef, const JpegGeom& g, int restart, uint32_t* hist) {
    const jpegenc::ScanGeom sg = scan_geom(g);
    memset(hist, 0, 4 * jpegenc::kHuffSymbols * sizeof(uint32_t));
    int bad = 0;
    for (int k = 0, nb = sg.blocks(); k < nb; ++k) {
        int c, b, pb;
        jpegenc::scan_block(sg, k, restart, &c, &b, &pb);
        const int pred = pb < 0 ? 0 : coef[(size_t)pb * 64];
        uint32_t* h = hist + (c ? 2 : 0) * jpegenc::kHuffSymbols;
        bad |= jpegenc::gather_block(coef + (size_t)b * 64, pred, jpegenc::kStd.zigzag, [&](int ac, int sym) { ++h[ac * jpegenc::kHuffSymbols + sym]; }).bad;
    }
    return bad ? JPEG_ENC_BAD_COEF : JPEG_ENC_OK;
}

// gather and the four tables of one frame -> JPEG_ENC_OK, JPEG_ENC_BAD_COEF or JPEG_ENC_HUFF_OVERFLOW
static int frame_tables(const int16_t* coef, const JpegGeom& g, int restart, jpegenc::HuffSpecWide* specs, jpegenc::HuffCodes* codes, uint32_t* hist_out) {
    uint32_t hist[4 * jpegenc::kHuffSymbols];
    const int rc = jpeg_enc_gather(coef, g, restart, hist);
    if (hist_out) memcpy(hist_out, hist, sizeof(hist));
    int overflow = 0;
    for (int t = 0; t < 4; ++t) overflow |= jpegenc::huff_optimal(hist + t * jpegenc::kHuffSymbols, specs[t], codes[t], nullptr) != jpegenc::HUFF_OK;
    return rc != JPEG_ENC_OK ? rc : (overflow ? JPEG_ENC_HUFF_OVERFLOW : JPEG_ENC_OK);
}

int jpeg_enc_scan_opt(const int16_t* coef, const JpegGeom& g, int restart, uint8_t* out, size_t cap, size_t* len, jpegenc::HuffSpecWide* specs,
                      uint32_t* hist, uint64_t* counters, uint64_t* rst_counters) {
    jpegenc::HuffCodes codes[4];
    *len = 0;
    const int rc = frame_tables(coef, g, restart, specs, codes, hist);
    return rc != JPEG_ENC_OK ? rc : emit_scan(coef, g, restart, codes, out, cap, len, counters, rst_counters);
}

// the four tables of a DHT-carrying header: no status, 1..256 symbols, lengths that count them
static bool specs_ok(const jpegenc::HuffSpecWide s[4]) {
    for (int t = 0; t < 4; ++t) {
        int sum = 0;
        for (int i = 0; i < 16; ++i) sum += s[t].bits[i];
        if (s[t].status != jpegenc::HUFF_OK || s[t].nvals < 1 || s[t].nvals > 256 || sum != s[t].nvals) return false;
    }
    return true;
}

namespace {

// run fn(i, counters of the worker) for i in [0, n) on up to `threads` workers; a worker's counters are the JPEG_ENC_N_* block
// with the JPEG_ENC_R_* block behind it; the workers' counters are summed into `counters` and `rst_counters`
constexpr int kWorkerCounters = JPEG_ENC_N_COUNTERS + JPEG_ENC_R_COUNTERS;
template <class F>
void parallel_frames(int n, int threads, uint64_t* counters, uint64_t* rst_counters, F fn) {
    const int allow = jpeg_thread_allowance(threads);
    const int t = allow < n ? allow : n;
    std::vector<uint64_t> local((size_t)(t < 1 ? 1 : t) * kWorkerCounters, 0);
    if (t <= 1) {
        for (int i = 0; i < n; ++i) fn(i, local.data());
    } else {
        std::atomic<int> next{0};
        std::vector<std::thread> pool;
        pool.reserve((size_t)t);
        for (int w = 0; w < t; ++w)
            pool.emplace_back([&, w] {
                for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i, local.data() + (size_t)w * kWorkerCounters);
            });
        for (auto& th : pool) th.join();
    }
    for (size_t k = 0; k < local.size(); ++k) {
        const size_t j = k % kWorkerCounters;
        if (j < JPEG_ENC_N_COUNTERS ? counters != nullptr : rst_counters != nullptr)
            (j < JPEG_ENC_N_COUNTERS ? counters[j] : rst_counters[j - JPEG_ENC_N_COUNTERS]) += local[k];
    }
}

bool frames_args_ok(const char* fn, const void* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs, JpegGeom* g) {
    *g = JpegGeom{W, H, 3, hs, vs};
    if (!frames || !idx || N < 1 || n < 1 || quality < 1 || quality > 100 || !jpeg_enc_geom_ok(*g)) {
        set_error(std::string(fn) + ": null argument, empty batch, quality outside 1..100 or unsupported geometry");
        return false;
    }
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= N) {
            set_error(std::string(fn) + ": frame index " + std::to_string(idx[i]) + " outside the " + std::to_string(N) + " frames");
            return false;
        }
    return true;
}

}  // namespace
}  // namespace tstar

// ---------------------------------------------------------------------------------------------- C ABI (include/tstar_hip.h)
using namespace tstar;

extern "C" {

// the entries without an interval forward to these with interval 0
int tstar_jpeg_encode_plan_rst(int W, int H, int hs, int vs, int n, size_t slot_bytes, int restart, size_t* out8, size_t* out2);
int tstar_jpeg_encode_header_rst(int W, int H, int quality, int hs, int vs, int restart, uint8_t* out, size_t cap, size_t* len);
int tstar_jpeg_encode_scan_host_rst(const int16_t* coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* out, size_t slot_bytes,
                                    uint32_t* lengths, int32_t* status, int threads, uint64_t* counters, uint64_t* rst_counters);
int tstar_jpeg_encode_host_rst(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                               int restart, uint8_t* out, size_t slot_bytes, uint32_t* lengths, int32_t* status, int threads,
                               uint64_t* counters, uint64_t* rst_counters);

int tstar_jpeg_encode_plan_opt(int W, int H, int hs, int vs, int n, size_t slot_bytes, int restart, int optimize, size_t* out8, size_t* out2,
                               size_t* out3) {
    if (!out8 || (optimize != 0 && optimize != 1)) { set_error("tstar_jpeg_encode_plan_opt: null argument or optimize outside 0 / 1"); return 1; }
    const JpegEncPlan p = plan_jpeg_encode(JpegGeom{W, H, 3, hs, vs}, n, slot_bytes, restart, optimize);
    if (p.error) { set_error(std::string("tstar_jpeg_encode_plan_opt: ") + p.error); return 1; }
    if (out2) { out2[0] = (size_t)p.restart; out2[1] = p.markers; }
    if (out3) { out3[0] = (size_t)p.optimize; out3[1] = p.off_hist; out3[2] = p.off_codes; }
    out8[0] = p.blocks; out8[1] = p.coef_bytes; out8[2] = p.max_scan_bytes; out8[3] = p.header_bytes; out8[4] = p.workspace_bytes;
    out8[5] = p.block_wgs; out8[6] = p.entropy_wgs_x; out8[7] = p.stuff_wgs_x;
    return 0;
}

int tstar_jpeg_huff_optimal(const uint32_t* freq, uint8_t* spec, uint16_t* code, uint8_t* len, int32_t* steps) {
    if (!freq || !spec) { set_error("tstar_jpeg_huff_optimal: null argument"); return 1; }
    uint64_t total = 0;
    for (int i = 0; i < 256; ++i) total += freq[i];
    if (total > jpegenc::kHuffMaxCount) { set_error("tstar_jpeg_huff_optimal: the counts sum to more than 1000000000"); return 1; }
    jpegenc::HuffSpecWide s;
    jpegenc::HuffCodes h;
    int n = 0;
    jpegenc::huff_optimal(freq, s, h, &n);
    memcpy(spec, &s, sizeof(s));
    if (code) memcpy(code, h.code, sizeof(h.code));
    if (len) memcpy(len, h.len, sizeof(h.len));
    if (steps) *steps = n;
    return 0;
}

int tstar_jpeg_encode_header_opt(int W, int H, int quality, int hs, int vs, int restart, const uint8_t* specs, uint8_t* out, size_t cap,
                                 size_t* len) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!out || !len || !specs || quality < 1 || quality > 100 || !jpeg_enc_geom_ok(g) || !jpeg_enc_restart_ok(restart)) {
        set_error("tstar_jpeg_encode_header_opt: null argument, quality outside 1..100, unsupported geometry or restart interval outside 0..65535");
        return 1;
    }
    jpegenc::HuffSpecWide s[4];
    memcpy(s, specs, sizeof(s));
    if (!specs_ok(s)) {
        set_error("tstar_jpeg_encode_header_opt: a table without symbols, with a status, or whose lengths do not count its symbols");
        return 1;
    }
    uint8_t buf[kJpegEncHeaderOptMax + kJpegEncDriBytes];
    *len = jpeg_enc_header_opt(g, quality, restart, s, buf);
    if (cap < *len) { set_error("tstar_jpeg_encode_header_opt: the buffer is shorter than the header"); return 4; }
    memcpy(out, buf, *len);
    return 0;
}

int tstar_jpeg_encode_scan_host_opt(const int16_t* coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* out, size_t slot_bytes,
                                    uint32_t* lengths, int32_t* status, uint8_t* specs, uint32_t* hist, int threads, uint64_t* counters,
                                    uint64_t* rst_counters) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!coef || !lengths || !status || !specs || (!out && slot_bytes) || n < 1 || !jpeg_enc_geom_ok(g) || !jpeg_enc_restart_ok(restart)) {
        set_error("tstar_jpeg_encode_scan_host_opt: null argument, empty batch, unsupported geometry or restart interval outside 0..65535");
        return 1;
    }
    const size_t per = g.blocks() * 64;
    parallel_frames(n, threads, counters, rst_counters, [&](int i, uint64_t* cnt) {
        size_t len = 0;
        jpegenc::HuffSpecWide s[4];
        status[i] = jpeg_enc_scan_opt(coef + per * (size_t)i, g, restart, out + slot_bytes * (size_t)i, slot_bytes, &len, s,
                                      hist ? hist + (size_t)i * 4 * jpegenc::kHuffSymbols : nullptr, cnt, cnt + JPEG_ENC_N_COUNTERS);
        memcpy(specs + (size_t)i * sizeof(s), s, sizeof(s));
        lengths[i] = (uint32_t)len;
    });
    return 0;
}

// Shared tables, host twin of tstar_jpeg_encode_scan_grp.  stages as there: 1 the frames' counts and their sums per group (into
// group_hist), 2 the groups' tables from group_hist AS IT IS (a caller may have put counts of its own there), 4 the scans.
int tstar_jpeg_encode_scan_host_grp(const int16_t* coef, int n, int W, int H, int hs, int vs, int restart, const int32_t* group,
                                    int n_groups, int stages, uint32_t* group_hist, uint8_t* specs, uint8_t* out, size_t slot_bytes,
                                    uint32_t* lengths, int32_t* status, int threads) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!coef || !group || !group_hist || !specs || n < 1 || stages < 1 || stages > 7 || !jpeg_enc_geom_ok(g) || !jpeg_enc_restart_ok(restart) ||
        ((stages & 4) && (!lengths || !status || (!out && slot_bytes)))) {
        set_error("tstar_jpeg_encode_scan_host_grp: null argument, empty batch, stages outside 1..7, unsupported geometry or restart interval outside 0..65535");
        return 1;
    }
    std::vector<int32_t> span((size_t)2 * (n_groups > 0 ? n_groups : 1));
    const char* bad = jpeg_enc_groups_check(group, n, n_groups, g.blocks(), span.data());
    if (bad) { set_error(std::string("tstar_jpeg_encode_scan_host_grp: ") + bad); return 1; }
    constexpr size_t kH = 4 * jpegenc::kHuffSymbols;
    const size_t per = g.blocks() * 64;
    if (stages & 1) {
        std::vector<uint32_t> hist((size_t)n * kH, 0);
        parallel_frames(n, threads, nullptr, nullptr, [&](int i, uint64_t*) {
            if (group[i] >= 0) jpeg_enc_gather(coef + per * (size_t)i, g, restart, hist.data() + (size_t)i * kH);
        });
        for (int q = 0; q < n_groups; ++q) {                          // the frames of a group in order: the sums are exact
            uint32_t* gh = group_hist + (size_t)q * kH;
            memset(gh, 0, kH * sizeof(uint32_t));
            for (int f = span[2 * q]; f < span[2 * q + 1]; ++f)
                if (group[f] == q)
                    for (size_t i = 0; i < kH; ++i) gh[i] += hist[(size_t)f * kH + i];
        }
    }
    if (!(stages & 6)) return 0;
    std::vector<jpegenc::HuffCodes> codes((size_t)4 * n_groups);
    std::vector<jpegenc::HuffSpecWide> sp((size_t)4 * n_groups);
    if (stages & 2) {
        for (int q = 0; q < 4 * n_groups; ++q)
            jpegenc::huff_optimal(group_hist + (size_t)(q / 4) * kH + (size_t)(q % 4) * jpegenc::kHuffSymbols, sp[q], codes[q], nullptr);
        memcpy(specs, sp.data(), sp.size() * sizeof(jpegenc::HuffSpecWide));
    } else {                                                          // the scans alone: with the tables the caller kept
        memcpy(sp.data(), specs, sp.size() * sizeof(jpegenc::HuffSpecWide));
        for (int q = 0; q < 4 * n_groups; ++q) jpegenc::huff_assign_codes(sp[q], codes[q]);
    }
    if (!(stages & 4)) return 0;
    parallel_frames(n, threads, nullptr, nullptr, [&](int i, uint64_t*) {
        lengths[i] = 0;
        status[i] = JPEG_ENC_HUFF_OVERFLOW;
        const int q = group[i];
        if (q < 0) return;
        bool overflow = false;
        for (int t = 0; t < 4; ++t) overflow |= sp[(size_t)4 * q + t].status != jpegenc::HUFF_OK;
        // a group whose tables have a status is walked too, into no slot: a coefficient without a code comes before the tables' word,
        // as per frame
        size_t len = 0;
        const int rc = emit_scan(coef + per * (size_t)i, g, restart, codes.data() + (size_t)4 * q, overflow ? nullptr : out + slot_bytes * (size_t)i,
                                 overflow ? 0 : slot_bytes, &len, nullptr, nullptr);
        if (overflow && rc != JPEG_ENC_BAD_COEF) return;
        lengths[i] = (uint32_t)(len > 0xffffffffull ? 0xffffffffull : len);
        status[i] = rc;
    });
    return 0;
}

// group i32 [n] -> span i32 [n_groups][2]: what the device entry wants next to the groups (and checks)
int tstar_jpeg_encode_group_spans(const int32_t* group, int n, int n_groups, int W, int H, int hs, int vs, int32_t* span) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!span || !jpeg_enc_geom_ok(g)) { set_error("tstar_jpeg_encode_group_spans: null argument or unsupported geometry"); return 1; }
    const char* bad = jpeg_enc_groups_check(group, n, n_groups, g.blocks(), span);
    if (bad) { set_error(std::string("tstar_jpeg_encode_group_spans: ") + bad); return 1; }
    return 0;
}

int tstar_jpeg_encode_group_frames(int W, int H, int hs, int vs) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!jpeg_enc_geom_ok(g)) { set_error("tstar_jpeg_encode_group_frames: unsupported geometry"); return 0; }
    return jpeg_enc_group_frames(g.blocks());
}

int tstar_jpeg_encode_header_tables_opt(int W, int H, const uint16_t* quant, int hs, int vs, int restart, const uint8_t* specs, uint8_t* out,
                                        size_t cap, size_t* len) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!out || !len || !quant || !specs || !jpeg_enc_geom_ok(g) || !jpeg_enc_restart_ok(restart)) {
        set_error("tstar_jpeg_encode_header_tables_opt: null argument, unsupported geometry or restart interval outside 0..65535");
        return 1;
    }
    for (int k = 0; k < 192; ++k)
        if (quant[k] < 1) { set_error("tstar_jpeg_encode_header_tables_opt: a quantisation value of 0"); return 1; }
    jpegenc::HuffSpecWide s[4];
    memcpy(s, specs, sizeof(s));
    if (!specs_ok(s)) {
        set_error("tstar_jpeg_encode_header_tables_opt: a table without symbols, with a status, or whose lengths do not count its symbols");
        return 1;
    }
    uint8_t buf[kJpegEncHeaderTablesOptMax];
    *len = jpeg_enc_header_tables_opt(g, quant, restart, s, buf);
    if (cap < *len) { set_error("tstar_jpeg_encode_header_tables_opt: the buffer is shorter than the header"); return 4; }
    memcpy(out, buf, *len);
    return 0;
}

int tstar_jpeg_encode_host_opt(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                               int restart, uint8_t* out, size_t slot_bytes, uint32_t* lengths, int32_t* status, int threads,
                               uint64_t* counters, uint64_t* rst_counters) {
    JpegGeom g;
    if (!frames_args_ok("tstar_jpeg_encode_host_opt", frames, N, H, W, idx, n, quality, hs, vs, &g)) return 1;
    if (!lengths || !status || (!out && slot_bytes)) { set_error("tstar_jpeg_encode_host_opt: null argument"); return 1; }
    if (!jpeg_enc_restart_ok(restart)) { set_error("tstar_jpeg_encode_host_opt: restart interval outside 0..65535 MCUs"); return 1; }
    uint16_t q[192];
    jpeg_enc_quant(quality, q);
    const size_t per = g.blocks() * 64, frame = (size_t)W * H * 3;
    parallel_frames(n, threads, counters, rst_counters, [&](int i, uint64_t* cnt) {
        std::vector<int16_t> coef(per);
        jpeg_enc_blocks(frames + frame * (size_t)idx[i], g, q, coef.data(), cnt + JPEG_ENC_N_DUMMY_RIGHT);
        jpegenc::HuffSpecWide specs[4];
        jpegenc::HuffCodes codes[4];
        lengths[i] = 0;
        status[i] = frame_tables(coef.data(), g, restart, specs, codes, nullptr);
        if (status[i] != JPEG_ENC_OK) return;
        uint8_t header[kJpegEncHeaderOptMax + kJpegEncDriBytes];
        const size_t head = write_header(g, q, restart, specs, header);
        status[i] = emit_file(coef.data(), g, restart, codes, header, head, out + slot_bytes * (size_t)i, slot_bytes, &lengths[i], cnt);
    });
    return 0;
}

int tstar_jpeg_encode_plan(int W, int H, int hs, int vs, int n, size_t slot_bytes, size_t* out8) {
    return tstar_jpeg_encode_plan_rst(W, H, hs, vs, n, slot_bytes, 0, out8, nullptr);
}

int tstar_jpeg_encode_plan_rst(int W, int H, int hs, int vs, int n, size_t slot_bytes, int restart, size_t* out8, size_t* out2) {
    if (!out8) { set_error("tstar_jpeg_encode_plan: null argument"); return 1; }
    const JpegEncPlan p = plan_jpeg_encode(JpegGeom{W, H, 3, hs, vs}, n, slot_bytes, restart);
    if (p.error) { set_error(std::string("tstar_jpeg_encode_plan: ") + p.error); return 1; }
    if (out2) { out2[0] = (size_t)p.restart; out2[1] = p.markers; }
    out8[0] = p.blocks; out8[1] = p.coef_bytes; out8[2] = p.max_scan_bytes; out8[3] = p.header_bytes; out8[4] = p.workspace_bytes;
    out8[5] = p.block_wgs; out8[6] = p.entropy_wgs_x; out8[7] = p.stuff_wgs_x;
    return 0;
}

int tstar_jpeg_encode_header(int W, int H, int quality, int hs, int vs, uint8_t* out, size_t cap, size_t* len) {
    return tstar_jpeg_encode_header_rst(W, H, quality, hs, vs, 0, out, cap, len);
}

int tstar_jpeg_encode_header_rst(int W, int H, int quality, int hs, int vs, int restart, uint8_t* out, size_t cap, size_t* len) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!out || !len || quality < 1 || quality > 100 || !jpeg_enc_geom_ok(g) || !jpeg_enc_restart_ok(restart)) {
        set_error("tstar_jpeg_encode_header: null argument, quality outside 1..100, unsupported geometry or restart interval outside 0..65535");
        return 1;
    }
    *len = (size_t)jpeg_enc_header_bytes(restart);
    if (cap < *len) { set_error("tstar_jpeg_encode_header: the buffer is shorter than the header"); return 4; }
    jpeg_enc_header(g, quality, restart, out);
    return 0;
}

int tstar_jpeg_encode_header_tables(int W, int H, const uint16_t* quant, int hs, int vs, int restart, uint8_t* out, size_t cap, size_t* len) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!out || !len || !quant || !jpeg_enc_geom_ok(g) || !jpeg_enc_restart_ok(restart)) {
        set_error("tstar_jpeg_encode_header_tables: null argument, unsupported geometry or restart interval outside 0..65535");
        return 1;
    }
    for (int k = 0; k < 192; ++k)
        if (quant[k] == 0) { set_error("tstar_jpeg_encode_header_tables: a quantisation value of 0"); return 1; }
    uint8_t buf[kJpegEncHeaderTablesMax];
    *len = jpeg_enc_header_tables(g, quant, restart, buf);
    if (cap < *len) { set_error("tstar_jpeg_encode_header_tables: the buffer is shorter than the header"); return 4; }
    memcpy(out, buf, *len);
    return 0;
}

int tstar_jpeg_encode_blocks_host(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                                  int16_t* coef, uint16_t* quant, int threads, uint64_t* counters) {
    JpegGeom g;
    if (!frames_args_ok("tstar_jpeg_encode_blocks_host", frames, N, H, W, idx, n, quality, hs, vs, &g)) return 1;
    if (!coef) { set_error("tstar_jpeg_encode_blocks_host: null argument"); return 1; }
    uint16_t q[192];
    jpeg_enc_quant(quality, q);
    if (quant) memcpy(quant, q, sizeof(q));
    const size_t per = g.blocks() * 64, frame = (size_t)W * H * 3;
    parallel_frames(n, threads, counters, nullptr, [&](int i, uint64_t* cnt) {
        jpeg_enc_blocks(frames + frame * (size_t)idx[i], g, q, coef + per * (size_t)i, cnt + JPEG_ENC_N_DUMMY_RIGHT);
    });
    return 0;
}

int tstar_jpeg_encode_scan_host(const int16_t* coef, int n, int W, int H, int hs, int vs, uint8_t* out, size_t slot_bytes,
                                uint32_t* lengths, int32_t* status, int threads, uint64_t* counters) {
    return tstar_jpeg_encode_scan_host_rst(coef, n, W, H, hs, vs, 0, out, slot_bytes, lengths, status, threads, counters, nullptr);
}

int tstar_jpeg_encode_scan_host_rst(const int16_t* coef, int n, int W, int H, int hs, int vs, int restart, uint8_t* out, size_t slot_bytes,
                                    uint32_t* lengths, int32_t* status, int threads, uint64_t* counters, uint64_t* rst_counters) {
    const JpegGeom g{W, H, 3, hs, vs};
    if (!coef || !lengths || !status || (!out && slot_bytes) || n < 1 || !jpeg_enc_geom_ok(g) || !jpeg_enc_restart_ok(restart)) {
        set_error("tstar_jpeg_encode_scan_host: null argument, empty batch, unsupported geometry or restart interval outside 0..65535");
        return 1;
    }
    const size_t per = g.blocks() * 64;
    parallel_frames(n, threads, counters, rst_counters, [&](int i, uint64_t* cnt) {
        size_t len = 0;
        status[i] = jpeg_enc_scan(coef + per * (size_t)i, g, restart, out + slot_bytes * (size_t)i, slot_bytes, &len, cnt,
                                  cnt + JPEG_ENC_N_COUNTERS);
        lengths[i] = (uint32_t)len;
    });
    return 0;
}

int tstar_jpeg_encode_host(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                           uint8_t* out, size_t slot_bytes, uint32_t* lengths, int32_t* status, int threads, uint64_t* counters) {
    return tstar_jpeg_encode_host_rst(frames, N, H, W, idx, n, quality, hs, vs, 0, out, slot_bytes, lengths, status, threads, counters, nullptr);
}

int tstar_jpeg_encode_host_rst(const uint8_t* frames, int N, int H, int W, const int32_t* idx, int n, int quality, int hs, int vs,
                               int restart, uint8_t* out, size_t slot_bytes, uint32_t* lengths, int32_t* status, int threads,
                               uint64_t* counters, uint64_t* rst_counters) {
    JpegGeom g;
    if (!frames_args_ok("tstar_jpeg_encode_host", frames, N, H, W, idx, n, quality, hs, vs, &g)) return 1;
    if (!lengths || !status || (!out && slot_bytes)) { set_error("tstar_jpeg_encode_host: null argument"); return 1; }
    if (!jpeg_enc_restart_ok(restart)) { set_error("tstar_jpeg_encode_host: restart interval outside 0..65535 MCUs"); return 1; }
    uint16_t q[192];
    jpeg_enc_quant(quality, q);
    uint8_t header[kJpegEncHeaderBytes + kJpegEncDriBytes];
    const size_t head = (size_t)jpeg_enc_header_bytes(restart);
    jpeg_enc_header(g, quality, restart, header);
    const size_t per = g.blocks() * 64, frame = (size_t)W * H * 3;
    parallel_frames(n, threads, counters, rst_counters, [&](int i, uint64_t* cnt) {
        std::vector<int16_t> coef(per);
        jpeg_enc_blocks(frames + frame * (size_t)idx[i], g, q, coef.data(), cnt + JPEG_ENC_N_DUMMY_RIGHT);
        status[i] = emit_file(coef.data(), g, restart, kTables.codes, header, head, out + slot_bytes * (size_t)i, slot_bytes, &lengths[i], cnt);
    });
    return 0;
}

}  // extern "C"
