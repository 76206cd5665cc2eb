// Lossless re-coding of baseline JPEG frames with a restart interval: the records and checks of the stage that ASSEMBLES a piece
// of a new arena from the scans the encoder's scan stage left in fixed-size slots.  Shared by the kernels (jpeg_recode.hip) and
// their host mirror (jpeg_recode_host.cpp): same checks, same words.  HIP-free.
//
// A PIECE is m frames of one geometry that were entropy-decoded together (the SOURCE batch: their files end to end in one byte
// buffer, with the planner's quant rows, frame records and segments).  Frame j of the piece is either
//   re-coded  header hdr (one of the piece's few distinct headers: SOI .. SOS with the source's quantisation tables, the standard
//             Huffman tables and DRI) followed by the scan in slot j, or
//   kept      its source bytes as they are, with the source's records (a frame the decoder or the encoder does not vouch for).
// The output is the frames end to end (the arena packs files without padding) and ONE record buffer (recode_layout):
//   off u64 [m + 1] (off[m]: the piece's bytes) | len u32 [m] | quant u16 [m][192] | frame records [m] | segments [n_segments]
// which is what jpeg_plan_segments says about the output bytes: a re-coded frame has one segment per restart interval, begin
// behind the header / the previous marker, end at the marker's FF (the EOI's for the last), first_mcu = k * restart.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_entropy_core.h"

namespace tstar {
namespace jpegrec {

enum { RECODE_NEW = 0, RECODE_KEPT = 1 };
constexpr uint32_t kHeaderPitch = 1024;      // bytes of a row of the header table (the longest header: three 16-bit tables, DRI: 890)
// Rows of the _opt entries: a header with tables of its own is up to 177 + 4 * 277 + 14 + 6 = 1305 bytes, a third quantisation table
// and 16-bit entries add 69 + 3 * 64.  Their pitch is an argument: a multiple of 16 that holds the longest header of the piece.
constexpr uint32_t kHeaderPitchOpt = 1568;

// One frame of a piece, written by the host once the scan stage's lengths and statuses are known.
struct RecodeDesc {
    uint32_t kind;               // RECODE_NEW / RECODE_KEPT
    uint32_t hdr;                // RECODE_NEW: row of the header table
    uint32_t src;                // frame of the source batch: its quant row; RECODE_KEPT: its bytes and records too (the scan is in slot j)
    uint32_t src_off, src_len;   // RECODE_KEPT: the frame's bytes in the source batch
    int32_t table_set;           // of the output's frame record (-1: a kept frame the planner routed to the host)
    uint32_t first_segment;      // of the output's segment list (prefix sum of n_segments)
    uint32_t n_segments;         // RECODE_NEW: ceil(MCUs / restart); RECODE_KEPT: the source frame record's count
};
static_assert(sizeof(RecodeDesc) == 32, "the descriptor is part of the C ABI (include/tstar_hip.h)");

struct Source {                  // the batch the frames were decoded from
    const uint8_t* bytes;
    uint64_t total_bytes;
    const uint16_t* quant;       // [n_frames][192]
    const JpegFrameDesc* frames;
    const JpegSegment* segments; // begin / end count from the start of `bytes`
    uint32_t n_frames, n_segments;
};

struct Scans {                   // what the scan stage wrote
    const uint8_t* headers;      // [n_headers][header_pitch]
    const uint32_t* header_len;  // [n_headers]
    uint32_t n_headers;
    uint32_t header_pitch;       // kHeaderPitch for the entries without an argument for it
    const uint8_t* slots;        // [m][slot_bytes], 16-byte aligned, slot_bytes a multiple of 16
    uint64_t slot_bytes;
    const uint32_t* scan_len;    // [m]
    uint32_t restart, n_mcu;     // MCUs per interval (0, _opt entries only: none, the frame is one segment), MCUs per frame
};

struct Records {                 // views into the record buffer
    uint64_t* off;
    uint32_t* len;
    uint16_t* quant;
    JpegFrameDesc* frames;
    JpegSegment* segments;
    uint64_t off_at, len_at, quant_at, frames_at, segments_at, nbytes;
    uint32_t m, n_segments;
};

struct Output {
    uint8_t* bytes;
    uint64_t cap;                // no store at or behind it
};

TSTAR_JPEG_HD inline uint64_t round16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// Offsets of the parts of the record buffer -> false when the arguments are not a piece.
inline bool recode_layout(int m, int n_segments, Records* r) {
    if (m <= 0 || m > 65535 || n_segments < 0) return false;
    r->m = (uint32_t)m; r->n_segments = (uint32_t)n_segments;
    r->off_at = 0;
    r->len_at = round16((uint64_t)(m + 1) * 8);
    r->quant_at = r->len_at + round16((uint64_t)m * 4);
    r->frames_at = r->quant_at + (uint64_t)m * 384;
    r->segments_at = r->frames_at + (uint64_t)m * sizeof(JpegFrameDesc);
    r->nbytes = round16(r->segments_at + (uint64_t)n_segments * sizeof(JpegSegment));
    return true;
}
inline void recode_views(uint8_t* buf, Records* r) {
    r->off = reinterpret_cast<uint64_t*>(buf + r->off_at);
    r->len = reinterpret_cast<uint32_t*>(buf + r->len_at);
    r->quant = reinterpret_cast<uint16_t*>(buf + r->quant_at);
    r->frames = reinterpret_cast<JpegFrameDesc*>(buf + r->frames_at);
    r->segments = reinterpret_cast<JpegSegment*>(buf + r->segments_at);
}

TSTAR_JPEG_HD inline uint32_t recode_intervals(uint32_t n_mcu, uint32_t restart) { return restart ? (n_mcu + restart - 1) / restart : 1u; }

// What the host checks before any launch, on ITS copy of the descriptor: kinds, rows, source frames, segment counts and the exact
// segment prefix.  nullptr, or what is wrong.
inline const char* recode_check(const RecodeDesc* d, const Records& r, const Source& s, const Scans& c) {
    uint64_t seg = 0;
    for (uint32_t j = 0; j < r.m; ++j) {
        if (d[j].kind != RECODE_NEW && d[j].kind != RECODE_KEPT) return "a frame is neither re-coded nor kept";
        if (d[j].src >= s.n_frames) return "a source frame outside the batch";
        if (d[j].kind == RECODE_NEW) {
            if (d[j].hdr >= c.n_headers) return "a header row outside the table";
            if (d[j].n_segments != recode_intervals(c.n_mcu, c.restart)) return "a re-coded frame's segment count is not its interval count";
            if (d[j].table_set < 0) return "a re-coded frame without a table set";
        } else {
            if ((uint64_t)d[j].src_off + d[j].src_len > s.total_bytes) return "a kept frame's bytes leave the source batch";
            if (d[j].table_set < 0 && d[j].n_segments) return "a kept frame without a table set has no segments";
        }
        if (d[j].first_segment != seg) return "the segment prefix does not match the counts";
        seg += d[j].n_segments;
        if (seg > r.n_segments) return "more segments than the record buffer holds";
    }
    if (seg != r.n_segments) return "the segments do not fill the list exactly";
    return nullptr;
}

// The one place that checks the arguments of the launcher and of its mirror and fills the views -> nullptr, or what is wrong.
inline const char* recode_args(const void* h_desc, int m, int n_segments, const uint8_t* headers, const uint32_t* header_len, int n_headers,
                               const uint8_t* slots, size_t slot_bytes, const uint32_t* scan_len, int restart, int n_mcu,
                               const uint8_t* src_bytes, size_t src_total, const uint16_t* src_quant, const void* src_frames,
                               const void* src_segments, int n_src_frames, int n_src_segments, uint8_t* rec, size_t rec_bytes, uint8_t* out,
                               size_t out_bytes, Source* s, Scans* c, Records* r, Output* o, size_t header_pitch) {
    if (!h_desc || !headers || !header_len || !slots || !scan_len || !src_bytes || !src_quant || !src_frames || !src_segments || !rec || !out)
        return "null argument";
    if (!recode_layout(m, n_segments, r)) return "m outside 1..65535 or n_segments < 0";
    if (rec_bytes < r->nbytes) return "the record buffer is shorter than tstar_jpeg_recode_layout says";
    if (n_headers <= 0 || n_src_frames <= 0 || n_src_segments < 0) return "no header or an empty source batch";
    if (restart < 0 || restart > 65535 || n_mcu < 1) return "restart interval outside 0..65535 or no MCU";
    if (header_pitch < 16 || header_pitch % 16 || header_pitch > 65536) return "header_pitch must be a multiple of 16 in 16..65536";
    if (slot_bytes < 16 || slot_bytes % 16 || slot_bytes >= (1ull << 31)) return "slot_bytes must be a multiple of 16 in 16..2^31-1";
    if (src_total >= (1ull << 32) || out_bytes >= (1ull << 32)) return "a piece addresses its bytes with 32 bits";
    if ((uintptr_t)rec % 16 || (uintptr_t)slots % 16 || (uintptr_t)headers % 16 || (uintptr_t)src_quant % 16 || (uintptr_t)h_desc % 4 ||
        (uintptr_t)header_len % 4 || (uintptr_t)scan_len % 4 || (uintptr_t)src_frames % 4 || (uintptr_t)src_segments % 4)
        return "misaligned buffer";
    s->bytes = src_bytes; s->total_bytes = src_total; s->quant = src_quant; s->frames = (const JpegFrameDesc*)src_frames;
    s->segments = (const JpegSegment*)src_segments; s->n_frames = (uint32_t)n_src_frames; s->n_segments = (uint32_t)n_src_segments;
    c->headers = headers; c->header_len = header_len; c->n_headers = (uint32_t)n_headers; c->header_pitch = (uint32_t)header_pitch; c->slots = slots; c->slot_bytes = slot_bytes;
    c->scan_len = scan_len; c->restart = (uint32_t)restart; c->n_mcu = (uint32_t)n_mcu;
    recode_views(rec, r);
    o->bytes = out; o->cap = out_bytes;
    return recode_check((const RecodeDesc*)h_desc, *r, *s, *c);
}

// The device's own check of frame j's descriptor against what lies in device memory -> the bytes the frame takes in the output,
// 0 for a frame that fails (it gets no bytes, a record without a table set and segments that name no frame).
TSTAR_JPEG_HD inline bool recode_frame_ok(const RecodeDesc& d, uint32_t j, const Source& s, const Scans& c, const Records& r) {
    if (d.src >= s.n_frames || (uint64_t)d.first_segment + d.n_segments > r.n_segments) return false;
    if (d.kind == RECODE_NEW) {
        if (d.hdr >= c.n_headers || c.header_len[d.hdr] > c.header_pitch) return false;
        const uint32_t n = c.scan_len[j];
        return n >= 2 && n <= c.slot_bytes && d.n_segments == recode_intervals(c.n_mcu, c.restart);
    }
    if (d.kind != RECODE_KEPT || (uint64_t)d.src_off + d.src_len > s.total_bytes) return false;
    const JpegFrameDesc f = s.frames[d.src];
    if (d.n_segments == 0) return true;
    return f.n_segments >= 0 && (uint32_t)f.n_segments == d.n_segments && f.first_segment >= 0 &&
           (uint64_t)f.first_segment + d.n_segments <= s.n_segments;
}
TSTAR_JPEG_HD inline uint32_t recode_frame_len(const RecodeDesc& d, uint32_t j, const Source& s, const Scans& c, const Records& r) {
    if (!recode_frame_ok(d, j, s, c, r)) return 0;
    return d.kind == RECODE_NEW ? c.header_len[d.hdr] + c.scan_len[j] : d.src_len;
}

// Frame j's record.
TSTAR_JPEG_HD inline JpegFrameDesc recode_frame_record(const RecodeDesc& d, bool ok) {
    JpegFrameDesc f;
    f.table_set = ok ? d.table_set : -1;
    f.first_segment = ok && d.table_set >= 0 ? (int32_t)d.first_segment : 0;
    f.n_segments = ok && d.table_set >= 0 ? (int32_t)d.n_segments : 0;
    f.reserved = 0;
    return f;
}

// Segment i of kept frame j: the source's, moved with the frame from src_off to `at` of the output.
TSTAR_JPEG_HD inline JpegSegment recode_kept_segment(const RecodeDesc& d, const Source& s, uint32_t j, uint32_t i, uint32_t at, bool ok) {
    JpegSegment g;
    g.frame = 0xffffffffu; g.begin = 0; g.end = 0; g.first_mcu = 0; g.n_mcu = 0; g.last = 0;
    if (!ok) return g;
    const JpegSegment q = s.segments[(uint32_t)s.frames[d.src].first_segment + i];
    if (q.begin > q.end || q.begin < d.src_off || q.end > d.src_off + d.src_len) return g;
    g.frame = j; g.begin = q.begin - d.src_off + at; g.end = q.end - d.src_off + at;
    g.first_mcu = q.first_mcu; g.n_mcu = q.n_mcu; g.last = q.last;
    return g;
}

// Interval i of re-coded frame j without its byte range (the marker pass fills begin and end).
TSTAR_JPEG_HD inline JpegSegment recode_new_segment(const Scans& c, uint32_t j, uint32_t i, uint32_t n_intervals) {
    JpegSegment g;
    g.frame = j; g.begin = 0; g.end = 0;
    g.first_mcu = i * c.restart;
    g.n_mcu = i + 1 < n_intervals ? c.restart : c.n_mcu - g.first_mcu;
    g.last = i + 1 == n_intervals ? 1u : 0u;
    return g;
}

// In stuffed entropy-coded data an FF followed by D0..D7 is a restart marker and nothing else.
TSTAR_JPEG_HD inline bool recode_is_marker(uint8_t b0, uint8_t b1) { return b0 == 0xFF && (b1 & 0xF8) == 0xD0; }

}  // namespace jpegrec

// Host mirror of the launcher (jpeg_recode_host.cpp): the same record buffer and output bytes, word for word.
void jpeg_recode_assemble_host(const jpegrec::RecodeDesc* desc, const jpegrec::Source& s, const jpegrec::Scans& c, const jpegrec::Records& r,
                               const jpegrec::Output& o);

}  // namespace tstar
