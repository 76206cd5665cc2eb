// Compressed-resident JPEG store: the records of the ARENA (every wanted frame of a file, compressed, on the device) and the
// code that turns a list of arena frames into one batch buffer for the entropy launchers.  Shared by the kernel
// (jpeg_resident.hip) and its host mirror (jpeg_resident_host.cpp): same checks, same words.  HIP-free.
//
// Arena, per frame e of n_entries: off[e] (u64: the arena may exceed 4 GiB), len[e], quant row [192], a frame record whose
// first_segment indexes the arena's segment list, and segments whose begin / end count from the frame's first byte.
// Batch buffer for m frames (gather_layout): the frames' bytes end to end, each at a 16-byte-aligned start and padded with zeros
// to the next one | quant rows [m][192] | frame records [m] | segments [n_segments]; every part 16-byte aligned.  This is what
// the entropy launchers take (the table sets stay where they are: one list for the whole file).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_entropy_core.h"

namespace tstar {
namespace jpegres {

// One frame of a fetch, written by the host from the counts it kept at open.
struct GatherDesc {
    uint32_t id;                 // arena frame
    uint32_t dst;                // byte offset of the frame in the batch buffer (multiple of 16)
    uint32_t len;                // its bytes (the arena's len[id])
    uint32_t first_segment;      // of the batch's segment list (prefix sum of n_segments)
    uint32_t n_segments;         // the arena frame record's count
    uint32_t reserved;
};
static_assert(sizeof(GatherDesc) == 24, "the descriptor is part of the C ABI (include/tstar_hip.h)");

struct Arena {
    const uint8_t* bytes;
    uint64_t total_bytes;
    const uint64_t* off;
    const uint32_t* len;
    const uint16_t* quant;       // [n_entries][192]
    const JpegFrameDesc* frames;
    const JpegSegment* segments;
    uint32_t n_entries, n_segments;
};

struct Batch {
    uint8_t* buf;
    uint64_t total_bytes;        // of the byte part
    uint64_t quant_at, frames_at, segments_at, nbytes;
    uint32_t m, n_segments;
};

TSTAR_JPEG_HD inline uint64_t round16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// Offsets of the parts behind total_bytes bytes of frames -> false when the arguments are not a batch.
inline bool gather_layout(uint64_t total_bytes, int m, int n_segments, Batch* b) {
    if (m <= 0 || n_segments < 0 || total_bytes >= (1ull << 32) || total_bytes % 16) return false;
    b->total_bytes = total_bytes;
    b->m = (uint32_t)m; b->n_segments = (uint32_t)n_segments;
    b->quant_at = total_bytes;
    b->frames_at = b->quant_at + (uint64_t)m * 384;
    b->segments_at = b->frames_at + (uint64_t)m * sizeof(JpegFrameDesc);
    b->nbytes = round16(b->segments_at + (uint64_t)n_segments * sizeof(JpegSegment));
    return true;
}

// What the host checks before any launch: every id names an arena frame, the frames tile the byte part in order at aligned
// starts, the segment prefix is exact.  nullptr, or what is wrong.
inline const char* gather_check(const GatherDesc* d, int m, uint32_t n_entries, const Batch& b) {
    uint64_t at = 0, seg = 0;
    for (int j = 0; j < m; ++j) {
        if (d[j].id >= n_entries) return "a frame id outside the arena";
        if (d[j].dst != at) return "frames are not end to end at 16-byte-aligned starts";
        at += round16(d[j].len);
        if (at > b.total_bytes) return "the frames do not fit the byte part of the batch";
        if (d[j].first_segment != seg) return "the segment prefix does not match the counts";
        seg += d[j].n_segments;
        if (seg > b.n_segments) return "more segments than the batch holds";
    }
    if (at != b.total_bytes || seg != b.n_segments) return "the frames or their segments do not fill the batch exactly";
    return nullptr;
}

// The one place that checks the arguments of the launcher and of its mirror and fills the two views -> nullptr, or what is
// wrong.  h_desc is the host's copy of the descriptor (the launcher reads the device's copy of the same words).
inline const char* gather_args(const uint8_t* arena, size_t arena_bytes, const uint64_t* off, const uint32_t* len, const uint16_t* quant,
                               const void* frames, const void* segments, int n_entries, int n_arena_segments, const void* h_desc, int m,
                               size_t total_bytes, int n_segments, uint8_t* batch, size_t batch_bytes, Arena* a, Batch* b) {
    if (!arena || !off || !len || !quant || !frames || !segments || !h_desc || !batch) return "null argument";
    if (n_entries <= 0 || n_arena_segments < 0) return "empty arena";
    if (!gather_layout(total_bytes, m, n_segments, b))
        return "m <= 0, n_segments < 0, or total_bytes no multiple of 16 below 2^32";
    if (batch_bytes < b->nbytes) return "the batch buffer is shorter than tstar_jpeg_gather_bytes says";
    if ((uintptr_t)batch % 16 || (uintptr_t)quant % 16 || (uintptr_t)off % 8 || (uintptr_t)len % 4 || (uintptr_t)frames % 4 ||
        (uintptr_t)segments % 4 || (uintptr_t)h_desc % 4)
        return "misaligned buffer";
    a->bytes = arena; a->total_bytes = arena_bytes; a->off = off; a->len = len; a->quant = quant;
    a->frames = (const JpegFrameDesc*)frames; a->segments = (const JpegSegment*)segments;
    a->n_entries = (uint32_t)n_entries; a->n_segments = (uint32_t)n_arena_segments;
    b->buf = batch;
    return gather_check((const GatherDesc*)h_desc, m, a->n_entries, *b);
}

// The device's own check of frame j against the ARENA's records (the descriptor came from host copies of them): a frame that
// fails copies nothing (its bytes are zeros) and gets a record without a table set, its segments point nowhere (status 1,
// nothing touched); one whose destination is outside the batch writes its frame record and quant row only.
TSTAR_JPEG_HD inline bool gather_dest_ok(const Batch& b, const GatherDesc& d) {
    return d.dst % 16 == 0 && (uint64_t)d.dst + round16(d.len) <= b.total_bytes &&
           (uint64_t)d.first_segment + d.n_segments <= b.n_segments;
}
TSTAR_JPEG_HD inline bool gather_frame_ok(const Arena& a, const Batch& b, const GatherDesc& d) {
    if (!gather_dest_ok(b, d) || d.id >= a.n_entries) return false;
    if (a.len[d.id] != d.len || a.off[d.id] > a.total_bytes || d.len > a.total_bytes - a.off[d.id]) return false;
    const JpegFrameDesc f = a.frames[d.id];
    if (f.n_segments < 0 || (uint32_t)f.n_segments != d.n_segments) return false;
    if (d.n_segments && (f.first_segment < 0 || (uint64_t)f.first_segment + d.n_segments > a.n_segments)) return false;
    return true;
}

// Frame j's record.
TSTAR_JPEG_HD inline JpegFrameDesc gather_frame_record(const Arena& a, const GatherDesc& d, bool ok) {
    JpegFrameDesc f;
    f.table_set = ok ? a.frames[d.id].table_set : -1;
    f.first_segment = ok ? (int32_t)d.first_segment : 0;
    f.n_segments = ok ? (int32_t)d.n_segments : 0;
    f.reserved = 0;
    return f;
}

// Segment i of frame j, rebased to the batch.
TSTAR_JPEG_HD inline JpegSegment gather_segment(const Arena& a, const GatherDesc& d, uint32_t j, uint32_t i, bool ok) {
    JpegSegment s;
    s.frame = 0xffffffffu; s.begin = 0; s.end = 0; s.first_mcu = 0; s.n_mcu = 0; s.last = 0;
    if (!ok) return s;
    const JpegSegment r = a.segments[(uint32_t)a.frames[d.id].first_segment + i];
    if (r.begin > r.end || r.end > d.len) return s;
    s.frame = j; s.begin = d.dst + r.begin; s.end = d.dst + r.end;
    s.first_mcu = r.first_mcu; s.n_mcu = r.n_mcu; s.last = r.last;
    return s;
}

}  // namespace jpegres

// Host mirror of the gather launcher (jpeg_resident_host.cpp): the same buffer, word for word.  False on arguments the launcher
// refuses; *why (optional) says which.
bool jpeg_gather_host(const jpegres::Arena& a, const jpegres::GatherDesc* desc, const jpegres::Batch& b, const char** why);

}  // namespace tstar
