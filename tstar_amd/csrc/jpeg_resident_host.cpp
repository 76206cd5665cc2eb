// Host mirror of the gather kernel (jpeg_resident.hip) over the records of jpeg_resident_core.h: the same checks in the same
// order, the same batch buffer word for word.  HIP-free: also compiled alone by the CPU sanitizer build.
#include <string.h>

#include <string>

#include "jpeg_resident_core.h"

namespace tstar {

void set_error(const std::string& msg);          // capi.hip (or the stand-alone checker): thread-local last error

using namespace jpegres;

bool jpeg_gather_host(const Arena& a, const GatherDesc* desc, const Batch& b, const char** why) {
    if (const char* bad = gather_check(desc, (int)b.m, a.n_entries, b)) {
        if (why) *why = bad;
        return false;
    }
    uint16_t* quant = reinterpret_cast<uint16_t*>(b.buf + b.quant_at);
    JpegFrameDesc* frames = reinterpret_cast<JpegFrameDesc*>(b.buf + b.frames_at);
    JpegSegment* segments = reinterpret_cast<JpegSegment*>(b.buf + b.segments_at);
    for (uint32_t j = 0; j < b.m; ++j) {
        const GatherDesc& d = desc[j];
        const bool ok = gather_frame_ok(a, b, d);
        if (ok) memcpy(quant + (size_t)j * 192, a.quant + (size_t)d.id * 192, 384);
        else memset(quant + (size_t)j * 192, 0, 384);
        frames[j] = gather_frame_record(a, d, ok);
        if (!gather_dest_ok(b, d)) continue;               // never after gather_check; the kernel asks its own copy of the words
        const uint32_t copied = ok ? d.len : 0;
        if (copied) memcpy(b.buf + d.dst, a.bytes + a.off[d.id], copied);
        memset(b.buf + d.dst + copied, 0, (size_t)(round16(d.len) - copied));
        for (uint32_t i = 0; i < d.n_segments; ++i) segments[d.first_segment + i] = gather_segment(a, d, j, i, ok);
    }
    const uint64_t used = b.segments_at + (uint64_t)b.n_segments * sizeof(JpegSegment);
    memset(b.buf + used, 0, (size_t)(b.nbytes - used));
    return true;
}

}  // namespace tstar

// ---------------------------------------------------------------------------------------------- C ABI (include/tstar_hip.h)
using namespace tstar;

extern "C" {

size_t tstar_jpeg_gather_bytes(size_t total_bytes, int m, int n_segments, size_t* out3) {
    Batch b;
    if (!gather_layout(total_bytes, m, n_segments, &b)) return 0;
    if (out3) { out3[0] = (size_t)b.quant_at; out3[1] = (size_t)b.frames_at; out3[2] = (size_t)b.segments_at; }
    return (size_t)b.nbytes;
}

int tstar_jpeg_gather_host(const uint8_t* arena, size_t arena_bytes, const uint64_t* off, const uint32_t* len, const uint16_t* quant,
                           const void* frames, const void* segments, int n_entries, int n_arena_segments, const void* desc, int m,
                           size_t total_bytes, int n_segments, uint8_t* batch, size_t batch_bytes) {
    Arena a;
    Batch b;
    const char* bad = gather_args(arena, arena_bytes, off, len, quant, frames, segments, n_entries, n_arena_segments, desc, m, total_bytes,
                                  n_segments, batch, batch_bytes, &a, &b);
    if (!bad) jpeg_gather_host(a, (const GatherDesc*)desc, b, &bad);
    if (bad) { set_error(std::string("tstar_jpeg_gather_host: ") + bad); return 1; }
    return 0;
}

}  // extern "C"
