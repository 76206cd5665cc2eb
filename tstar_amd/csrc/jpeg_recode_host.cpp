// Host mirror of the re-code assembly (jpeg_recode.hip) over the records of jpeg_recode_core.h: the same checks, the same record
// buffer and output bytes word for word.  HIP-free: also compiled alone by the CPU sanitizer build.
#include <string.h>

#include <string>

#include "jpeg_recode_core.h"

namespace tstar {

void set_error(const std::string& msg);          // capi.hip (or the stand-alone checker): thread-local last error

using namespace jpegrec;

void jpeg_recode_assemble_host(const RecodeDesc* desc, const Source& s, const Scans& c, const Records& r, const Output& o) {
    uint64_t at = 0;
    for (uint32_t j = 0; j < r.m; ++j) {                              // offsets: one exclusive sum
        r.off[j] = at;
        r.len[j] = recode_frame_len(desc[j], j, s, c, r);
        at += r.len[j];
    }
    r.off[r.m] = at;
    for (uint32_t j = 0; j < r.m; ++j) {
        const RecodeDesc& d = desc[j];
        const bool seg_ok = (uint64_t)d.first_segment + d.n_segments <= r.n_segments;
        const bool ok = recode_frame_ok(d, j, s, c, r) && r.off[j] + r.len[j] <= o.cap;
        if (d.src < s.n_frames) memcpy(r.quant + (size_t)j * 192, s.quant + (size_t)d.src * 192, 384);
        else memset(r.quant + (size_t)j * 192, 0, 384);
        r.frames[j] = recode_frame_record(d, ok);
        if (!seg_ok) continue;
        JpegSegment* segs = r.segments + d.first_segment;
        const uint32_t base = (uint32_t)r.off[j];
        if (!ok || d.kind == RECODE_KEPT) {
            if (ok && d.src_len) memcpy(o.bytes + r.off[j], s.bytes + d.src_off, d.src_len);
            for (uint32_t i = 0; i < d.n_segments; ++i) segs[i] = recode_kept_segment(d, s, j, i, base, ok);
            continue;
        }
        const uint32_t hlen = c.header_len[d.hdr], n = c.scan_len[j];
        const uint8_t* scan = c.slots + (size_t)j * c.slot_bytes;
        memcpy(o.bytes + r.off[j], c.headers + (size_t)d.hdr * c.header_pitch, hlen);
        memcpy(o.bytes + r.off[j] + hlen, scan, n);
        for (uint32_t i = 0; i < d.n_segments; ++i) segs[i] = recode_new_segment(c, j, i, d.n_segments);
        segs[0].begin = base + hlen;
        segs[d.n_segments - 1].end = base + hlen + n - 2;              // the EOI's FF
        uint32_t k = 0;
        for (uint32_t p = 0; p + 1 < n; ++p)
            if (recode_is_marker(scan[p], scan[p + 1])) {
                if (k + 1 < d.n_segments) { segs[k].end = base + hlen + p; segs[k + 1].begin = base + hlen + p + 2; }
                ++k;
            }
    }
    const uint64_t used = r.segments_at + (uint64_t)r.n_segments * sizeof(JpegSegment);
    memset(reinterpret_cast<uint8_t*>(r.off) - r.off_at + used, 0, (size_t)(r.nbytes - used));
}

}  // namespace tstar

// ---------------------------------------------------------------------------------------------- C ABI (include/tstar_hip.h)
using namespace tstar;

extern "C" {

size_t tstar_jpeg_recode_layout(int m, int n_segments, size_t* out5) {
    Records r;
    if (!recode_layout(m, n_segments, &r)) return 0;
    if (out5) {
        out5[0] = (size_t)r.off_at; out5[1] = (size_t)r.len_at; out5[2] = (size_t)r.quant_at; out5[3] = (size_t)r.frames_at;
        out5[4] = (size_t)r.segments_at;
    }
    return (size_t)r.nbytes;
}

// rows of header_pitch bytes (a multiple of 16; headers with tables of their own are longer than 1024 bytes), one row per frame or
// per group of frames, and restart 0 allowed (no DRI, no marker: a frame is one segment)
int tstar_jpeg_recode_assemble_host_opt(const void* desc, int m, int n_segments, const uint8_t* headers, size_t header_pitch,
                                        const uint32_t* header_len, int n_headers, const uint8_t* slots, size_t slot_bytes,
                                        const uint32_t* scan_len, int restart, int n_mcu, const uint8_t* src_bytes, size_t src_total,
                                        const uint16_t* src_quant, const void* src_frames, const void* src_segments, int n_src_frames,
                                        int n_src_segments, uint8_t* rec, size_t rec_bytes, uint8_t* out, size_t out_bytes) {
    Source s; Scans c; Records r; Output o;
    const char* bad = recode_args(desc, m, n_segments, headers, header_len, n_headers, slots, slot_bytes, scan_len, restart, n_mcu, src_bytes,
                                  src_total, src_quant, src_frames, src_segments, n_src_frames, n_src_segments, rec, rec_bytes, out, out_bytes,
                                  &s, &c, &r, &o, header_pitch);
    if (bad) { set_error(std::string("tstar_jpeg_recode_assemble_host_opt: ") + bad); return 1; }
    jpeg_recode_assemble_host((const RecodeDesc*)desc, s, c, r, o);
    return 0;
}

int tstar_jpeg_recode_assemble_host(const void* desc, int m, int n_segments, const uint8_t* headers, const uint32_t* header_len, int n_headers,
                                    const uint8_t* slots, size_t slot_bytes, const uint32_t* scan_len, int restart, int n_mcu,
                                    const uint8_t* src_bytes, size_t src_total, const uint16_t* src_quant, const void* src_frames,
                                    const void* src_segments, int n_src_frames, int n_src_segments, uint8_t* rec, size_t rec_bytes,
                                    uint8_t* out, size_t out_bytes) {
    // the entry of the standard tables: rows of kHeaderPitch bytes and always an interval; the rest is the _opt entry's
    if (restart < 1) { set_error("tstar_jpeg_recode_assemble_host: restart interval outside 1..65535 or no MCU"); return 1; }
    return tstar_jpeg_recode_assemble_host_opt(desc, m, n_segments, headers, kHeaderPitch, header_len, n_headers, slots, slot_bytes, scan_len, restart,
                                               n_mcu, src_bytes, src_total, src_quant, src_frames, src_segments, n_src_frames, n_src_segments, rec,
                                               rec_bytes, out, out_bytes);
}

}  // extern "C"
