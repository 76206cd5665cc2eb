// Lossless re-coding with a restart interval, device half: the scans tstar_jpeg_encode_scan_rst left in fixed-size slots -> a
// piece of a new arena and the records the gather and the entropy launchers need for it, without a compressed byte going to the
// host (records, layout and checks: jpeg_recode_core.h; host mirror: jpeg_recode_host.cpp).  Three launches on one stream:
//   jpeg_recode_offsets_kernel  one workgroup: every frame's length (header + scan, or the kept source bytes) and ONE exclusive
//                               sum over them -> off[0 .. m], len[0 .. m)
//   jpeg_recode_bytes_kernel    grid (x, j): workgroups x of frame j copy 16 KiB pieces of its bytes to off[j]: the header row and
//                               the scan, or the source frame.  The arena packs frames end to end, so a destination starts at any
//                               byte: single bytes up to its first 16-byte boundary and behind its last, 16-byte stores between
//                               them, from aligned loads shifted together (jpeg_vec_copy.h)
//   jpeg_recode_records_kernel  one workgroup per frame: quant row, frame record, and the segments -- a kept frame's are the
//                               source's moved with it; a re-coded frame's come from a pass over its stuffed bytes, 16 per lane and
//                               4 KiB per step with a workgroup sum in between: an FF followed by D0..D7 is marker k in stream
//                               order, which ends interval k at its FF and starts interval k + 1 behind it
// No load leaves the slot, the header row or the source frame it reads; no store leaves [off[j], off[j] + len[j]) below the
// output's capacity, or the record buffer.  Plain vector stores only; nothing synchronises.
// tstar_jpeg_recode_assemble_opt is the one launcher: header rows of a pitch the caller gives (a header with tables of its own exceeds
// 1024 bytes; a row per frame, or per group of frames and quantisation set) and any interval, 0 among them: no marker, one segment,
// which the marker pass finds by finding nothing.  tstar_jpeg_recode_assemble forwards to it with rows of 1024 bytes and an interval.
#include "common.h"
#include "jpeg_recode_core.h"
#include "jpeg_vec_copy.h"
#include "../../include/tstar_hip.h"

namespace tstar {

namespace {

using namespace jpegrec;

constexpr int kThreads = 256;
constexpr uint32_t kPiece = 16384;            // bytes of a frame a workgroup copies per step
constexpr uint32_t kTile = kThreads * 16;     // bytes of a scan the marker pass takes per step

__global__ __launch_bounds__(kThreads) void jpeg_recode_offsets_kernel(const RecodeDesc* __restrict__ desc, Source s, Scans c, Records r) {
    __shared__ uint64_t part[kThreads];
    const uint32_t t = threadIdx.x, per = (r.m + kThreads - 1) / kThreads;
    const uint32_t j0 = min(r.m, t * per), j1 = min(r.m, j0 + per);
    uint64_t sum = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t len = recode_frame_len(desc[j], j, s, c, r);
        r.len[j] = len;
        sum += len;
    }
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint64_t at = 0;
        for (int i = 0; i < kThreads; ++i) { const uint64_t v = part[i]; part[i] = at; at += v; }
        r.off[r.m] = at;
    }
    __syncthreads();
    uint64_t at = part[t];
    for (uint32_t j = j0; j < j1; ++j) { r.off[j] = at; at += r.len[j]; }
}

__device__ inline void copy_pieces(uint8_t* dst, const uint8_t* src, uint32_t n, const uint8_t* lo, const uint8_t* hi) {
    for (uint64_t p = (uint64_t)blockIdx.x * kPiece; p < n; p += (uint64_t)gridDim.x * kPiece) {
        const uint32_t q = (uint32_t)p, take = n - q < kPiece ? n - q : kPiece;
        jpegvec::copy_bytes(dst + q, src + q, take, lo, hi, threadIdx.x, kThreads);
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_recode_bytes_kernel(const RecodeDesc* __restrict__ desc, Source s, Scans c, Records r, Output o) {
    const uint32_t j = blockIdx.y;
    const RecodeDesc d = desc[j];
    const uint64_t off = r.off[j];
    const uint32_t len = r.len[j];
    if (!recode_frame_ok(d, j, s, c, r) || off + len > o.cap) return;
    uint8_t* dst = o.bytes + off;
    if (d.kind == RECODE_KEPT) {
        if (d.src_len != len) return;
        const uint8_t* src = s.bytes + d.src_off;
        copy_pieces(dst, src, len, src, src + len);
        return;
    }
    const uint32_t hlen = c.header_len[d.hdr], n = c.scan_len[j];
    if (hlen + n != len) return;
    const uint8_t* row = c.headers + (size_t)d.hdr * c.header_pitch;
    if (blockIdx.x == 0) jpegvec::copy_bytes(dst, row, hlen, row, row + c.header_pitch, threadIdx.x, kThreads);
    const uint8_t* scan = c.slots + (size_t)j * c.slot_bytes;
    copy_pieces(dst + hlen, scan, n, scan, scan + c.slot_bytes);
}

__global__ __launch_bounds__(kThreads) void jpeg_recode_records_kernel(const RecodeDesc* __restrict__ desc, Source s, Scans c, Records r, Output o) {
    __shared__ uint32_t cnt[kThreads];
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    const RecodeDesc d = desc[j];
    const uint64_t off = r.off[j];
    const uint32_t len = r.len[j];
    const bool ok = recode_frame_ok(d, j, s, c, r) && off + len <= o.cap;
    if (t < 24) {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (d.src < s.n_frames) q = reinterpret_cast<const uint4*>(s.quant + (size_t)d.src * 192)[t];
        reinterpret_cast<uint4*>(r.quant + (size_t)j * 192)[t] = q;
    }
    if (t == 32) r.frames[j] = recode_frame_record(d, ok);
    if (j == 0 && t == 33 && (r.n_segments & 1))                      // the 8 bytes behind an odd number of segments
        *reinterpret_cast<uint2*>(r.segments + r.n_segments) = make_uint2(0, 0);
    if ((uint64_t)d.first_segment + d.n_segments > r.n_segments) return;
    JpegSegment* segs = r.segments + d.first_segment;
    const uint32_t base = (uint32_t)off;
    if (!ok || d.kind == RECODE_KEPT) {
        for (uint32_t i = t; i < d.n_segments; i += kThreads) segs[i] = recode_kept_segment(d, s, j, i, base, ok);
        return;
    }
    const uint32_t first = base + c.header_len[d.hdr], n = c.scan_len[j];
    for (uint32_t i = t; i < d.n_segments; i += kThreads) {
        JpegSegment g = recode_new_segment(c, j, i, d.n_segments);
        if (i == 0) g.begin = first;
        if (i + 1 == d.n_segments) g.end = first + n - 2;             // the EOI's FF
        segs[i] = g;
    }
    __syncthreads();
    const uint8_t* scan = c.slots + (size_t)j * c.slot_bytes;
    uint32_t before = 0;                                              // markers in front of this step
    for (uint32_t tile = 0; tile < n; tile += kTile) {
        const uint32_t at = tile + 16 * t;
        uint32_t mask = 0;
        if (at < n) {                                                 // at + 16 <= slot_bytes: both are multiples of 16 and at < n <= slot_bytes
            const uint4 v = *reinterpret_cast<const uint4*>(scan + at);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint32_t next = at + 16 < n ? scan[at + 16] : 0;
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t b0 = (w[i >> 2] >> (8 * (i & 3))) & 255;
                const uint32_t b1 = i < 15 ? (w[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 255 : next;
                if (at + i + 1 < n && recode_is_marker((uint8_t)b0, (uint8_t)b1)) mask |= 1u << i;
            }
        }
        const uint32_t own = (uint32_t)__popc(mask);
        cnt[t] = own;
        __syncthreads();
        for (uint32_t step = 1; step < (uint32_t)kThreads; step <<= 1) {      // inclusive sum over the workgroup
            const uint32_t add = t >= step ? cnt[t - step] : 0;
            __syncthreads();
            cnt[t] += add;
            __syncthreads();
        }
        uint32_t k = before + cnt[t] - own;
        const uint32_t total = cnt[kThreads - 1];
        while (mask) {
            const uint32_t i = (uint32_t)__ffs((int)mask) - 1;
            mask &= mask - 1;
            if (k + 1 < d.n_segments) { segs[k].end = first + at + i; segs[k + 1].begin = first + at + i + 2; }
            ++k;
        }
        before += total;
        __syncthreads();
    }
}

}  // namespace

int jpeg_recode_assemble(const RecodeDesc* d_desc, const Source& s, const Scans& c, const Records& r, const Output& o, size_t longest,
                         hipStream_t st) {
    const uint64_t gx = (longest + kPiece - 1) / kPiece;
    hipLaunchKernelGGL(jpeg_recode_offsets_kernel, dim3(1), dim3(kThreads), 0, st, d_desc, s, c, r);
    TSTAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_recode_bytes_kernel, dim3((unsigned)(gx < 1 ? 1 : (gx > 1024 ? 1024 : gx)), r.m), dim3(kThreads), 0, st, d_desc, s,
                       c, r, o);
    TSTAR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_recode_records_kernel, dim3(r.m), dim3(kThreads), 0, st, d_desc, s, c, r, o);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

}  // namespace tstar

// ---------------------------------------------------------------------------------------------- C ABI (include/tstar_hip.h)
using namespace tstar;

extern "C" int tstar_jpeg_recode_assemble(const void* h_desc, const void* d_desc, int m, int n_segments, const uint8_t* d_headers,
                                          const uint32_t* d_header_len, int n_headers, const uint8_t* d_slots, size_t slot_bytes,
                                          const uint32_t* d_scan_len, int restart, int n_mcu, const uint8_t* d_src_bytes, size_t src_total,
                                          const uint16_t* d_src_quant, const void* d_src_frames, const void* d_src_segments, int n_src_frames,
                                          int n_src_segments, uint8_t* d_rec, size_t rec_bytes, uint8_t* d_out, size_t out_bytes,
                                          size_t longest, void* stream) {
    // the entry of the standard tables: rows of kHeaderPitch bytes and always an interval; the rest is the _opt entry's
    TSTAR_REQUIRE(restart >= 1, "tstar_jpeg_recode_assemble: restart interval outside 1..65535 or no MCU");
    return tstar_jpeg_recode_assemble_opt(h_desc, d_desc, m, n_segments, d_headers, jpegrec::kHeaderPitch, d_header_len, n_headers, d_slots, slot_bytes,
                                          d_scan_len, restart, n_mcu, d_src_bytes, src_total, d_src_quant, d_src_frames, d_src_segments, n_src_frames,
                                          n_src_segments, d_rec, rec_bytes, d_out, out_bytes, longest, stream);
}

// rows of header_pitch bytes and restart 0 allowed, as tstar_jpeg_recode_assemble_host_opt
extern "C" int tstar_jpeg_recode_assemble_opt(const void* h_desc, const void* d_desc, int m, int n_segments, const uint8_t* d_headers,
                                              size_t header_pitch, const uint32_t* d_header_len, int n_headers, const uint8_t* d_slots,
                                              size_t slot_bytes, const uint32_t* d_scan_len, int restart, int n_mcu,
                                              const uint8_t* d_src_bytes, size_t src_total, const uint16_t* d_src_quant,
                                              const void* d_src_frames, const void* d_src_segments, int n_src_frames, int n_src_segments,
                                              uint8_t* d_rec, size_t rec_bytes, uint8_t* d_out, size_t out_bytes, size_t longest,
                                              void* stream) {
    jpegrec::Source s; jpegrec::Scans c; jpegrec::Records r; jpegrec::Output o;
    const char* bad = jpegrec::recode_args(h_desc, m, n_segments, d_headers, d_header_len, n_headers, d_slots, slot_bytes, d_scan_len, restart,
                                           n_mcu, d_src_bytes, src_total, d_src_quant, d_src_frames, d_src_segments, n_src_frames,
                                           n_src_segments, d_rec, rec_bytes, d_out, out_bytes, &s, &c, &r, &o, header_pitch);
    TSTAR_REQUIRE(!bad, std::string("tstar_jpeg_recode_assemble_opt: ") + bad);
    TSTAR_REQUIRE(d_desc && (uintptr_t)d_desc % 4 == 0, "tstar_jpeg_recode_assemble_opt: null or misaligned device descriptor");
    return jpeg_recode_assemble((const jpegrec::RecodeDesc*)d_desc, s, c, r, o, longest, (hipStream_t)stream);
}
