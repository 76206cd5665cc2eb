// Compressed-resident JPEG store, device half: a list of arena frames -> the batch buffer the entropy launchers take
// (records, layout and checks: jpeg_resident_core.h; host mirror: jpeg_resident_host.cpp).  One launch per fetch:
//   grid (x, j)  workgroups x of frame j copy its bytes in 16-byte vectors to the frame's 16-byte-aligned start in the batch;
//                workgroup 0 of the frame also writes its quant row, its frame record and its rebased segments.
// An arena frame starts at any byte (the arena packs files end to end), so a destination vector is either one aligned load
// (source aligned too), two aligned loads shifted together (both wholly inside the frame), or -- the first vector of a
// misaligned frame, and its last one or two -- up to 16 single bytes.  No load leaves [off, off + len) of the arena, no store
// leaves the frame's padded range of the batch; the padding is written as zeros, so that the buffer is the mirror's word for word.
#include "common.h"
#include "jpeg_resident_core.h"
#include "jpeg_vec_copy.h"

namespace tstar {

namespace {

using namespace jpegres;
using jpegvec::funnel;

constexpr int kThreads = 256;
constexpr uint32_t kVecPerWg = 1024;          // 16 KiB of a frame per workgroup: a 22 KB 360x640 frame takes two

__global__ __launch_bounds__(kThreads) void jpeg_gather_kernel(Arena a, Batch b, const GatherDesc* __restrict__ desc) {
    const uint32_t j = blockIdx.y, t = threadIdx.x;
    const GatherDesc d = desc[j];
    const bool ok = gather_frame_ok(a, b, d);
    if (blockIdx.x == 0) {
        if (t < 24) {
            uint4 q = make_uint4(0, 0, 0, 0);
            if (ok) q = reinterpret_cast<const uint4*>(a.quant + (size_t)d.id * 192)[t];
            reinterpret_cast<uint4*>(b.buf + b.quant_at + (size_t)j * 384)[t] = q;
        }
        if (t == 32) reinterpret_cast<JpegFrameDesc*>(b.buf + b.frames_at)[j] = gather_frame_record(a, d, ok);
        if (j == 0 && t == 33 && (b.n_segments & 1))              // the 8 bytes behind an odd number of segments
            *reinterpret_cast<uint2*>(b.buf + b.segments_at + (size_t)b.n_segments * sizeof(JpegSegment)) = make_uint2(0, 0);
    }
    if (!gather_dest_ok(b, d)) return;
    if (blockIdx.x == 0) {
        JpegSegment* segs = reinterpret_cast<JpegSegment*>(b.buf + b.segments_at) + d.first_segment;
        for (uint32_t i = t; i < d.n_segments; i += kThreads) segs[i] = gather_segment(a, d, j, i, ok);
    }
    const uint32_t nvec = (d.len + 15) / 16, len = ok ? d.len : 0;
    const uint8_t* src = a.bytes + (ok ? a.off[d.id] : 0);
    const uint32_t mis = (uint32_t)((uintptr_t)src & 15);
    uint4* dst = reinterpret_cast<uint4*>(b.buf + d.dst);
    const uint32_t v1 = min(nvec, (blockIdx.x + 1) * kVecPerWg);
    for (uint32_t k = blockIdx.x * kVecPerWg + t; k < v1; k += kThreads) {
        const uint32_t at = 16 * k;                     // nvec <= 2^28: no overflow
        uint4 v;
        if (mis == 0 && len >= 16 && at <= len - 16) {
            v = *reinterpret_cast<const uint4*>(src + at);
        } else if (mis != 0 && k >= 1 && len >= 32 && at - mis <= len - 32) {
            const uint4* p = reinterpret_cast<const uint4*>(src + at - mis);
            v = funnel(p[0], p[1], mis);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t i = 0; i < 16; ++i)
                if (at + i < len) w[i >> 2] |= (uint32_t)src[at + i] << (8 * (i & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        dst[k] = v;
    }
}

}  // namespace

int jpeg_gather(const Arena& a, const Batch& b, const GatherDesc* h_desc, const GatherDesc* d_desc, hipStream_t s) {
    TSTAR_REQUIRE(d_desc && (uintptr_t)d_desc % 4 == 0, "jpeg_gather: null or misaligned device descriptor");
    TSTAR_REQUIRE(b.m <= 65535, "jpeg_gather: more than 65535 frames in one fetch");
    uint32_t longest = 0;
    for (uint32_t j = 0; j < b.m; ++j) longest = h_desc[j].len > longest ? h_desc[j].len : longest;
    const uint32_t gx = (uint32_t)((((uint64_t)longest + 15) / 16 + kVecPerWg - 1) / kVecPerWg);
    hipLaunchKernelGGL(jpeg_gather_kernel, dim3(gx ? gx : 1, b.m), dim3(kThreads), 0, s, a, b, d_desc);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

}  // namespace tstar
