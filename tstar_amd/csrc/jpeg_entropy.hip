// Baseline JPEG entropy stage on the device: compressed bytes -> the int16 coefficient blocks jpeg.hip reads.
// One lane per segment (jpeg_entropy_core.h: a restart interval, or a whole scan without DRI); all segments of a chunk in
// one launch.  The decode itself is jpegcore::decode_segment, the code the host runs in jpeg_entropy_segments_host.
//
// Lanes of a wave sit in different streams, so the core is one loop whose iteration decodes one symbol with its magnitude
// bits and picks table, predictor and destination by data.  A workgroup is one wave; when all its usable segments name
// the same table set (the normal case: an AVI has one) the 9 KB set is staged in LDS, else each lane reads its own set
// from global memory.  That choice is the same for the whole wave, so it is a branch no lane diverges on.
#include "common.h"
#include "heads.h"
#include "jpeg_entropy_core.h"

namespace tstar {

namespace {

constexpr int kLanes = 64;             // one wave per workgroup: the uniformity vote below is a wave vote
constexpr int kSetWords = (int)(sizeof(JpegTableSet) / 4);
static_assert(sizeof(JpegTableSet) % 8 == 0, "staged as dwords");

__global__ __launch_bounds__(kLanes) void jpeg_entropy_kernel(jpegcore::SegmentBatch b) {
    __shared__ __attribute__((aligned(8))) uint32_t lds_words[kSetWords];
    const uint32_t i = blockIdx.x * kLanes + threadIdx.x;
    const bool in_range = i < b.n_segments;
    JpegSegment seg = {0, 0, 0, 0, 0, 0};
    int ts = -1;
    if (in_range) {
        seg = b.segments[i];
        ts = jpegcore::segment_table_set(b, seg);
    }
    const bool usable = ts >= 0;
    // one table set for the whole wave?  (lanes without a usable segment do not vote)
    const unsigned long long voters = __ballot(usable);
    const int first = voters ? __ffsll((long long)voters) - 1 : 0;
    const int ref = __shfl(ts, first);
    const bool uniform = voters != 0 && __all(!usable || ts == ref);
    if (uniform) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(b.tables + ref);
        for (int w = threadIdx.x; w < kSetWords; w += kLanes) lds_words[w] = src[w];
    }
    __syncthreads();
    int status = JPEG_MALFORMED;                                    // a record that points outside the batch
    if (usable) {
        int16_t* coef = b.coef + (size_t)seg.frame * b.g.per_frame;
        if (uniform)
            status = jpegcore::decode_segment(b.bytes, seg.begin, seg.end, reinterpret_cast<const JpegTableSet*>(lds_words), b.g,
                                              seg.first_mcu, seg.n_mcu, seg.last != 0, coef);
        else
            status = jpegcore::decode_segment(b.bytes, seg.begin, seg.end, b.tables + ts, b.g, seg.first_mcu, seg.n_mcu,
                                              seg.last != 0, coef);
    }
    if (in_range) b.seg_status[i] = status;
}

}  // namespace

int jpeg_entropy_segments(const jpegcore::SegmentBatch& b, hipStream_t s) {
    TSTAR_REQUIRE(b.bytes && b.segments && b.tables && b.frames && b.coef && b.seg_status, "jpeg_entropy_segments: null argument");
    TSTAR_REQUIRE(b.n_frames > 0 && b.n_segments > 0 && b.n_sets > 0 && b.total_bytes > 0 && b.total_bytes < 0xffffffffull,
                  "jpeg_entropy_segments: empty batch, or more bytes than a segment's 32-bit offsets reach");
    TSTAR_REQUIRE((uintptr_t)b.segments % 4 == 0 && (uintptr_t)b.tables % 8 == 0 && (uintptr_t)b.frames % 4 == 0 &&
                      (uintptr_t)b.coef % 2 == 0 && (uintptr_t)b.seg_status % 4 == 0,
                  "jpeg_entropy_segments: misaligned record buffer");
    TSTAR_REQUIRE(b.n_segments <= 0x7fffffffu - kLanes, "jpeg_entropy_segments: chunk too large for one launch");
    TSTAR_HIP_CHECK(hipMemsetAsync(b.coef, 0, (size_t)b.n_frames * b.g.per_frame * sizeof(int16_t), s));   // EOB leaves zeros
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((b.n_segments + kLanes - 1) / kLanes), dim3(kLanes), 0, s, b);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

}  // namespace tstar
