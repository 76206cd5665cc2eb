// Baseline JPEG entropy stage on the device: compressed bytes -> the int16 coefficient blocks jpeg.hip reads.  The decode
// itself is jpeg_entropy_core.h, the code the host runs in jpeg_entropy_segments_host and jpeg_entropy_split_host (the
// latter in the same round order), so host and device agree word for word.
//
// jpeg_entropy_segments: one lane per segment (a restart interval, or a whole scan without DRI); all segments of a chunk
// in one launch.  Lanes of a wave sit in different streams, so the core is one loop whose iteration decodes one symbol with
// its magnitude bits and picks table, predictor and destination by data.
//
// jpeg_entropy_split, for frames WITHOUT restart markers: a long segment is cut into sub-sequences of sub_bytes bytes, one
// lane each (jpeg_entropy_core.h "sub-sequences"; Weissenberger & Schmidt, ICPP 2018).
// One call is a chain of launches on one stream; order between phases comes from the kernel boundaries alone (no lane
// ever waits on a value another workgroup produces in the same launch):
//   layout      one workgroup: which segments are cut, and where their sub-sequences sit in the workspace
//   round r     r = 0 .. max_rounds, one lane per sub-sequence, count form: reads the exits of round r - 1 (copy (r - 1) & 1),
//               writes copy r & 1; a lane whose predecessor's exit did not change copies its own
//   scan        one wave per segment: seg_info, then first block and DC predictors of each sub-sequence
//   write       one lane per sub-sequence of a converged segment, write form
//   one lane    every segment that is not cut or was abandoned, and again every cut one the write pass refused
// Lanes of a wave take adjacent sub-sequences, so they read neighbouring bytes and, all but the waves that straddle two
// frames with different tables, one table set.
//
// Every decoding kernel stages the 9 KB table set in LDS when all the segments of its workgroup name the same one (the
// normal case: an AVI has one), else each lane reads its own set from global memory; the choice is the workgroup's, so
// no lane diverges on it.
//
// This parses untrusted bytes: every loop of a lane is bounded by the bits of its sub-sequence plus one symbol, reads stay
// inside the segment's byte range, stores inside the frame's coefficient region and the caller-sized workspace.
#include "common.h"
#include "heads.h"
#include "jpeg_entropy_core.h"

namespace tstar {

namespace {

using namespace jpegcore;

constexpr int kBlock = 256;            // sub-sequence kernels: four waves share one staged table set
constexpr int kWave = 64;              // one lane per segment, and the scan: one wave per workgroup
constexpr int kLayoutThreads = 1024;
constexpr int kSetWords = (int)(sizeof(JpegTableSet) / 4);
static_assert(sizeof(JpegTableSet) % 8 == 0, "staged as dwords");

struct SplitArgs {
    SegmentBatch b;
    SplitWs w;
    uint32_t sub_bytes, min_split_bytes, max_rounds;
    int32_t* seg_info;
};

// One workgroup: n_sub and the exclusive prefix sub_first over all segments (64-bit sums: a list of overlapping records may
// ask for more sub-sequences than the workspace holds; such segments stay whole).
__global__ __launch_bounds__(kLayoutThreads) void jpeg_split_layout_kernel(SplitArgs a) {
    __shared__ unsigned long long part[kLayoutThreads];
    const uint32_t nseg = a.b.n_segments, t = threadIdx.x;
    const uint32_t per = (nseg + kLayoutThreads - 1) / kLayoutThreads;
    const uint32_t lo = t * per < nseg ? t * per : nseg, hi = lo + per < nseg ? lo + per : nseg;
    unsigned long long sum = 0;
    for (uint32_t si = lo; si < hi; ++si) sum += split_n_sub(a.b, a.b.segments[si], a.sub_bytes, a.min_split_bytes);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kLayoutThreads; d <<= 1) {                  // inclusive scan of the per-thread sums
        const unsigned long long v = t >= (uint32_t)d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long at = part[t] - sum;
    uint32_t total = 0;
    bool any = false;
    for (uint32_t si = lo; si < hi; ++si) {
        const uint32_t n = split_n_sub(a.b, a.b.segments[si], a.sub_bytes, a.min_split_bytes);
        const bool fits = n != 0 && at + n <= a.w.cap;
        a.w.n_sub[si] = fits ? n : 0;
        a.w.sub_first[si] = (uint32_t)(at < 0xffffffffull ? at : 0xffffffffull);
        a.w.last_changed[si] = 0;
        at += n;
        if (fits) { total = (uint32_t)at; any = true; }
    }
    // the total is the end of the last segment that fits: the largest of the threads' ends
    __shared__ uint32_t s_total;
    if (t == 0) s_total = 0;
    __syncthreads();
    if (any) atomicMax(&s_total, total);
    __syncthreads();
    if (t == 0) *a.w.total = s_total;
}

// The segment of sub-sequence `lane` (< *w.total): the last one whose first sub-sequence is not behind it (segments that
// are not cut share their sub_first with the next one that is).
__device__ inline uint32_t segment_of_lane(const SplitWs& w, uint32_t nseg, uint32_t lane) {
    uint32_t lo = 0, hi = nseg;                                     // sub_first[lo] <= lane; the answer is in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (w.sub_first[mid] <= lane) lo = mid; else hi = mid;
    }
    return lo;
}

// The staged table set of a workgroup of kThreads threads, and the two words its threads agree through.
struct StagedTables {
    __attribute__((aligned(8))) uint32_t words[kSetWords];
    int ref, mixed;
    __device__ const JpegTableSet* set() const { return reinterpret_cast<const JpegTableSet*>(words); }
};

// Does the whole workgroup name one table set (ts of its active lanes; the others do not vote)?  Stages it in LDS when it
// does.  Every thread of the workgroup calls this (barriers inside).
template <int kThreads>
__device__ inline bool stage_tables(const SegmentBatch& b, bool active, int ts, StagedTables* lds) {
    if (threadIdx.x == 0) { lds->ref = -1; lds->mixed = 0; }
    __syncthreads();
    if (active) {
        const int old = atomicCAS(&lds->ref, -1, ts);
        if (old != -1 && old != ts) lds->mixed = 1;
    }
    __syncthreads();
    const bool uniform = lds->ref >= 0 && lds->mixed == 0;
    if (uniform) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(b.tables + lds->ref);
        for (int wd = threadIdx.x; wd < kSetWords; wd += kThreads) lds->words[wd] = src[wd];
    }
    __syncthreads();
    return uniform;
}

template <bool kWritePass>
__global__ __launch_bounds__(kBlock) void jpeg_split_lane_kernel(SplitArgs a, uint32_t round) {
    __shared__ StagedTables lds;
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t total = *a.w.total;
    if (blockIdx.x * kBlock >= total) return;                       // the whole workgroup: no barrier is skipped by some
    bool active = lane < total && lane < a.w.cap;
    uint32_t si = 0;
    int ts = -1;
    if (active) {
        si = segment_of_lane(a.w, a.b.n_segments, lane);
        const uint32_t first = a.w.sub_first[si], n = a.w.n_sub[si];
        active = lane >= first && lane - first < n;                 // always, by the layout
        if (active && kWritePass) active = a.seg_info[si] > 0;
        if (active && !kWritePass) active = !split_round_copies(a.w, round, first, lane);     // a lane that only copies its exit needs no tables
        if (active) ts = segment_table_set(a.b, a.b.segments[si]);
        active = active && ts >= 0;                                 // always: only usable segments are cut
    }
    const bool uniform = stage_tables<kBlock>(a.b, active, ts, &lds);
    if (!active) return;
    if (kWritePass) {
        const int st = uniform ? split_write_lane(a.b, a.w, a.sub_bytes, a.max_rounds, si, lane, lds.set())
                               : split_write_lane(a.b, a.w, a.sub_bytes, a.max_rounds, si, lane, a.b.tables + ts);
        if (st != JPEG_OK) a.b.seg_status[si] = JPEG_MALFORMED;     // any sub-sequence: the segment is decoded again by one lane
    } else {
        if (uniform) split_round_lane(a.b, a.w, a.sub_bytes, round, si, lane, lds.set());
        else split_round_lane(a.b, a.w, a.sub_bytes, round, si, lane, a.b.tables + ts);
    }
}

// One wave per segment: seg_info, and for a converged segment the exclusive scan over (blocks, DC sums) of its sub-sequences.
__global__ __launch_bounds__(kWave) void jpeg_split_scan_kernel(SplitArgs a) {
    const uint32_t si = blockIdx.x, t = threadIdx.x;
    const int32_t info = split_seg_info(a.w, si, a.max_rounds);
    if (t == 0) {
        a.seg_info[si] = info;
        if (info > 0) a.b.seg_status[si] = JPEG_OK;
    }
    if (info <= 0) return;
    const uint32_t first = a.w.sub_first[si], n = a.w.n_sub[si];
    unsigned long long blocks = 0;
    uint32_t d0 = 0, d1 = 0, d2 = 0;                                // carried from chunk to chunk (the same in every lane)
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t i = base + t;
        const bool in = i < n;
        unsigned long long vb = in ? a.w.blocks[first + i] : 0;
        uint32_t v0 = in ? a.w.dc0[first + i] : 0, v1 = in ? a.w.dc1[first + i] : 0, v2 = in ? a.w.dc2[first + i] : 0;
        const unsigned long long ob = vb;
        const uint32_t o0 = v0, o1 = v1, o2 = v2;
        for (int d = 1; d < kWave; d <<= 1) {                       // inclusive wave scan
            const unsigned long long ub = __shfl_up(vb, d);
            const uint32_t u0 = __shfl_up(v0, d), u1 = __shfl_up(v1, d), u2 = __shfl_up(v2, d);
            if ((int)t >= d) { vb += ub; v0 += u0; v1 += u1; v2 += u2; }
        }
        if (in) {
            const unsigned long long fb = blocks + vb - ob;
            a.w.first_block[first + i] = (uint32_t)(fb < 0xffffffffull ? fb : 0xffffffffull);
            a.w.pred0[first + i] = d0 + v0 - o0; a.w.pred1[first + i] = d1 + v1 - o1; a.w.pred2[first + i] = d2 + v2 - o2;
        }
        blocks += __shfl(vb, kWave - 1);
        d0 += __shfl(v0, kWave - 1); d1 += __shfl(v1, kWave - 1); d2 += __shfl(v2, kWave - 1);
    }
}

// One lane per segment.  seg_info == nullptr (jpeg_entropy_segments): every segment, and the status stands.  Else the
// segments a split call leaves to it: not cut, abandoned, or cut and refused by the write pass.  The last kind keeps
// decode_segment's status, but OK becomes UNCOVERED: the write pass refused what one lane accepts, which must never happen.
__global__ __launch_bounds__(kWave) void jpeg_one_lane_kernel(SegmentBatch b, const int32_t* seg_info) {
    __shared__ StagedTables lds;
    const uint32_t i = blockIdx.x * kWave + threadIdx.x;
    JpegSegment seg = {0, 0, 0, 0, 0, 0};
    int ts = -1;
    bool mine = false, redo = false;
    if (i < b.n_segments) {
        redo = seg_info && seg_info[i] > 0;
        mine = !redo || b.seg_status[i] != JPEG_OK;
        if (mine) {
            seg = b.segments[i];
            ts = segment_table_set(b, seg);
        }
    }
    const bool usable = ts >= 0;
    const bool uniform = stage_tables<kWave>(b, usable, ts, &lds);
    int status = JPEG_MALFORMED;                                    // a record that points outside the batch
    if (usable) {
        int16_t* coef = b.coef + (size_t)seg.frame * b.g.per_frame;
        status = uniform ? decode_segment(b.bytes, seg.begin, seg.end, lds.set(), b.g, seg.first_mcu, seg.n_mcu, seg.last != 0, coef)
                         : decode_segment(b.bytes, seg.begin, seg.end, b.tables + ts, b.g, seg.first_mcu, seg.n_mcu, seg.last != 0, coef);
        if (redo && status == JPEG_OK) status = JPEG_UNCOVERED;
    }
    if (mine) b.seg_status[i] = status;
}

// What both launchers ask of a batch -> TSTAR_OK, or TSTAR_ERR_ARG with the error set under the caller's name.
int require_batch(const SegmentBatch& b, const char* who) {
    const std::string w = std::string(who) + ": ";
    TSTAR_REQUIRE(b.bytes && b.segments && b.tables && b.frames && b.coef && b.seg_status, w + "null argument");
    TSTAR_REQUIRE(b.n_frames > 0 && b.n_segments > 0 && b.n_sets > 0 && b.total_bytes > 0 && b.total_bytes < 0xffffffffull,
                  w + "empty batch, or more bytes than a segment's 32-bit offsets reach");
    TSTAR_REQUIRE((uintptr_t)b.segments % 4 == 0 && (uintptr_t)b.tables % 8 == 0 && (uintptr_t)b.frames % 4 == 0 &&
                      (uintptr_t)b.coef % 2 == 0 && (uintptr_t)b.seg_status % 4 == 0,
                  w + "misaligned record buffer");
    TSTAR_REQUIRE(b.n_segments <= 0x7fffffffu - kWave, w + "chunk too large for one launch");
    return TSTAR_OK;
}

// EOB leaves zeros
hipError_t clear_coef(const SegmentBatch& b, hipStream_t s) {
    return hipMemsetAsync(b.coef, 0, (size_t)b.n_frames * b.g.per_frame * sizeof(int16_t), s);
}

void launch_one_lane(const SegmentBatch& b, const int32_t* seg_info, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_one_lane_kernel, dim3((b.n_segments + kWave - 1) / kWave), dim3(kWave), 0, s, b, seg_info);
}

}  // namespace

int jpeg_entropy_segments(const jpegcore::SegmentBatch& b, hipStream_t s) {
    if (const int rc = require_batch(b, "jpeg_entropy_segments")) return rc;
    TSTAR_HIP_CHECK(clear_coef(b, s));
    launch_one_lane(b, nullptr, s);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

int jpeg_entropy_split(const jpegcore::SegmentBatch& b, int sub_bytes, int min_split_bytes, int max_rounds, void* workspace,
                       size_t workspace_bytes, int32_t* seg_info, hipStream_t s) {
    TSTAR_REQUIRE(seg_info, "jpeg_entropy_split: null argument");
    if (const int rc = require_batch(b, "jpeg_entropy_split")) return rc;
    TSTAR_REQUIRE((uintptr_t)seg_info % 4 == 0, "jpeg_entropy_split: misaligned record buffer");
    TSTAR_REQUIRE(jpeg_split_args_ok(b.total_bytes, (int)b.n_segments, sub_bytes, min_split_bytes, max_rounds, workspace, workspace_bytes),
                  "jpeg_entropy_split: sub_bytes below TSTAR_JPEG_SUB_BYTES_MIN or no multiple of 4, min_split_bytes < 0, max_rounds "
                  "outside 1 .. TSTAR_JPEG_SPLIT_MAX_ROUNDS, or a workspace that is null, misaligned or smaller than "
                  "tstar_jpeg_split_workspace_bytes says");
    SplitArgs a;
    a.b = b;
    const uint64_t cap = split_cap(b.total_bytes, b.n_segments, (uint32_t)sub_bytes);
    a.w = split_ws_carve(workspace, cap, b.n_segments);
    a.sub_bytes = (uint32_t)sub_bytes; a.min_split_bytes = (uint32_t)min_split_bytes; a.max_rounds = (uint32_t)max_rounds;
    a.seg_info = seg_info;
    TSTAR_HIP_CHECK(clear_coef(b, s));
    hipLaunchKernelGGL(jpeg_split_layout_kernel, dim3(1), dim3(kLayoutThreads), 0, s, a);
    const dim3 lanes((unsigned)((cap + kBlock - 1) / kBlock));
    if (min_split_bytes > 0)                                        // 0: nothing is cut, the rounds would find no sub-sequence
        for (uint32_t r = 0; r <= a.max_rounds; ++r) hipLaunchKernelGGL(jpeg_split_lane_kernel<false>, lanes, dim3(kBlock), 0, s, a, r);
    hipLaunchKernelGGL(jpeg_split_scan_kernel, dim3(b.n_segments), dim3(kWave), 0, s, a);
    if (min_split_bytes > 0) hipLaunchKernelGGL(jpeg_split_lane_kernel<true>, lanes, dim3(kBlock), 0, s, a, 0u);
    launch_one_lane(b, seg_info, s);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

}  // namespace tstar
