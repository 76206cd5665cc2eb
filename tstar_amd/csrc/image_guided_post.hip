// Image-guided (one-shot) detection: HF's post_process_image_guided_detection on the device.  The statements are those of
// image_guided_post_core.h (shared with the host entry, image_guided_post_host.cpp); this file is compiled with
// -ffp-contract=off (tstar_amd/build.py), so every float32 operation is the one torch performs.
//
// image_guided_post_kernel: ONE workgroup of 1024 threads (sixteen wave64) per image, everything of the image in LDS
// (dynamic: 8 n2 + 20 np bytes + the reduction partials, n2 = np rounded up to a power of two; 104.8 KB at np = 3600, so one
// workgroup per CU), phases separated by barriers:
//   1. every row: corners, the scaled box written out (by its own row), the sort key (score descending, index ascending:
//      igp_sort_key) into LDS; the tail of the key array up to n2 is filled with the largest key;
//   2. when nms_threshold < 1: bitonic sort of the n2 keys in LDS (log2(n2) (log2(n2) + 1) / 2 barriers; 78 at 4096).  Without
//      NMS the keys stay in row order;
//   3. corners and scores are laid out IN THE ORDER: position k holds the box and the live score of the k-th candidate, so the
//      sweep reads LDS contiguously (a 16-byte and a 4-byte read per lane, conflict-free) instead of gathering by row;
//   4. the sweep, one candidate per step: every thread reads the live score of position k (a broadcast); 0 -> the step is
//      skipped by the whole block, without a barrier (nothing was written).  Otherwise the lanes test the positions BEHIND k,
//      position k + 1 + tid, + 1024, ...: a position still live whose IoU with candidate k exceeds nms_threshold gets score 0;
//      one barrier ends the step.  A thread writes only positions it alone visits in that step, and position k' > k is read as
//      a candidate only after the barrier of the last live step before it;
//   5. block reductions (wave shuffles, then the waves' partials through LDS; max and an integer sum, neither depends on its
//      order): is any score non-zero, the largest thresholded score; alphas, the keep mask and the kept count, written by row.
//
// Why only the positions behind k.  HF lets a live candidate i zero EVERY j != i with iou(i, j) > nms_threshold.  box_iou is
// symmetric in its bits: area_i + area_j, max and min commute (up to the sign of a zero, which no comparison sees), so
// iou(i, j) and iou(j, i) are the same float.  Take a candidate e ahead of i in the order.  If e was live at its step, it tested
// i then; i is live now, so iou(e, i) did not exceed the threshold (or was NaN), and neither does iou(i, e).  If e was not live
// at its step, its score already is 0 and zeroing it again changes nothing.  So a live candidate has nothing to do ahead of
// itself, and the result is HF's; image_guided_post_host.cpp keeps HF's literal form and the tests compare the two word for word.
//
// No atomics; image b reads rows b np .. (b + 1) np - 1 of scores / boxes and writes the same rows of the outputs and n_kept[b].
#include "common.h"
#include "image_guided_post.h"
#include "image_guided_post_core.h"

namespace tstar {

constexpr int IGP_THREADS = 1024, IGP_WAVES = IGP_THREADS / 64;

static inline int igp_pow2(int np) {
    int n2 = 1;
    while (n2 < np) n2 <<= 1;
    return n2;
}
// keys [n2] u64 | boxes [np] 4 x f32 | live scores [np] f32 | wave partials: max f32 [16], any i32 [16], count i32 [16]
__host__ __device__ static inline size_t igp_key_bytes(int n2) { return ((size_t)n2 * 8 + 15) & ~(size_t)15; }     // the boxes behind them are read 16 bytes at a time
static inline size_t igp_lds_bytes(int np) { return igp_key_bytes(igp_pow2(np)) + (size_t)np * 20 + IGP_WAVES * 12; }

__global__ __launch_bounds__(IGP_THREADS) void image_guided_post_kernel(const float* __restrict__ scores_all, const float* __restrict__ boxes_all,
                                                                        const float* __restrict__ scale_xy, int np, int n2, float threshold,
                                                                        float nms_threshold, float* __restrict__ alphas_all,
                                                                        float* __restrict__ xyxy_all, uint8_t* __restrict__ keep_all,
                                                                        int* __restrict__ n_kept) {
    extern __shared__ __attribute__((aligned(16))) unsigned char igp_lds[];
    uint64_t* s_key = reinterpret_cast<uint64_t*>(igp_lds);
    f32x4* s_box = reinterpret_cast<f32x4*>(igp_lds + igp_key_bytes(n2));
    float* s_live = reinterpret_cast<float*>(igp_lds + igp_key_bytes(n2) + (size_t)np * 16);
    float* s_wmax = s_live + np;
    int* s_wany = reinterpret_cast<int*>(s_wmax + IGP_WAVES);
    int* s_wcount = s_wany + IGP_WAVES;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* scores = scores_all + (size_t)b * np;
    const float* boxes = boxes_all + (size_t)b * np * 4;
    float* alphas = alphas_all + (size_t)b * np;
    float* xyxy = xyxy_all + (size_t)b * np * 4;
    uint8_t* keep = keep_all + (size_t)b * np;
    const float sx = scale_xy ? scale_xy[2 * b] : 1.0f, sy = scale_xy ? scale_xy[2 * b + 1] : 1.0f;
    const bool nms = nms_threshold < 1.0f;

    // ---- 1. scaled boxes by row; sort keys
    for (int p = tid; p < n2; p += IGP_THREADS) {
        if (p < np) {
            const IgpBox c = igp_corners(boxes + (size_t)p * 4);
            igp_scaled(c, sx, sy, xyxy + (size_t)p * 4);
            s_key[p] = igp_sort_key(scores[p], (uint32_t)p);
        } else {
            s_key[p] = ~0ull;                                     // behind every row's key: a row's low word is below 2^32 - 1
        }
    }
    __syncthreads();

    // ---- 2. bitonic sort, ascending
    if (nms) {
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (n2 >> 1); t += IGP_THREADS) {
                    const int i = 2 * t - (t & (j - 1)), l = i + j;       // the t-th pair at distance j
                    const uint64_t a = s_key[i], c = s_key[l];
                    if ((a > c) == ((i & k) == 0)) { s_key[i] = c; s_key[l] = a; }
                }
                __syncthreads();
            }
        }
    }

    // ---- 3. boxes and scores in the order
    for (int k = tid; k < np; k += IGP_THREADS) {
        const uint32_t p = igp_key_index(s_key[k]);               // < np: the np smallest keys are the rows'
        const IgpBox c = igp_corners(boxes + (size_t)p * 4);
        f32x4 v; v[0] = c.x0; v[1] = c.y0; v[2] = c.x1; v[3] = c.y1;
        s_box[k] = v;
        s_live[k] = scores[p];
    }
    __syncthreads();

    // ---- 4. the sweep
    if (nms) {
        for (int k = 0; k + 1 < np; ++k) {
            if (s_live[k] == 0.0f) continue;                      // block-uniform: read after the last step's barrier
            const f32x4 cv = s_box[k];
            const IgpBox c{cv[0], cv[1], cv[2], cv[3]};
            const float area_c = igp_area(c);
            for (int q = k + 1 + tid; q < np; q += IGP_THREADS) {
                if (s_live[q] == 0.0f) continue;
                const f32x4 ov = s_box[q];
                const IgpBox o{ov[0], ov[1], ov[2], ov[3]};
                if (igp_iou(c, area_c, o, igp_area(o)) > nms_threshold) s_live[q] = 0.0f;
            }
            __syncthreads();
        }
    }

    // ---- 5. any non-zero score, the largest thresholded score
    int any = 0;
    float m = -INFINITY;
    for (int k = tid; k < np; k += IGP_THREADS) {
        const float s = s_live[k];
        any |= (s != 0.0f);
        m = fmaxf(m, igp_threshold(s, threshold));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    any = __any(any);
    if (lane == 0) { s_wmax[wave] = m; s_wany[wave] = any; }
    __syncthreads();
    m = s_wmax[0];
    any = s_wany[0];
#pragma unroll
    for (int w = 1; w < IGP_WAVES; ++w) { m = fmaxf(m, s_wmax[w]); any |= s_wany[w]; }
    m = m + 1e-6f;

    int count = 0;
    for (int k = tid; k < np; k += IGP_THREADS) {
        const uint32_t p = igp_key_index(s_key[k]);
        const float a = any ? igp_alpha(igp_threshold(s_live[k], threshold), m) : 0.0f;
        const int kept = a > 0.0f;
        alphas[p] = a;
        keep[p] = (uint8_t)kept;
        count += kept;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
    if (lane == 0) s_wcount[wave] = count;
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int w = 0; w < IGP_WAVES; ++w) n += s_wcount[w];
        n_kept[b] = n;
    }
}

int image_guided_post(const float* scores, const float* boxes_cxcywh, const float* scale_xy, int B, int np, float threshold, float nms_threshold,
                      float* alphas, float* boxes_xyxy, uint8_t* keep, int* n_kept, hipStream_t s) {
    TSTAR_REQUIRE(scores && boxes_cxcywh && alphas && boxes_xyxy && keep && n_kept, "image_guided_post: null argument");
    TSTAR_REQUIRE(B >= 1 && B <= 65535, "image_guided_post: B must be in 1..65535");
    TSTAR_REQUIRE(np >= 1 && np <= IMAGE_GUIDED_POST_MAX_NP, "image_guided_post: np must be in 1..3600");
    RC(ensure_dyn_lds(reinterpret_cast<const void*>(image_guided_post_kernel), (int)igp_lds_bytes(IMAGE_GUIDED_POST_MAX_NP)));
    hipLaunchKernelGGL(image_guided_post_kernel, dim3(B), dim3(IGP_THREADS), igp_lds_bytes(np), s, scores, boxes_cxcywh, scale_xy, np, igp_pow2(np),
                       threshold, nms_threshold, alphas, boxes_xyxy, keep, n_kept);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

}  // namespace tstar
