// HF's post_process_image_guided_detection (image_processing_pil_owlvit.py; Owlv2's is the same statements) for one image, in
// float32: the statements the device kernel (image_guided_post.hip) and the host entry (image_guided_post_host.cpp) share.
// HIP-free: this header compiles as device code under hipcc and as plain C++ (the host entry, the stand-alone checker
// image_guided_post_check_main.cpp).  Every file that includes it is compiled with -ffp-contract=off: a fused multiply-add in the
// corner, area or IoU arithmetic would change which side of nms_threshold an IoU falls on.
//
// Per image, with scores [np] (the sigmoid of the max logit over the queries) and boxes [np, 4] (cxcywh, relative):
//   1. corners x0 = cx - 0.5 w, y0 = cy - 0.5 h, x1 = cx + 0.5 w, y1 = cy + 0.5 h;
//   2. when nms_threshold < 1: greedy NMS.  Candidates in descending score order (equal scores: lowest index first -- torch's
//      argsort leaves ties open); a candidate whose score is 0 is skipped; a live candidate i sets the score of every j != i with
//      iou(i, j) > nms_threshold to 0, iou = inter / ((area_i + area_j) - inter), inter from max of the top-left and min of the
//      bottom-right corners, extents clamped at 0.  A NaN IoU (two degenerate boxes: 0 / 0) compares false, as in torch;
//   3. boxes scaled by (sx, sy, sx, sy);
//   4. no non-zero score left: alphas 0, nothing kept (HF drops such an image from its list);
//   5. otherwise scores < threshold become 0, m = max + 1e-6f, alpha = clip((s - m * 0.1f) / (m * 0.9f), 0, 1), kept: alpha > 0.
// Inputs hold no NaN (a sigmoid and a box head's sigmoid never give one); with NaN the results are defined (fmaxf / fminf drop
// it where torch would carry it on) and every access stays in bounds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TSTAR_IGP_HD __host__ __device__
#else
#include <math.h>
#define TSTAR_IGP_HD
#endif

namespace tstar {

constexpr int IMAGE_GUIDED_POST_MAX_NP = 3600;     // the largest patch grid a handle may have (owl_geom_input)

struct IgpBox { float x0, y0, x1, y1; };

TSTAR_IGP_HD inline IgpBox igp_corners(const float* cxcywh) {
    const float cx = cxcywh[0], cy = cxcywh[1], w = cxcywh[2], h = cxcywh[3];
    return IgpBox{cx - 0.5f * w, cy - 0.5f * h, cx + 0.5f * w, cy + 0.5f * h};
}

TSTAR_IGP_HD inline float igp_area(const IgpBox& b) { return (b.x1 - b.x0) * (b.y1 - b.y0); }

// box_iou(a, b): symmetric in its bits (+, max and min commute; a zero's sign, which max / min of +0 and -0 may give either
// way, reaches no comparison)
TSTAR_IGP_HD inline float igp_iou(const IgpBox& a, float area_a, const IgpBox& b, float area_b) {
    const float iw = fmaxf(fminf(a.x1, b.x1) - fmaxf(a.x0, b.x0), 0.0f), ih = fmaxf(fminf(a.y1, b.y1) - fmaxf(a.y0, b.y0), 0.0f);
    const float inter = iw * ih;
    return inter / ((area_a + area_b) - inter);
}

// The NMS order as ONE ascending unsigned key: score descending (through the usual order-preserving map of float bits), then index
// ascending.  Total and free of ties for any bits, NaN included, so a sort by it cannot leave its array.
TSTAR_IGP_HD inline uint64_t igp_sort_key(float score, uint32_t index) {
    union { float f; uint32_t u; } v;
    v.f = score;
    const uint32_t asc = (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
    return ((uint64_t)(~asc) << 32) | index;
}
TSTAR_IGP_HD inline uint32_t igp_key_index(uint64_t key) { return (uint32_t)key; }

TSTAR_IGP_HD inline float igp_threshold(float s, float threshold) { return s < threshold ? 0.0f : s; }

// m = the image's largest thresholded score + 1e-6f
TSTAR_IGP_HD inline float igp_alpha(float s, float m) {
    const float a = (s - m * 0.1f) / (m * 0.9f);
    return fminf(fmaxf(a, 0.0f), 1.0f);
}

TSTAR_IGP_HD inline void igp_scaled(const IgpBox& b, float sx, float sy, float* out4) {
    out4[0] = b.x0 * sx; out4[1] = b.y0 * sy; out4[2] = b.x1 * sx; out4[3] = b.y1 * sy;
}

}  // namespace tstar
