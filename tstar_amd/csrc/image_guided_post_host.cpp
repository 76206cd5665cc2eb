// HF's post_process_image_guided_detection on host arrays: the statements of image_guided_post_core.h in HF's own order, one
// image after the other.  HIP-free (compiled as plain C++ with -ffp-contract=off): what the device kernel is compared against word
// for word, what tests pin to HF without a GPU, and what the stand-alone checker runs under the sanitizers.
//
// Unlike the kernel, a live candidate here tests EVERY other box, as HF does, not only the candidates behind it in the order: the
// kernel's shortcut (image_guided_post.hip) is checked against the literal form.
#include "image_guided_post_core.h"

#include <algorithm>
#include <string>
#include <vector>

namespace tstar {

void set_error(const std::string& msg);          // capi.hip (or the stand-alone checker): thread-local last error

void image_guided_post_image_host(const float* scores, const float* boxes_cxcywh, int np, float threshold, float nms_threshold, float sx,
                                  float sy, float* alphas, float* boxes_xyxy, uint8_t* keep, int32_t* n_kept) {
    std::vector<float> s(scores, scores + np), area((size_t)np);
    std::vector<IgpBox> box((size_t)np);
    for (int p = 0; p < np; ++p) {
        box[(size_t)p] = igp_corners(boxes_cxcywh + (size_t)p * 4);
        area[(size_t)p] = igp_area(box[(size_t)p]);
    }
    if (nms_threshold < 1.0f) {
        std::vector<uint64_t> order((size_t)np);
        for (int p = 0; p < np; ++p) order[(size_t)p] = igp_sort_key(s[(size_t)p], (uint32_t)p);
        std::sort(order.begin(), order.end());
        for (int k = 0; k < np; ++k) {
            const size_t i = igp_key_index(order[(size_t)k]);
            if (s[i] == 0.0f) continue;
            for (size_t j = 0; j < (size_t)np; ++j)
                if (j != i && igp_iou(box[i], area[i], box[j], area[j]) > nms_threshold) s[j] = 0.0f;
        }
    }
    for (int p = 0; p < np; ++p) igp_scaled(box[(size_t)p], sx, sy, boxes_xyxy + (size_t)p * 4);
    bool any = false;
    for (int p = 0; p < np; ++p) any |= s[(size_t)p] != 0.0f;
    int n = 0;
    float m = 0.0f;
    if (any) {
        for (int p = 0; p < np; ++p) {
            s[(size_t)p] = igp_threshold(s[(size_t)p], threshold);
            m = p == 0 ? s[0] : fmaxf(m, s[(size_t)p]);
        }
        m = m + 1e-6f;
    }
    for (int p = 0; p < np; ++p) {
        const float a = any ? igp_alpha(s[(size_t)p], m) : 0.0f;
        alphas[p] = a;
        keep[p] = a > 0.0f ? 1 : 0;
        n += keep[p];
    }
    *n_kept = n;
}

}  // namespace tstar

using namespace tstar;

extern "C" int tstar_image_guided_postprocess_host(const float* scores, const float* boxes_cxcywh, int B, int np, float threshold,
                                                   float nms_threshold, const float* scale_xy, float* alphas, float* boxes_xyxy,
                                                   uint8_t* keep, int32_t* n_kept) {
    if (!scores || !boxes_cxcywh || !alphas || !boxes_xyxy || !keep || !n_kept) {
        set_error("tstar_image_guided_postprocess_host: null argument");
        return 1;
    }
    if (B < 1 || B > 65535 || np < 1 || np > IMAGE_GUIDED_POST_MAX_NP) {
        set_error("tstar_image_guided_postprocess_host: B must be in 1..65535 and np in 1..3600");
        return 1;
    }
    for (int b = 0; b < B; ++b) {
        const size_t o = (size_t)b * np;
        image_guided_post_image_host(scores + o, boxes_cxcywh + o * 4, np, threshold, nms_threshold, scale_xy ? scale_xy[2 * b] : 1.0f,
                                     scale_xy ? scale_xy[2 * b + 1] : 1.0f, alphas + o, boxes_xyxy + o * 4, keep + o, n_kept + b);
    }
    return 0;
}
