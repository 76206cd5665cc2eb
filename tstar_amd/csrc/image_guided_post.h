// Launcher of image_guided_post.hip (internal): HF's post_process_image_guided_detection, one workgroup per image.
#pragma once
#include "common.h"

namespace tstar {

// scores [B * np], boxes_cxcywh [B * np, 4], scale_xy [B, 2] (sx, sy per image; null = 1) -> alphas [B * np], boxes_xyxy [B * np, 4]
// (scaled), keep u8 [B * np] (alpha > 0, in patch order), n_kept [B]; all device pointers.  np <= 3600, refused beyond before
// anything is launched.  nms_threshold >= 1: no NMS.
int image_guided_post(const float* scores, const float* boxes_cxcywh, const float* scale_xy, int B, int np, float threshold, float nms_threshold,
                      float* alphas, float* boxes_xyxy, uint8_t* keep, int* n_kept, hipStream_t s);

}  // namespace tstar
