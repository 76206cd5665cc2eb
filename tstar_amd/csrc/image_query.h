// Launcher of image_query.hip (internal): the query-box selection of image-guided detection.
#pragma once
#include "common.h"

namespace tstar {

constexpr int IMAGE_QUERY_MAX_NP = 3600;       // the largest patch grid a handle may have (owl_geom_input)

struct ImageQueryOut {                          // device pointers, one entry per example image
    float* embeds;      // [n, 512] class embedding of the chosen row (the input row's bits); zeros when nothing is selected
    int* best;          // [n] chosen row, -1 when nothing is selected
    float* boxes;       // [n, 4] cxcywh of the chosen row (zeros when nothing is selected)
    int* n_selected;    // [n] rows with IoU (GIoU) >= 0.8 x the maximum
    int* status;        // [n] 0 IoU, 1 GIoU fallback used, 2 empty selection
};
static inline size_t image_query_out_bytes(int n) { return (size_t)n * (512 + 4 + 3) * 4; }
ImageQueryOut image_query_out_at(void* d_buf, int n);
static inline ImageQueryOut image_query_out_offset(const ImageQueryOut& o, int b0) {
    return ImageQueryOut{o.embeds + (size_t)b0 * 512, o.best + b0, o.boxes + (size_t)b0 * 4, o.n_selected + b0, o.status + b0};
}

// cls [n * np, 512], boxes_cxcywh [n * np, 4]: one workgroup per image; np <= IMAGE_QUERY_MAX_NP.  boxes_q [n, 4] (device):
// the query box of every example, relative xyxy; null = the unit box [0, 0, 1, 1] for all
int image_query_select(const float* cls, const float* boxes_cxcywh, const float* boxes_q, int n, int np, const ImageQueryOut& out, hipStream_t s);

// The end of an image-query entry `fn`: with rc == 0 the device results go to the caller's host arrays; the stream is synchronised
// and the staging buffer d_buf (what image_query_out_at carved `o` from) freed either way.  Returns rc, or the copies' error.
int image_query_finish(const char* fn, int rc, void* d_buf, const ImageQueryOut& o, int n, float* h_embeds, int32_t* h_best, float* h_boxes,
                       int32_t* h_n_selected, int32_t* h_status, hipStream_t s);

}  // namespace tstar
