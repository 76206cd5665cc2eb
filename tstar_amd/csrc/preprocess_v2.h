// OWLv2 pre-processing (preprocess_v2.hip): the policy, the per-axis tables and the launcher (internal).
#pragma once
#include "common.h"
#include <vector>

namespace tstar {

enum { OWLV2_FORM_DIRECT = 0, OWLV2_FORM_FILTERED = 1 };
constexpr int OWLV2_LDS_LIMIT = 160 * 1024;      // LDS per CU on gfx950: the most one workgroup may ask for
constexpr int OWLV2_LDS_TARGET = 64 * 1024;      // preferred ceiling: two workgroups per CU

// One axis of the resize: S samples of the padded square -> `out` samples.  radius < 0: the Gaussian pass is skipped
// (sigma <= 1e-15, the axis does not shrink); radius 0 is a one-tap filter of weight 1.0: both are the identity pass.
struct Owlv2Axis {
    double factor, sigma;
    int radius;
};
Owlv2Axis owlv2_axis(int S, int out);
// the two taps of output index j: sample i0 with weight 1 - t, sample i1 with weight t (scipy zoom order 1, mirror, grid_mode)
void owlv2_zoom_tap(int S, int out, int j, int* i0, int* i1, double* t);
// the source window [lo, lo + n) that the outputs [k * tile, min((k + 1) * tile, out)) of an axis read: their taps, widened by
// `radius` samples on both sides and cut at the square's edges (a mirrored index falls back inside the cut window)
void owlv2_axis_window(int S, int out, int tile, int k, int radius, int* lo, int* n);

// What one pre-processing launch does.  Pure arithmetic, no HIP call.  error != null: the arguments are refused.
struct Owlv2Plan {
    int form;                  // OWLV2_FORM_*
    int tile_h, tile_w;        // output pixels per workgroup (filtered form); 1 x 4 per thread in the direct form
    int win_h, win_w;          // largest source window of any tile (filtered form), samples
    int lds_bytes;             // LDS per workgroup (direct form: the 256-entry table)
    int grid_x, grid_y;        // filtered: tiles along x / y (per image); direct: workgroups of 256 threads per batch image / 1
    int radius_y, radius_x;    // Gaussian radius per axis, -1 = skipped
    const char* error;
};
Owlv2Plan plan_owlv2_preprocess(int H, int W, int out_h, int out_w);

// the tables of one axis on the host, float64 with scipy's statements: taps (i0, i1, t) per output index and the Gaussian's
// left half gw [max(radius, 0) + 1] (gw[radius - k] weighs the samples at distance k)
void owlv2_axis_host(int S, int out, std::vector<int>& i0, std::vector<int>& i1, std::vector<double>& t, std::vector<double>& gw);

struct Owlv2AxisTable {
    int S = 0, out = 0, radius = -1;
    int* d_i0 = nullptr;       // [out]
    int* d_i1 = nullptr;       // [out]
    double* d_t = nullptr;     // [out]
    double* d_gw = nullptr;    // [max(radius, 0) + 1]: d_gw[radius - k] weighs the samples at distance k (d_gw[radius]: the centre)
};
// gw_given: the Gaussian's left half computed elsewhere (radius + 1 values) instead of this library's own (libm exp): HF's witness is
// numpy, whose exp may differ from libm's in the last bit
int build_owlv2_axis_table(Owlv2AxisTable* t, int S, int out, const std::vector<double>* gw_given = nullptr);
void free_owlv2_axis_table(Owlv2AxisTable* t);

// u8 [B, H, W, 3] -> im2col f32 [B * (out_h / 16) * (out_w / 16), 768] with the bits of HF's Owlv2ImageProcessorPil.
// d_norm: f32 [262] = the 256-entry rescale table | mean[3] | std[3]; d_minmax: int [B, 2] workspace (per-image clip bounds).
// *form_ran receives the form of the plan that was launched.
int owlv2_preprocess(const uint8_t* in, float* out, int* d_minmax, int B, int H, int W, int out_h, int out_w,
                     const Owlv2AxisTable& ty, const Owlv2AxisTable& tx, const float* d_norm, hipStream_t s, int* form_ran);

}  // namespace tstar
