// The YOLO-World convolutions (yolo_conv.hip) as the program interpreter (yolo.hip) sees them.  Internal.
#pragma once
#include "common.h"
#include "yolo_program.h"

namespace tstar {

// A kernel argument: field order and types are part of the generated code.
struct ConvArgs {
    const float* src; int src_ld, src_off, cin, H, W;       // input NHWC [B,H,W,src_ld], channels [src_off, src_off+cin)
    float* dst; int dst_ld, dst_off, cout, Ho, Wo;
    const float* w;                                          // [cout][ks*ks*cin]
    const float* wt;                                         // the same matrix transposed, [ks*ks*cin][cout] (scalar-weight kernel)
    const float* bias;                                       // [cout] or null
    unsigned zoff;                                           // element offset (from src) of the zero quad kept behind the source buffer
    const float* aux; int aux_ld, aux_off;                   // residual tensor (same spatial size as dst) or attention [P, heads]
    int ks, stride, act, mode, heads;
    int M;                                                   // B * Ho * Wo
};

// Which kernel a conv launches (TSTAR_YOLO_FORM_* in include/tstar_hip.h) and its grid: mt x nt workgroups of 256 threads; for the
// direct form mt blocks of nt threads.  error != null: the launcher refuses the layer.
struct ConvPlan { int form = -1, mt = 0, nt = 0; const char* error = nullptr; };

// The integers of a conv op's launch for B images of a handle whose buffers hold max_batch; the caller sets the pointers.
ConvArgs conv_args(const YoloProgram& p, const YoloConvOp& c, int B, int max_batch);

// Launches the form the policy plans for `a`; *form_out (optional) receives it.
int launch_conv(const ConvArgs& a, hipStream_t s, int* form_out = nullptr);

// W [cout][K] -> Wt [K][cout]
int launch_transpose_w(const float* w, float* wt, int cout, int K, hipStream_t s);

}  // namespace tstar
