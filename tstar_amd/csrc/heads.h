// Launchers of heads.hip / preprocess.hip / jpeg.hip (internal); the searcher ingest is ingest.h.
#pragma once
#include "../../include/tstar_hip.h"
#include "device_buf.h"

namespace tstar {

struct DetectRowsArgs {
    const float* feats;    // [rows, 768]  image feats after detection LayerNorm
    const float* cls;      // [rows, 512]  class_head.dense0 output
    const float* boxh;     // [rows, 768]  box_head after dense1 + GELU, or null: no box tail, xyxy / cxcywh are not written
    const float* qn;       // [sets][32][512]  query embeds / (||q|| + 1e-6)
    const uint8_t* qmask;  // [sets][32]       0 = padded query
    const int* image_set;  // [B] query set of every image, or null (all images use set 0)
    const int* setQ;       // [sets] number of queries per set
    const float* shift_w; const float* shift_b;
    const float* scale_w; const float* scale_b;
    const float* box2_w;   // [4, 768]
    const float* box2_b;   // [4]
    const float* box_bias; // [np, 4]
    float* scores;         // [rows]
    int* labels;           // [rows]
    float* xyxy;           // [rows, 4] pixels of the passed image (may be null when boxh is)
    float* logits;         // [rows, Q] or null
    float* cxcywh;         // [rows, 4] or null
    int rows, np, Q;       // Q: common query count (row stride of `logits`), 0 if the sets differ
    float box_sx, box_sy;  // pixels per unit of the relative boxes: (W, H) of the passed image for OWL-ViT, (max(H, W), max(H, W)) for OWLv2
};
int detect_rows(const DetectRowsArgs& a, hipStream_t s);

// out[r] = dot(h[r, :768], w) + b[0]: the last layer of OWLv2's objectness head (one wave per row)
int row_dot768(const float* h, const float* w, const float* b, float* out, int rows, hipStream_t s);

// xyxy may be null for a 1 x 1 grid: every kept detection then falls in cell 0, where the clamped centre puts it anyway
int cell_reduce(const float* scores, const int* labels, const float* xyxy, const double* qweight, const int* image_set, int B, int np,
                int img_w, int img_h, int grows, int gcols, float thr, double* cell_conf, uint32_t* cell_mask,
                int* n_kept, hipStream_t s);

// paint the kept detections' boxes (score > thr) on u8 images [B,H,W,3] in place; xyxy [B,np,4], scores [B,np]
int draw_boxes(uint8_t* images, int B, int H, int W, const float* xyxy, const float* scores, int np, float thr, hipStream_t s);

// The per-image query sets of a call on either detector handle (Q[slot]: the queries installed there).  Every image's slot
// (h_image_set[b]; slot 0 without an array) is in range and has queries installed -- `missing` says what is not there and which
// entry installs it.  *q_uniform = the common Q when every image uses one set size, else 0; *q_max (optional) the largest.  A
// passed array is copied into `staged` on stream s (grown when a larger batch arrives).
static inline int check_query_sets(const std::string& fn, const char* missing, const int* Q, const int32_t* h_image_set, int B,
                                   DeviceBuf<int>& staged, hipStream_t s, int* q_uniform, int* q_max = nullptr) {
    int qu = -1, qm = 0;
    for (int b = 0; b < B; ++b) {
        const int set = h_image_set ? h_image_set[b] : 0;
        TSTAR_CHECK_SET(set, fn);
        if (Q[set] == 0) { set_error(fn + ": " + missing); return TSTAR_ERR_STATE; }
        qu = (b == 0 || qu == Q[set]) ? Q[set] : 0;
        qm = qm > Q[set] ? qm : Q[set];
    }
    if (h_image_set) {
        RC(staged.reserve((size_t)B, s));
        TSTAR_HIP_CHECK(hipMemcpyAsync(staged.p, h_image_set, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    }
    *q_uniform = qu;
    if (q_max) *q_max = qm;
    return TSTAR_OK;
}

// ---- preprocess.hip: the detector's bicubic pass ----
// Pillow-compatible fixed-point resampling tables for one axis (host side).
struct ResampleTable {
    int in_size = 0, out_size = 0, ksize = 0;
    int* d_bounds = nullptr;   // [out, 2] (first input index, tap count)
    int* d_coefs = nullptr;    // [out, ksize] int32, 22 fractional bits
};
int build_bicubic_table(ResampleTable* t, int in_size, int out_size, hipStream_t s);
void free_table(ResampleTable* t);

// u8 [B,H,W,3] -> u8 [B,H,OW,3]   (Pillow 8bpc horizontal pass)
int resample_h_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const ResampleTable& t, hipStream_t s);
// u8 [B,H,OW,3] -> vertical pass to t.out_size rows -> LUT normalise -> im2col f32 [B*np, 3*patch^2] (768 x 768: patch 32
// [B*576, 3072], patch 16 [B*2304, 768]); OW and t.out_size are multiples of the patch size
int resample_v_normalize_patchify(const uint8_t* in, float* out, uint8_t* out_u8, int B, int H, int OW, const ResampleTable& t,
                                  const float* lut, int patch, hipStream_t s);

// jpeg.hip: n frames of coefficient blocks [n][g.blocks()][64] + tables u16 [n][3][64] -> RGB u8 [n,H,W,3]; planes is a
// workspace of n * g.plane_bytes() bytes (layouts in jpeg_host.h)
struct JpegGeom;
int jpeg_reconstruct_u8(const int16_t* coef, const uint16_t* quant, int n, const JpegGeom& g, uint8_t* planes, uint8_t* rgb,
                        hipStream_t s);
// the same pixels with frame j written to pool[slots[j]] (pool u8 [pool_frames,H,W,3]; slots i32 [m], device memory; a slot
// outside the pool is skipped)
int jpeg_reconstruct_slots_u8(const int16_t* coef, const uint16_t* quant, int m, const JpegGeom& g, uint8_t* planes, uint8_t* pool,
                              int pool_frames, const int32_t* slots, hipStream_t s);
// both at 1/sg.scale size (scale 2, 4, 8; jpeg_host.h JpegScaledGeom): rgb u8 [n,oh,ow,3], pool u8 [pool_frames,oh,ow,3], planes
// a workspace of n * sg.plane_bytes() bytes
struct JpegScaledGeom;
int jpeg_reconstruct_scaled_u8(const int16_t* coef, const uint16_t* quant, int n, const JpegScaledGeom& sg, uint8_t* planes, uint8_t* rgb,
                               hipStream_t s);
int jpeg_reconstruct_slots_scaled_u8(const int16_t* coef, const uint16_t* quant, int m, const JpegScaledGeom& sg, uint8_t* planes,
                                     uint8_t* pool, int pool_frames, const int32_t* slots, hipStream_t s);
namespace jpegres { struct Arena; struct Batch; struct GatherDesc; }
// jpeg_resident.hip: arena frames -> the batch buffer of the entropy launchers (h_desc: what gather_args checked; d_desc: the
// same words in device memory, like every pointer of a and b)
int jpeg_gather(const jpegres::Arena& a, const jpegres::Batch& b, const jpegres::GatherDesc* h_desc, const jpegres::GatherDesc* d_desc,
                hipStream_t s);
namespace jpegcore { struct SegmentBatch; }
// jpeg_entropy.hip: clear b.coef, then one lane per segment of the batch (every pointer of b is device memory)
int jpeg_entropy_segments(const jpegcore::SegmentBatch& b, hipStream_t s);
// the same result, with segments of at least min_split_bytes bytes cut into sub-sequences of sub_bytes
// bytes, one lane each (workspace: jpeg_split_workspace_bytes bytes of device memory; seg_info i32 [n_segments])
int jpeg_entropy_split(const jpegcore::SegmentBatch& b, int sub_bytes, int min_split_bytes, int max_rounds, void* workspace,
                       size_t workspace_bytes, int32_t* seg_info, hipStream_t s);

}  // namespace tstar
