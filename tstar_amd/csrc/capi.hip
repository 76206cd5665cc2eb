// C ABI of libtstar_hip.so (include/tstar_hip.h): the error plumbing and the stateless entry points (GEMM, attention, ingest, JPEG,
// cell_reduce, draw_boxes, plans).  The detector handles live beside their kernels: owl.hip, yolo.hip (+ yolo_conv.hip), searcher.hip.
#include "../../include/tstar_hip.h"
#include "common.h"
#include "heads.h"
#include "image_guided_post.h"
#include "image_query.h"
#include "ingest.h"
#include "jpeg_entropy_core.h"
#include "jpeg_host.h"
#include "jpeg_resident_core.h"
#include "kernels.h"
#include "owl_weights.h"
#include <mutex>
#include <set>

namespace tstar {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

int ensure_dyn_lds(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("ensure_dyn_lds: hipGetDevice failed"); return 2; }
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(kernel, dev);
    if (done.count(key)) return 0;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) { set_error(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e)); return 2; }
    done.insert(key);
    return 0;
}

// Wb[i] = bfloat16(W[i]), round to nearest even (exact when W already holds bf16 values);
// optional second term Wlo[i] = bfloat16(W[i] - Wb[i]) (the difference is exact in f32)
__global__ void f32_to_bf16_kernel(const float* __restrict__ W, __bf16* __restrict__ Wb, __bf16* __restrict__ Wlo, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float w = W[i];
        const __bf16 hi = (__bf16)w;
        Wb[i] = hi;
        if (Wlo) Wlo[i] = (__bf16)(w - (float)hi);
    }
}
int convert_f32_to_bf16(const float* W, __bf16* Wb, __bf16* Wlo, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(1024), dim3(256), 0, s, W, Wb, Wlo, n);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}
}  // namespace tstar

using namespace tstar;

extern "C" {

const char* tstar_last_error(void) { return g_err.c_str(); }
int tstar_abi_version(void) { return 3; }

int tstar_cell_reduce(const float* d_scores, const int32_t* d_labels, const float* d_boxes_xyxy, const double* h_weights, int n_sets,
                      const int32_t* h_image_set, int B, int np, int W, int H, int grid_rows, int grid_cols, float thr,
                      double* d_cell_conf, uint32_t* d_cell_mask, int32_t* d_n_kept, void* stream) {
    TSTAR_REQUIRE(d_scores && d_labels && d_boxes_xyxy && h_weights && d_cell_conf && d_cell_mask && d_n_kept, "tstar_cell_reduce: null argument");
    TSTAR_REQUIRE(B >= 1 && np >= 1 && W >= 1 && H >= 1, "tstar_cell_reduce: empty batch or image");
    TSTAR_REQUIRE(n_sets >= 1 && n_sets <= TSTAR_OWL_MAX_SETS, "tstar_cell_reduce: n_sets must be in 1..64");
    TSTAR_REQUIRE(grid_rows > 0 && grid_cols > 0 && grid_rows * grid_cols <= 4096, "tstar_cell_reduce: grid must have 1..4096 cells");
    for (int b = 0; h_image_set && b < B; ++b)
        TSTAR_REQUIRE(h_image_set[b] >= 0 && h_image_set[b] < n_sets, "tstar_cell_reduce: image set out of range");
    hipStream_t s = (hipStream_t)stream;
    double* d_w = nullptr;
    int* d_set = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&d_w, (size_t)n_sets * TSTAR_OWL_MAX_QUERIES * sizeof(double)));
    hipError_t e = hipMemcpyAsync(d_w, h_weights, (size_t)n_sets * TSTAR_OWL_MAX_QUERIES * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && h_image_set) {
        e = hipMalloc(&d_set, (size_t)B * sizeof(int));
        if (e == hipSuccess) e = hipMemcpyAsync(d_set, h_image_set, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s);
    }
    int rc = TSTAR_OK;
    if (e == hipSuccess)
        rc = cell_reduce(d_scores, d_labels, d_boxes_xyxy, d_w, d_set, B, np, W, H, grid_rows, grid_cols, thr, d_cell_conf, d_cell_mask, d_n_kept, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);           // the staging copies are freed below
    (void)hipFree(d_w);
    if (d_set) (void)hipFree(d_set);
    if (!rc && e != hipSuccess) { set_error(std::string("tstar_cell_reduce: ") + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    return rc;
}

// the selection launcher on caller tensors; fn: the entry's name in messages
static int image_query_select_entry(const std::string& fn, const float* d_cls, const float* d_boxes_cxcywh, const float* d_boxes_q, int n, int np,
                                    float* h_embeds, int32_t* h_best, float* h_boxes_cxcywh, int32_t* h_n_selected, int32_t* h_status, void* stream) {
    TSTAR_REQUIRE(d_cls && d_boxes_cxcywh && h_embeds && h_best && h_boxes_cxcywh && h_n_selected && h_status, fn + ": null argument");
    TSTAR_REQUIRE(n >= 1 && n <= 65535, fn + ": n must be in 1..65535");
    TSTAR_REQUIRE(np >= 1 && np <= IMAGE_QUERY_MAX_NP, fn + ": np must be in 1..3600");
    TSTAR_REQUIRE(((uintptr_t)d_cls & 15) == 0, fn + ": d_cls must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    void* d_buf = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&d_buf, image_query_out_bytes(n)));
    const ImageQueryOut o = image_query_out_at(d_buf, n);
    const int rc = image_query_select(d_cls, d_boxes_cxcywh, d_boxes_q, n, np, o, s);
    return image_query_finish(fn.c_str(), rc, d_buf, o, n, h_embeds, h_best, h_boxes_cxcywh, h_n_selected, h_status, s);
}

int tstar_image_query_select_box(const float* d_cls, const float* d_boxes_cxcywh, const float* d_boxes_q, int n, int np, float* h_embeds,
                                 int32_t* h_best, float* h_boxes_cxcywh, int32_t* h_n_selected, int32_t* h_status, void* stream) {
    return image_query_select_entry("tstar_image_query_select_box", d_cls, d_boxes_cxcywh, d_boxes_q, n, np, h_embeds, h_best, h_boxes_cxcywh,
                                    h_n_selected, h_status, stream);
}

int tstar_image_query_select(const float* d_cls, const float* d_boxes_cxcywh, int n, int np, float* h_embeds, int32_t* h_best, float* h_boxes_cxcywh,
                             int32_t* h_n_selected, int32_t* h_status, void* stream) {
    return image_query_select_entry("tstar_image_query_select", d_cls, d_boxes_cxcywh, nullptr, n, np, h_embeds, h_best, h_boxes_cxcywh, h_n_selected,
                                    h_status, stream);
}

int tstar_image_guided_postprocess(const float* d_scores, const float* d_boxes_cxcywh, int B, int np, float threshold, float nms_threshold,
                                   const float* h_scale_xy, float* d_alphas, float* d_boxes_xyxy, uint8_t* d_keep, int32_t* d_n_kept, void* stream) {
    TSTAR_REQUIRE(d_scores && d_boxes_cxcywh && d_alphas && d_boxes_xyxy && d_keep && d_n_kept, "tstar_image_guided_postprocess: null argument");
    TSTAR_REQUIRE(B >= 1 && B <= 65535, "tstar_image_guided_postprocess: B must be in 1..65535");
    TSTAR_REQUIRE(np >= 1 && np <= 3600, "tstar_image_guided_postprocess: np must be in 1..3600");
    hipStream_t s = (hipStream_t)stream;
    if (!h_scale_xy) return image_guided_post(d_scores, d_boxes_cxcywh, nullptr, B, np, threshold, nms_threshold, d_alphas, d_boxes_xyxy, d_keep, d_n_kept, s);
    float* d_scale = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&d_scale, (size_t)B * 2 * sizeof(float)));
    hipError_t e = hipMemcpyAsync(d_scale, h_scale_xy, (size_t)B * 2 * sizeof(float), hipMemcpyHostToDevice, s);
    int rc = TSTAR_OK;
    if (e == hipSuccess) rc = image_guided_post(d_scores, d_boxes_cxcywh, d_scale, B, np, threshold, nms_threshold, d_alphas, d_boxes_xyxy, d_keep, d_n_kept, s);
    const hipError_t e2 = hipStreamSynchronize(s);              // the staging copy is freed below
    if (e == hipSuccess) e = e2;
    (void)hipFree(d_scale);
    if (!rc && e != hipSuccess) { set_error(std::string("tstar_image_guided_postprocess: ") + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    return rc;
}

int tstar_frames_to_grid(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx, int grid_rows,
                         int grid_cols, uint8_t* d_grid, int nv12, void* stream) {
    TSTAR_REQUIRE(d_video && d_frame_idx && d_grid, "tstar_frames_to_grid: null argument");
    TSTAR_REQUIRE(N >= 1 && H >= 2 && W >= 2, "tstar_frames_to_grid: bad video shape");
    TSTAR_REQUIRE(!nv12 || (H % 2 == 0 && W % 2 == 0), "tstar_frames_to_grid: NV12 needs even dimensions");
    return frames_to_grid_u8(d_video, H, W, d_frame_idx, grid_rows, grid_cols, 200, 95, d_grid, nv12, (hipStream_t)stream);
}

int tstar_frames_resize(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx, int n, int out_w,
                        int out_h, uint8_t* d_out, int nv12, void* stream) {
    TSTAR_REQUIRE(d_video && d_frame_idx && d_out, "tstar_frames_resize: null argument");
    TSTAR_REQUIRE(N >= 1 && H >= 2 && W >= 2, "tstar_frames_resize: bad video shape");
    TSTAR_REQUIRE(!nv12 || (H % 2 == 0 && W % 2 == 0), "tstar_frames_resize: NV12 needs even dimensions");
    return bilinear_gather_u8(d_video, H, W, d_frame_idx, n, out_w, out_h, d_out, nv12, (hipStream_t)stream);
}

int tstar_nv12_to_rgb(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx, int n, uint8_t* d_out,
                      void* stream) {
    TSTAR_REQUIRE(d_video && d_frame_idx && d_out, "tstar_nv12_to_rgb: null argument");
    TSTAR_REQUIRE(N >= 1 && H >= 2 && W >= 2, "tstar_nv12_to_rgb: bad video shape");
    return nv12_to_rgb_u8(d_video, H, W, d_frame_idx, n, d_out, (hipStream_t)stream);
}

int tstar_i420_to_nv12(const uint8_t* d_i420, int n, int H, int W, uint8_t* d_nv12, void* stream) {
    TSTAR_REQUIRE(d_i420 && d_nv12 && d_i420 != d_nv12, "tstar_i420_to_nv12: null or aliased argument");
    return i420_to_nv12_u8(d_i420, n, H, W, d_nv12, (hipStream_t)stream);
}

int tstar_jpeg_entropy_device(const uint8_t* d_bytes, size_t total_bytes, const void* d_segments, const void* d_table_sets,
                              int n_sets, const void* d_frames, int n_frames, int n_segments, int W, int H, int ncomp, int hs,
                              int vs, int16_t* d_coef, int32_t* d_seg_status, void* stream) {
    jpegcore::SegmentBatch b;
    const char* bad = jpegcore::segment_batch(d_bytes, total_bytes, d_segments, d_table_sets, n_sets, d_frames, n_frames, n_segments,
                                              JpegGeom{W, H, ncomp, hs, vs}, d_coef, d_seg_status, &b);
    TSTAR_REQUIRE(!bad, std::string("tstar_jpeg_entropy_device: ") + bad);
    return jpeg_entropy_segments(b, (hipStream_t)stream);
}

int tstar_jpeg_entropy_split_device(const uint8_t* d_bytes, size_t total_bytes, const void* d_segments, const void* d_table_sets,
                                    int n_sets, const void* d_frames, int n_frames, int n_segments, int W, int H, int ncomp, int hs,
                                    int vs, int sub_bytes, int min_split_bytes, int max_rounds, void* d_workspace,
                                    size_t workspace_bytes, int16_t* d_coef, int32_t* d_seg_status, int32_t* d_seg_info, void* stream) {
    TSTAR_REQUIRE(d_seg_info && d_workspace, "tstar_jpeg_entropy_split_device: null argument");
    jpegcore::SegmentBatch b;
    const char* bad = jpegcore::segment_batch(d_bytes, total_bytes, d_segments, d_table_sets, n_sets, d_frames, n_frames, n_segments,
                                              JpegGeom{W, H, ncomp, hs, vs}, d_coef, d_seg_status, &b);
    TSTAR_REQUIRE(!bad, std::string("tstar_jpeg_entropy_split_device: ") + bad);
    return jpeg_entropy_split(b, sub_bytes, min_split_bytes, max_rounds, d_workspace, workspace_bytes, d_seg_info, (hipStream_t)stream);
}

int tstar_jpeg_reconstruct(const int16_t* d_coef, const uint16_t* d_quant, int n, int W, int H, int ncomp, int hs, int vs,
                           uint8_t* d_planes, uint8_t* d_rgb, void* stream) {
    TSTAR_REQUIRE(d_coef && d_quant && d_planes && d_rgb, "tstar_jpeg_reconstruct: null argument");
    const JpegGeom g{W, H, ncomp, hs, vs};
    return jpeg_reconstruct_u8(d_coef, d_quant, n, g, d_planes, d_rgb, (hipStream_t)stream);
}

int tstar_jpeg_reconstruct_slots(const int16_t* d_coef, const uint16_t* d_quant, int m, int W, int H, int ncomp, int hs, int vs,
                                 uint8_t* d_planes, uint8_t* d_pool, int pool_frames, const int32_t* d_slots, void* stream) {
    TSTAR_REQUIRE(d_coef && d_quant && d_planes && d_pool && d_slots, "tstar_jpeg_reconstruct_slots: null argument");
    const JpegGeom g{W, H, ncomp, hs, vs};
    return jpeg_reconstruct_slots_u8(d_coef, d_quant, m, g, d_planes, d_pool, pool_frames, d_slots, (hipStream_t)stream);
}

int tstar_jpeg_reconstruct_scaled(const int16_t* d_coef, const uint16_t* d_quant, int n, int W, int H, int ncomp, int hs, int vs,
                                  int scale, uint8_t* d_planes, uint8_t* d_rgb, void* stream) {
    if (scale == 1) return tstar_jpeg_reconstruct(d_coef, d_quant, n, W, H, ncomp, hs, vs, d_planes, d_rgb, stream);
    TSTAR_REQUIRE(d_coef && d_quant && d_planes && d_rgb, "tstar_jpeg_reconstruct_scaled: null argument");
    const JpegScaledGeom sg{JpegGeom{W, H, ncomp, hs, vs}, scale};
    return jpeg_reconstruct_scaled_u8(d_coef, d_quant, n, sg, d_planes, d_rgb, (hipStream_t)stream);
}

int tstar_jpeg_reconstruct_slots_scaled(const int16_t* d_coef, const uint16_t* d_quant, int m, int W, int H, int ncomp, int hs, int vs,
                                        int scale, uint8_t* d_planes, uint8_t* d_pool, int pool_frames, const int32_t* d_slots,
                                        void* stream) {
    if (scale == 1) return tstar_jpeg_reconstruct_slots(d_coef, d_quant, m, W, H, ncomp, hs, vs, d_planes, d_pool, pool_frames, d_slots, stream);
    TSTAR_REQUIRE(d_coef && d_quant && d_planes && d_pool && d_slots, "tstar_jpeg_reconstruct_slots_scaled: null argument");
    const JpegScaledGeom sg{JpegGeom{W, H, ncomp, hs, vs}, scale};
    return jpeg_reconstruct_slots_scaled_u8(d_coef, d_quant, m, sg, d_planes, d_pool, pool_frames, d_slots, (hipStream_t)stream);
}

int tstar_jpeg_gather(const uint8_t* d_arena, size_t arena_bytes, const uint64_t* d_off, const uint32_t* d_len, const uint16_t* d_quant,
                      const void* d_frames, const void* d_segments, int n_entries, int n_arena_segments, const void* h_desc,
                      const void* d_desc, int m, size_t total_bytes, int n_segments, uint8_t* d_batch, size_t batch_bytes, void* stream) {
    jpegres::Arena a;
    jpegres::Batch b;
    const char* bad = jpegres::gather_args(d_arena, arena_bytes, d_off, d_len, d_quant, d_frames, d_segments, n_entries, n_arena_segments,
                                           h_desc, m, total_bytes, n_segments, d_batch, batch_bytes, &a, &b);
    TSTAR_REQUIRE(!bad, std::string("tstar_jpeg_gather: ") + bad);
    return jpeg_gather(a, b, (const jpegres::GatherDesc*)h_desc, (const jpegres::GatherDesc*)d_desc, (hipStream_t)stream);
}

int tstar_gemm_f32(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual, int M,
                   int N, int K, int act, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_f32: null argument");
    return gemm_f32(gemm_args(d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act), (hipStream_t)stream);
}

int tstar_gemm_f32_cfg(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual,
                       int M, int N, int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_f32_cfg: null argument");
    GemmArgs g = gemm_args(d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act);
    g.tile_cfg = tile_cfg;
    return gemm_f32(g, (hipStream_t)stream);
}

// The converting diagnostics: the planes of `wmode` built for this one launch (a Wq plane wherever the shape allows), the launch,
// and a wait for it; the planes are freed by scope, after the wait.  g: the launch on the f32 matrix; fn: the entry's name.
static int gemm_on_built_planes(const char* fn, GemmArgs g, int wmode, int tile_cfg, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    g.tile_cfg = tile_cfg;
    WeightPlanes planes;
    int rc = build_weight_planes(g.W, g.N, g.K, wmode, true, s, &planes);
    if (!rc) rc = gemm_f32(with_planes(g, planes), s);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) { set_error(std::string(fn) + ": " + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    return rc;
}

int tstar_gemm_bf16w(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual, int M,
                     int N, int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_bf16w: null argument");
    return gemm_on_built_planes("tstar_gemm_bf16w", gemm_args(d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act), GEMM_W_BF16_EXACT, tile_cfg, stream);
}

int tstar_gemm_bf16w_pre(const float* d_A, const void* d_Wb, float* d_C, const float* d_bias, const float* d_residual, int M, int N,
                         int K, int act, int a_terms, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_Wb && d_C, "tstar_gemm_bf16w_pre: null argument");
    TSTAR_REQUIRE(a_terms == 2 || a_terms == 3, "tstar_gemm_bf16w_pre: a_terms must be 2 or 3");
    GemmArgs g = gemm_args(d_A, reinterpret_cast<const float*>(d_Wb), d_C, d_bias, d_residual, M, N, K, K, N, act);
    g.Wb = static_cast<const __bf16*>(d_Wb);                 // the caller's plane
    g.wmode = a_terms == 2 ? GEMM_W_BF16_2T : GEMM_W_BF16_EXACT;
    g.tile_cfg = tile_cfg;
    return gemm_f32(g, (hipStream_t)stream);
}

int tstar_gemm_bf16w2(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual, int M,
                      int N, int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_bf16w2: null argument");
    return gemm_on_built_planes("tstar_gemm_bf16w2", gemm_args(d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act), GEMM_W_BF16_2T, tile_cfg, stream);
}

int tstar_gemm_f32x3(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual, int M,
                     int N, int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_f32x3: null argument");
    TSTAR_REQUIRE(M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 32 == 0, "tstar_gemm_f32x3: N must be a multiple of 128, K of 32 (include/tstar_hip.h)");
    return gemm_on_built_planes("tstar_gemm_f32x3", gemm_args(d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act), GEMM_W_F32X3, tile_cfg, stream);
}

int tstar_pack_f32x3(const float* d_W, void* d_Wp, int N, int K, void* stream) {
    TSTAR_REQUIRE(d_W && d_Wp, "tstar_pack_f32x3: null argument");
    TSTAR_REQUIRE(N > 0 && K > 0, "tstar_pack_f32x3: empty matrix");
    return pack_weights_x3(d_W, d_Wp, N, K, (hipStream_t)stream);
}

int tstar_gemm_f32x3_pre(const float* d_A, const void* d_Wp, float* d_C, const float* d_bias, const float* d_residual, int M, int N,
                         int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_Wp && d_C, "tstar_gemm_f32x3_pre: null argument");
    TSTAR_REQUIRE(M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 32 == 0, "tstar_gemm_f32x3_pre: N must be a multiple of 128, K of 32 (include/tstar_hip.h)");
    GemmArgs g = gemm_args(d_A, reinterpret_cast<const float*>(d_Wp), d_C, d_bias, d_residual, M, N, K, K, N, act);
    g.Wp = d_Wp;                                             // the caller's planes (tstar_pack_f32x3)
    g.wmode = GEMM_W_F32X3;
    g.tile_cfg = tile_cfg;
    return gemm_f32(g, (hipStream_t)stream);
}

int tstar_gemm_plan(int weights_mode, int M, int N, int ldc, int patch_np, int tile_cfg, int has_packed_w2, int* plan4) {
    TSTAR_REQUIRE(plan4, "tstar_gemm_plan: null argument");
    const GemmPlan p = plan_gemm(gemm_wmode_of(weights_mode), M, N, ldc, patch_np, tile_cfg, has_packed_w2 != 0);
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    plan4[0] = p.kind; plan4[1] = p.m_split; plan4[2] = p.blocks; plan4[3] = p.lds_bytes;
    return TSTAR_OK;
}

// The patch-embedding launch of owl_forward_heads (pos != nullptr, patch_np = np: the PATCH epilogue) on caller-supplied operands, with
// the weight planes of `weights_mode` made as the tstar_gemm_* diagnostics make them.  Every refusal comes before the first allocation.
int tstar_gemm_patch_embed(const float* d_A, const float* d_W, float* d_X, const float* d_pos, int B, int np, int N, int K,
                           int weights_mode, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_X && d_pos, "tstar_gemm_patch_embed: null argument");
    TSTAR_REQUIRE(B >= 1 && np >= 1, "tstar_gemm_patch_embed: B and np must be at least 1");
    TSTAR_REQUIRE((long long)B * (np + 1ll) < (1ll << 31), "tstar_gemm_patch_embed: B * (np + 1) token rows do not fit an int");
    const int wmode = gemm_wmode_of(weights_mode);
    TSTAR_REQUIRE(wmode >= 0, "tstar_gemm_patch_embed: unknown weights_mode (a TSTAR_WEIGHTS_* value)");
    TSTAR_REQUIRE(N > 0 && K > 0 && K % 32 == 0, "tstar_gemm_patch_embed: K must be a positive multiple of 32 (gemm_f32)");
    const int M = B * np;
    const bool has_wq = wmode == GEMM_W_BF16_2T && w2_plane_shape_ok(N, K);     // what gemm_on_built_planes will hand the launch
    const GemmPlan p = plan_gemm(wmode, M, N, N, np, tile_cfg, has_wq);
    if (p.error) { set_error(std::string("tstar_gemm_patch_embed: ") + p.error); return TSTAR_ERR_ARG; }
    GemmArgs g = gemm_args(d_A, d_W, d_X, nullptr, nullptr, M, N, K, K, N, ACT_NONE);
    g.pos = d_pos; g.patch_np = np;
    return gemm_on_built_planes("tstar_gemm_patch_embed", g, wmode, tile_cfg, stream);
}

int tstar_ingest_plan(int op, int nv12, int H, int W, int n, int ow, int oh, int out_aligned4, int video_aligned4, int generic, int nv12_lds,
                      int grid_px, int* plan6) {
    TSTAR_REQUIRE(plan6, "tstar_ingest_plan: null argument");
    const IngestPlan p = plan_ingest(op, nv12 != 0, H, W, n, ow, oh, out_aligned4 != 0, video_aligned4 != 0, IngestOverrides{generic != 0, nv12_lds != 0, grid_px});
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    plan6[0] = p.kind; plan6[1] = p.px; plan6[2] = (int)p.grid_x; plan6[3] = (int)p.grid_y; plan6[4] = p.lds_bytes; plan6[5] = p.lds_pitch;
    return TSTAR_OK;
}

int tstar_layernorm_f32(const float* d_x, float* d_y, const float* d_w, const float* d_b, int rows, int D, void* stream) {
    TSTAR_REQUIRE(d_x && d_y && d_w && d_b, "tstar_layernorm_f32: null argument");
    return layernorm_f32(d_x, d_y, d_w, d_b, rows, D, (hipStream_t)stream);
}

int tstar_attention_f32(const float* d_qkv, float* d_out, int B, int T, int heads, int mode, const uint8_t* d_key_mask,
                        void* stream) {
    TSTAR_REQUIRE(d_qkv && d_out, "tstar_attention_f32: null argument");
    return attention_f32(d_qkv, d_out, B, T, heads, mode, d_key_mask, (hipStream_t)stream);
}

int tstar_draw_boxes(uint8_t* d_images, int B, int H, int W, const float* d_boxes_xyxy, const float* d_scores, void* stream) {
    TSTAR_REQUIRE(d_images && d_boxes_xyxy && d_scores, "tstar_draw_boxes: null argument");
    return draw_boxes(d_images, B, H, W, d_boxes_xyxy, d_scores, V_NP, 0.005f, (hipStream_t)stream);
}

int tstar_draw_boxes_np(uint8_t* d_images, int B, int H, int W, const float* d_boxes_xyxy, const float* d_scores, int np, void* stream) {
    TSTAR_REQUIRE(d_images && d_boxes_xyxy && d_scores, "tstar_draw_boxes_np: null argument");
    TSTAR_REQUIRE(np >= 1, "tstar_draw_boxes_np: np must be positive");
    return draw_boxes(d_images, B, H, W, d_boxes_xyxy, d_scores, np, 0.005f, (hipStream_t)stream);
}

int tstar_attention_x3(const float* d_qkv, float* d_out, int B, int T, int heads, void* stream) {
    TSTAR_REQUIRE(d_qkv && d_out, "tstar_attention_x3: null argument");
    return attention_x3(d_qkv, d_out, B, T, heads, (hipStream_t)stream);
}

int tstar_attention_x3_order(const float* d_qkv, float* d_out, int B, int T, int heads, int order, void* stream) {
    TSTAR_REQUIRE(d_qkv && d_out, "tstar_attention_x3_order: null argument");
    TSTAR_REQUIRE(order == 0 || order == 1, "tstar_attention_x3_order: order must be 0 (linear) or 1 (XCD groups)");
    return attention_x3(d_qkv, d_out, B, T, heads, (hipStream_t)stream, order);
}

int tstar_xcd_group_block(int bid, int ngroups, int gsize) {
    if (bid < 0 || ngroups < 1 || gsize < 1 || bid >= xcd_groups_grid(ngroups, gsize)) return -2;
    return xcd_remap_groups(bid, ngroups, gsize);
}
int tstar_xcd_groups_grid(int ngroups, int gsize) { return ngroups < 1 || gsize < 1 ? -1 : xcd_groups_grid(ngroups, gsize); }

int tstar_attention_split(const float* d_qkv, float* d_out, int B, int T, int heads, void* stream) {
    TSTAR_REQUIRE(d_qkv && d_out, "tstar_attention_split: null argument");
    return attention_split(d_qkv, d_out, B, T, heads, (hipStream_t)stream);
}

}  // extern "C"
