// Image-guided (one-shot) queries: the query-box selection of HF's embed_image_query (modeling_owlvit.py; modeling_owlv2.py is
// the same statements).  For one example image with class embeddings cls [np, 512] (class head dense0, NOT normalised) and
// boxes [np, 4] (cxcywh):
//   corners x0 = cx - 0.5 w, x1 = cx + 0.5 w (y likewise); IoU with the example's query box q = (qx0, qy0, qx1, qy1) (relative
//   xyxy; HF's own is the unit box [0, 0, 1, 1], which is what a null boxes_q stands for) in float32, HF's box_iou /
//   generalized_box_iou in their general form:
//     area_q = (qx1 - qx0)(qy1 - qy0), area = (x1 - x0)(y1 - y0), inter = the product of the extents
//     min(bottom-right corners) - max(top-left corners), each clamped at 0, union = (area_q + area) - inter, iou = inter / union;
//   when EVERY iou is 0: generalized IoU, iou - (enclosing - union) / enclosing, enclosing = the product of the extents
//     max(bottom-right corners) - min(top-left corners), each clamped at 0.
//   With the unit box area_q is exactly 1 and every min / max has the constant 0 or 1 on one side: the bits of the statements
//   this kernel had before it took a box;
//   thr = max * 0.8 (a float32 product); selected = rows with value >= thr (possibly none: a negative maximum);
//   mean = cls.mean(0) over ALL rows; mean_sim[i] = mean . cls[i] for the selected rows;
//   best = the selected row with the smallest mean_sim, lowest index on a tie; the query is cls[best].
// This file is compiled with -ffp-contract=off (tstar_amd/build.py): a fused multiply-add in the IoU arithmetic would change
// the selected set, which is required to be torch's bit for bit.
//
// image_query_select_kernel: ONE workgroup of 256 threads (four wave64) per example image, phases separated by barriers:
//   1. per-row IoU and GIoU into LDS (np <= 3600: 2 x 14400 bytes), per-thread running maxima and a "some iou != 0" flag;
//   2. block reduction (wave shuffles, then the four waves' partials through LDS): the block picks the IoU or the GIoU vector
//      and forms the threshold.  A maximum does not depend on the order it is taken in;
//   3. column sums of cls in a FIXED order that depends neither on n nor on the grid: thread t owns columns 2t and 2t + 1, reads
//      every row as one coalesced 8-byte load, row r goes to accumulator r % 8, the eight are combined as
//      ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)); mean = sum / np into LDS;
//   4. mean_sim of the selected rows, one wave per row (wave w takes rows w, w + 4, ...): 8 floats per lane in the layout of
//      heads.hip's class-embedding read, the same xor-shuffle sum; each wave keeps its running (value, row) minimum -- rows come
//      in increasing order, so a strict "<" keeps the lowest index;
//   5. thread 0 takes the arg-min over the four waves' (value, row), lowest row on equal values;
//   6. the block writes the 512-float row (the input row's bits; zeros when nothing is selected), the best index (-1), the
//      chosen box, the selected count and the status (0 IoU, 1 GIoU fallback used, 2 empty selection).
// No atomics; an image reads rows 0 .. np - 1 of its own block of cls / boxes and nothing else.
#include "common.h"
#include "image_query.h"
#include <float.h>

namespace tstar {

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float wsum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wmax64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void image_query_select_kernel(const float* __restrict__ cls_all, const float* __restrict__ boxes_all,
                                                                 const float* __restrict__ boxes_q, int np,
                                                                 float* __restrict__ embeds, int* __restrict__ best_out, float* __restrict__ box_out,
                                                                 int* __restrict__ nsel_out, int* __restrict__ status_out) {
    __shared__ float s_iou[IMAGE_QUERY_MAX_NP];
    __shared__ float s_giou[IMAGE_QUERY_MAX_NP];
    __shared__ float s_mean[512];
    __shared__ float s_wmax[2][4];
    __shared__ int s_wany[4];
    __shared__ float s_wbestv[4];
    __shared__ int s_wbest[4], s_wcount[4];
    __shared__ int s_best;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* cls = cls_all + (size_t)b * np * 512;
    const float* boxes = boxes_all + (size_t)b * np * 4;

    // ---- 1. IoU / GIoU of every row against the query box
    float qx0 = 0.0f, qy0 = 0.0f, qx1 = 1.0f, qy1 = 1.0f;
    if (boxes_q) { qx0 = boxes_q[(size_t)b * 4 + 0]; qy0 = boxes_q[(size_t)b * 4 + 1]; qx1 = boxes_q[(size_t)b * 4 + 2]; qy1 = boxes_q[(size_t)b * 4 + 3]; }
    const float area_q = (qx1 - qx0) * (qy1 - qy0);
    float mi = -FLT_MAX, mg = -FLT_MAX;
    int any = 0;
    for (int p = tid; p < np; p += 256) {
        const float cx = boxes[(size_t)p * 4 + 0], cy = boxes[(size_t)p * 4 + 1], w = boxes[(size_t)p * 4 + 2], h = boxes[(size_t)p * 4 + 3];
        const float x0 = cx - 0.5f * w, y0 = cy - 0.5f * h, x1 = cx + 0.5f * w, y1 = cy + 0.5f * h;
        const float area = (x1 - x0) * (y1 - y0);
        const float iw = fmaxf(fminf(qx1, x1) - fmaxf(qx0, x0), 0.0f), ih = fmaxf(fminf(qy1, y1) - fmaxf(qy0, y0), 0.0f);
        const float inter = iw * ih;
        const float uni = (area_q + area) - inter;
        const float iou = inter / uni;
        const float ew = fmaxf(fmaxf(qx1, x1) - fminf(qx0, x0), 0.0f), eh = fmaxf(fmaxf(qy1, y1) - fminf(qy0, y0), 0.0f);
        const float enc = ew * eh;
        const float giou = iou - (enc - uni) / enc;
        s_iou[p] = iou;
        s_giou[p] = giou;
        mi = fmaxf(mi, iou);
        mg = fmaxf(mg, giou);
        any |= (iou != 0.0f);
    }
    // ---- 2. maxima and the all-zero flag over the block
    mi = wmax64(mi);
    mg = wmax64(mg);
    any = __any(any);
    if (lane == 0) { s_wmax[0][wave] = mi; s_wmax[1][wave] = mg; s_wany[wave] = any; }
    __syncthreads();
    const bool use_giou = !(s_wany[0] | s_wany[1] | s_wany[2] | s_wany[3]);
    const float* s_val = use_giou ? s_giou : s_iou;
    const int k = use_giou ? 1 : 0;
    const float vmax = fmaxf(fmaxf(s_wmax[k][0], s_wmax[k][1]), fmaxf(s_wmax[k][2], s_wmax[k][3]));
    const float thr = vmax * 0.8f;

    // ---- 3. column mean of cls, fixed order
    {
        float ax[8], ay[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { ax[i] = 0.f; ay[i] = 0.f; }
        const float* col = cls + 2 * tid;
        int r = 0;
        for (; r + 8 <= np; r += 8) {
            f32x2 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x2*>(col + (size_t)(r + i) * 512);
#pragma unroll
            for (int i = 0; i < 8; ++i) { ax[i] += v[i][0]; ay[i] += v[i][1]; }
        }
        for (int i = 0; r + i < np; ++i) {                        // the last np % 8 rows: row r + i is accumulator i (r % 8 == 0)
            const f32x2 v = *reinterpret_cast<const f32x2*>(col + (size_t)(r + i) * 512);
            ax[i] += v[0]; ay[i] += v[1];
        }
        const float sx = ((ax[0] + ax[1]) + (ax[2] + ax[3])) + ((ax[4] + ax[5]) + (ax[6] + ax[7]));
        const float sy = ((ay[0] + ay[1]) + (ay[2] + ay[3])) + ((ay[4] + ay[5]) + (ay[6] + ay[7]));
        s_mean[2 * tid] = sx / (float)np;
        s_mean[2 * tid + 1] = sy / (float)np;
    }
    __syncthreads();

    // ---- 4. mean_sim of the selected rows, one wave per row
    f32x4 m[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) m[i] = *reinterpret_cast<const f32x4*>(s_mean + (i * 64 + lane) * 4);
    float bestv = 0.f;
    int best = -1, count = 0;
    for (int p = wave; p < np; p += 4) {
        if (!(s_val[p] >= thr)) continue;                         // wave-uniform
        ++count;
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(cls + (size_t)p * 512 + (i * 64 + lane) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) d += m[i][e] * c[e];
        }
        d = wsum64(d);
        if (best < 0 || d < bestv) { bestv = d; best = p; }
    }
    if (lane == 0) { s_wbestv[wave] = bestv; s_wbest[wave] = best; s_wcount[wave] = count; }
    __syncthreads();

    // ---- 5. arg-min over the waves: smallest value, lowest row on equal values
    if (tid == 0) {
        float bv = 0.f;
        int bi = -1, n = 0;
        for (int w = 0; w < 4; ++w) {
            n += s_wcount[w];
            const int wi = s_wbest[w];
            if (wi < 0) continue;
            const float wv = s_wbestv[w];
            if (bi < 0 || wv < bv || (wv == bv && wi < bi)) { bv = wv; bi = wi; }
        }
        s_best = bi;
        best_out[b] = bi;
        nsel_out[b] = n;
        status_out[b] = bi < 0 ? 2 : (use_giou ? 1 : 0);
    }
    __syncthreads();

    // ---- 6. the embedding row and its box
    const int bi = s_best;
    f32x2 o; o[0] = 0.f; o[1] = 0.f;
    if (bi >= 0) o = *reinterpret_cast<const f32x2*>(cls + (size_t)bi * 512 + 2 * tid);
    *reinterpret_cast<f32x2*>(embeds + (size_t)b * 512 + 2 * tid) = o;
    if (tid < 4) box_out[(size_t)b * 4 + tid] = bi >= 0 ? boxes[(size_t)bi * 4 + tid] : 0.f;
}

int image_query_select(const float* cls, const float* boxes_cxcywh, const float* boxes_q, int n, int np, const ImageQueryOut& out, hipStream_t s) {
    TSTAR_REQUIRE(cls && boxes_cxcywh && out.embeds && out.best && out.boxes && out.n_selected && out.status, "image_query_select: null argument");
    TSTAR_REQUIRE(n >= 1 && np >= 1 && np <= IMAGE_QUERY_MAX_NP, "image_query_select: n must be positive and np in 1..3600");
    TSTAR_REQUIRE(((uintptr_t)cls & 15) == 0 && ((uintptr_t)out.embeds & 7) == 0, "image_query_select: cls must be 16-byte aligned, embeds 8-byte aligned");
    hipLaunchKernelGGL(image_query_select_kernel, dim3(n), dim3(256), 0, s, cls, boxes_cxcywh, boxes_q, np, out.embeds, out.best, out.boxes, out.n_selected,
                       out.status);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

ImageQueryOut image_query_out_at(void* d_buf, int n) {
    // one device allocation of image_query_out_bytes(n): embeds [n, 512] | boxes [n, 4] | best [n] | n_selected [n] | status [n]
    ImageQueryOut o;
    o.embeds = static_cast<float*>(d_buf);
    o.boxes = o.embeds + (size_t)n * 512;
    o.best = reinterpret_cast<int*>(o.boxes + (size_t)n * 4);
    o.n_selected = o.best + n;
    o.status = o.n_selected + n;
    return o;
}

int image_query_finish(const char* fn, int rc, void* d_buf, const ImageQueryOut& o, int n, float* h_embeds, int32_t* h_best, float* h_boxes,
                       int32_t* h_n_selected, int32_t* h_status, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (!rc) {
        e = hipMemcpyAsync(h_embeds, o.embeds, (size_t)n * 512 * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_boxes, o.boxes, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_best, o.best, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_n_selected, o.n_selected, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_status, o.status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);             // also before the staging buffer is freed after a failed launch
    if (e == hipSuccess) e = e2;
    (void)hipFree(d_buf);
    if (!rc && e != hipSuccess) { set_error(std::string(fn) + ": " + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    return rc;
}

}  // namespace tstar
