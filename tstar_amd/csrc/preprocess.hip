// Detector pre-processing kernels (byte work, HBM-bound; no MFMA):
//
//  * Pillow-compatible 8-bit BICUBIC resampling to 768x768 (or the handle's input size), exactly as the HF
//    OWL-ViT image processor applies it to the grid image
//    (/root/reference/TStar/interface_heuristic.py:234 -> HF
//    image_processing_pil_owlvit.py:109-119 -> PIL.Image.resize(BICUBIC);
//    algorithm = Pillow src/libImaging/Resample.c precompute_coeffs /
//    normalize_coeffs_8bpc / ImagingResampleHorizontal_8bpc /
//    ImagingResampleVertical_8bpc, restated in SURVEY.md Appendix A2):
//    horizontal pass first, u8 intermediate, 22-bit fixed-point coefficients.
//    The vertical pass is fused with rescale+normalise (a 3x256-entry LUT the
//    host computes with the reference's f64->f32 arithmetic) and with the
//    patch im2col, so the 7 MB fp32 CHW image is never materialised: the
//    output IS the A operand of the patch-embed GEMM.
//
// The searcher's ingest (cv2-style bilinear, frame gather, grid tiling) is ingest.hip.
#include "common.h"
#include "heads.h"
#include <math.h>
#include <vector>

namespace tstar {

// ------------------------------------------------------------------ bicubic tables (host)
static inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int build_bicubic_table(ResampleTable* t, int in_size, int out_size, hipStream_t s) {
    TSTAR_REQUIRE(in_size > 0 && out_size > 0, "bicubic table: sizes must be positive");
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<int> bounds(out_size * 2), coefs((size_t)out_size * ksize, 0);
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            double w = bicubic_filter((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            const double v = k[x] * (double)(1 << 22);
            coefs[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v) : (int)(0.5 + v);
        }
        bounds[xx * 2] = xmin;
        bounds[xx * 2 + 1] = xmax;
    }
    free_table(t);
    t->in_size = in_size; t->out_size = out_size; t->ksize = ksize;
    TSTAR_HIP_CHECK(hipMalloc(&t->d_bounds, bounds.size() * sizeof(int)));
    TSTAR_HIP_CHECK(hipMalloc(&t->d_coefs, coefs.size() * sizeof(int)));
    TSTAR_HIP_CHECK(hipMemcpy(t->d_bounds, bounds.data(), bounds.size() * sizeof(int), hipMemcpyHostToDevice));
    TSTAR_HIP_CHECK(hipMemcpy(t->d_coefs, coefs.data(), coefs.size() * sizeof(int), hipMemcpyHostToDevice));
    (void)s;
    return TSTAR_OK;
}

void free_table(ResampleTable* t) {
    if (t->d_bounds) (void)hipFree(t->d_bounds);
    if (t->d_coefs) (void)hipFree(t->d_coefs);
    t->d_bounds = nullptr; t->d_coefs = nullptr;
}

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= 22;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// out[b,y,ox,:] = clip8(2^21 + sum_i in[b,y,xmin+i,:] * k[ox][i])
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                         int H, int W, int OW, int ksize,
                                                         const int* __restrict__ bounds, const int* __restrict__ coefs,
                                                         size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int ox = (int)(gid % OW);
    const size_t by = gid / OW;                     // b*H + y
    const int xmin = bounds[ox * 2], n = bounds[ox * 2 + 1];
    const uint8_t* src = in + (by * W + xmin) * 3;
    const int* k = coefs + (size_t)ox * ksize;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int i = 0; i < n; ++i) {
        const int kk = k[i];                       // |k| <= 2^22 (1.0 in 22-bit fixed point) and a pixel <= 255: 24-bit operands, so the
        s0 += __mul24(src[i * 3 + 0], kk);         // full-rate v_mad_i32_i24 computes the same 32-bit products as the quarter-rate
        s1 += __mul24(src[i * 3 + 1], kk);         // v_mul_lo_u32 the compiler has to assume
        s2 += __mul24(src[i * 3 + 2], kk);
    }
    uint8_t* dst = out + gid * 3;
    dst[0] = clip8(s0); dst[1] = clip8(s1); dst[2] = clip8(s2);
}

int resample_h_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const ResampleTable& t, hipStream_t s) {
    TSTAR_REQUIRE(t.in_size == W, "resample_h_u8: table does not match the input width");
    const size_t total = (size_t)B * H * t.out_size;
    hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, H, W,
                       t.out_size, t.ksize, t.d_bounds, t.d_coefs, total);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

// in u8 [B,H,OW,3]; vertical pass to OH rows; LUT normalise; write the patch-embed
// A operand for patch size P (patch grid GH x GW = OH / P x OW / P, np = GH GW patches per image, K = 3 P^2):
// row = b*np + (y/P)*GW + x/P, col = c*P^2 + (y%P)*P + x%P  (768 x 768, P = 32: b*576 + (y/32)*24 + x/32, c*1024 + (y%32)*32 + x%32).
// One thread per (b, y, x); x fastest -> 32 consecutive threads write 128 contiguous bytes per channel.
// Round 6: FOUR consecutive x per thread (12 source bytes = three dwords per tap and row instead of twelve byte loads, the products on the
// full-rate v_mad_i32_i24 -- |k| <= 2^22, pixels <= 255: the same 32-bit values --, one float4 store per channel: 4 | P, so the four stay in
// one patch row, 16-byte aligned), the normalisation LUT in LDS.  Same integers, same LUT entries: bit-exact
// (tests/test_gpu_detector.py::test_preprocess_*; P = 16: tests/test_gpu_owl_b16.py).
// SQ768: the checkpoint's own 768 x 768 output with every extent a compile-time constant (the default input size); otherwise
// the output size (OWr x OHr, both multiples of P, so 4 | OWr and the rows of 3 OWr bytes stay dword-aligned) comes at run time
// (tests/test_gpu_owl_input_size.py).
template <int P, bool SQ768>
__global__ __launch_bounds__(256) void resample_v_patchify_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                                  uint8_t* __restrict__ out_u8, int H, int OWr, int OHr, int ksize,
                                                                  const int* __restrict__ bounds,
                                                                  const int* __restrict__ coefs,
                                                                  const float* __restrict__ lut, size_t total4) {
    static_assert(P == 32 || P == 16, "patch sizes 32 and 16");
    constexpr int SH = P == 32 ? 5 : 4, PP = P * P, K = 3 * PP;
    const int OW = SQ768 ? 768 : OWr, OH = SQ768 ? 768 : OHr;
    const int GW = OW >> SH, NP = (OH >> SH) * GW, W4 = OW >> 2;
    __shared__ float slut[768];
    for (int i = threadIdx.x; i < 768; i += 256) slut[i] = lut[i];
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total4) return;
    const int x = (int)(gid % W4) * 4;
    const int y = (int)((gid / W4) % OH);
    const size_t b = gid / ((size_t)W4 * OH);
    const int ymin = bounds[y * 2], n = bounds[y * 2 + 1];
    const uint8_t* src = in + ((b * H + ymin) * OW + x) * 3;           // 12 bytes per tap row, dword-aligned (x % 4 == 0, rows of 3 OW bytes, 4 | OW)
    const int* k = coefs + (size_t)y * ksize;
    int s[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[j][c] = 1 << 21;
    for (int i = 0; i < n; ++i) {
        const int kk = k[i];
        const unsigned* p = reinterpret_cast<const unsigned*>(src + (size_t)i * OW * 3);
        const unsigned w[3] = {p[0], p[1], p[2]};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int byte = 3 * j + c;
                s[j][c] += __mul24((int)((w[byte >> 2] >> ((byte & 3) * 8)) & 0xFFu), kk);
            }
    }
    unsigned v[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = clip8(s[j][c]);
    if (out_u8) store_px4(out_u8 + ((b * OH + y) * OW + x) * 3, v);
    const size_t row = b * NP + (size_t)(y >> SH) * GW + (x >> SH);
    float* o = out + row * K + (y & (P - 1)) * P + (x & (P - 1));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f32x4 q;
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = slut[c * 256 + v[j][c]];
        *reinterpret_cast<f32x4*>(o + c * PP) = q;
    }
}

int resample_v_normalize_patchify(const uint8_t* in, float* out, uint8_t* out_u8, int B, int H, int OW, const ResampleTable& t,
                                  const float* lut, int patch, hipStream_t s) {
    const int OH = t.out_size;
    TSTAR_REQUIRE(t.in_size == H, "resample_v: table must map H -> the output height");
    TSTAR_REQUIRE(patch == 32 || patch == 16, "resample_v: patch size must be 32 or 16");
    TSTAR_REQUIRE(OW > 0 && OH > 0 && OW % patch == 0 && OH % patch == 0, "resample_v: the output size must be a positive multiple of the patch size");
    const size_t total4 = (size_t)B * OH * (OW / 4);                    // four consecutive x per thread
    const dim3 grid((unsigned)((total4 + 255) / 256));
    const bool sq = OW == 768 && OH == 768;
#define TSTAR_RV_LAUNCH(P, SQ) hipLaunchKernelGGL((resample_v_patchify_kernel<P, SQ>), grid, dim3(256), 0, s, in, out, out_u8, H, OW, OH, t.ksize, t.d_bounds, t.d_coefs, lut, total4)
    if (patch == 32) { if (sq) TSTAR_RV_LAUNCH(32, true); else TSTAR_RV_LAUNCH(32, false); }
    else { if (sq) TSTAR_RV_LAUNCH(16, true); else TSTAR_RV_LAUNCH(16, false); }
#undef TSTAR_RV_LAUNCH
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

}  // namespace tstar
