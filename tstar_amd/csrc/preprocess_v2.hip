// OWLv2 detector pre-processing: HF's Owlv2ImageProcessorPil ("the original implementation" path) with its exact bits.
//
// What HF does to one u8 image [H, W, 3] (image_processing_pil_owlv2.py): rescale by 1/255 (float64 product, rounded to
// float32) -> zero-pad bottom / right to the square of side S = max(H, W) -> scipy.ndimage.gaussian_filter (anti-aliasing;
// sigma = max(0, (S / out - 1) / 2) per axis, an axis with sigma <= 1e-15 is skipped; axis 0 first, float64 accumulation,
// one rounding to float32 after each axis, "mirror" extension) -> scipy.ndimage.zoom(order=1, mode="mirror", grid_mode=True)
// (float64, four taps, rounded to float32) -> clip to [min, max] of the padded float32 square -> (z - mean) / std in float32.
//
// Nothing of that is written to HBM at full resolution: the output IS the patch-embed GEMM's A operand (im2col, P = 16).
//   * direct form (no axis shrinks): one thread per four consecutive output pixels, the four taps of each straight from the u8
//     source through the 256-entry rescale table in LDS, one 16-byte store per channel;
//   * filtered form: a workgroup owns an output tile, loads the tile's source window as float32 into LDS, runs the row-axis
//     Gaussian for the source rows the zoom reads, then the column-axis Gaussian for the source columns it reads (each pass
//     rounds to float32 in LDS), then zoom, clip, normalise and the im2col store;
//   * the clip bounds are the per-image min / max of the u8 source (a small reduction kernel), mapped through the table; the
//     lower bound is 0 whenever the image was padded (H != W).
// This file is compiled with -ffp-contract=off (tstar_amd/build.py PER_FILE): a fused multiply-add changes the bits, on the
// device and in the host's float64 tables alike.
#include "../../include/tstar_hip.h"
#include "common.h"
#include "preprocess_v2.h"
#include <limits.h>
#include <math.h>
#include <vector>

namespace tstar {

// ------------------------------------------------------------------------------------------------------------ policy (host)
Owlv2Axis owlv2_axis(int S, int out) {
    Owlv2Axis a;
    a.factor = (double)S / (double)out;
    const double s = (a.factor - 1.0) / 2.0;
    a.sigma = s > 0.0 ? s : 0.0;
    a.radius = a.sigma <= 1e-15 ? -1 : (int)(4.0 * a.sigma + 0.5);
    return a;
}

static inline int mirror_index(int p, int S) { p = p < 0 ? -p : p; return p > S - 1 ? 2 * (S - 1) - p : p; }

void owlv2_zoom_tap(int S, int out, int j, int* i0, int* i1, double* t) {
    const double f = (double)S / (double)out;
    const double cc = ((double)j + 0.5) * f - 0.5;
    double c = fabs(cc);
    if (c > (double)(S - 1)) c = 2.0 * (double)(S - 1) - c;
    const double fl = floor(c);
    *i0 = (int)fl;
    *t = c - fl;
    *i1 = mirror_index(*i0 + 1, S);
}

void owlv2_axis_window(int S, int out, int tile, int k, int radius, int* lo, int* n) {
    int mn = INT_MAX, mx = -1;
    for (int j = k * tile; j < (k + 1) * tile && j < out; ++j) {
        int i0, i1; double t;
        owlv2_zoom_tap(S, out, j, &i0, &i1, &t);
        mn = i0 < mn ? i0 : mn; mn = i1 < mn ? i1 : mn;
        mx = i0 > mx ? i0 : mx; mx = i1 > mx ? i1 : mx;
    }
    const int r = radius > 0 ? radius : 0;
    const int a = mn - r > 0 ? mn - r : 0, b = mx + r < S - 1 ? mx + r : S - 1;
    *lo = a; *n = b - a + 1;
}

static int max_window(int S, int out, int tile, int radius) {
    int best = 0;
    for (int k = 0; k * tile < out; ++k) {
        int lo, n;
        owlv2_axis_window(S, out, tile, k, radius, &lo, &n);
        best = n > best ? n : best;
    }
    return best;
}

// LDS of the filtered form, in floats: A [win_h][win_w] the source window; B [2 th][win_w | 1] after the row pass (two tap
// rows per output row); C [2 th][2 tw | 1] after the column pass, in A's place (A is dead by then).
static long long filtered_lds_floats(int th, int tw, int win_h, int win_w) {
    const long long a = (long long)win_h * win_w, c = 2LL * th * ((2 * tw) | 1), b = 2LL * th * (win_w | 1);
    return (a > c ? a : c) + b;
}

Owlv2Plan plan_owlv2_preprocess(int H, int W, int out_h, int out_w) {
    Owlv2Plan p{};
    if (H < 1 || W < 1 || (H < 2 && W < 2)) { p.error = "owlv2 pre-processing: the image must be at least two pixels on its longer side"; return p; }
    if (out_h < 16 || out_w < 16 || out_h % 16 || out_w % 16) { p.error = "owlv2 pre-processing: the output size must be a positive multiple of 16 per side"; return p; }
    const int S = H > W ? H : W;
    const Owlv2Axis ay = owlv2_axis(S, out_h), ax = owlv2_axis(S, out_w);
    p.radius_y = ay.radius; p.radius_x = ax.radius;
    if (ay.radius < 0 && ax.radius < 0) {
        p.form = OWLV2_FORM_DIRECT;
        p.tile_h = 1; p.tile_w = 4; p.win_h = 2; p.win_w = 2;
        p.lds_bytes = 256 * (int)sizeof(float);
        const long long groups = (long long)out_h * (out_w / 4);
        p.grid_x = (int)((groups + 255) / 256); p.grid_y = 1;
        return p;
    }
    if (ay.radius > S - 1 || ax.radius > S - 1) { p.error = "owlv2 pre-processing: the shrink factor is too large for the image (the filter is wider than the image)"; return p; }
    static const int tiles[][2] = {{16, 32}, {16, 16}, {8, 16}, {8, 8}, {4, 8}, {4, 4}, {2, 4}, {2, 2}, {1, 2}, {1, 1}};
    p.form = OWLV2_FORM_FILTERED;
    for (int limit : {OWLV2_LDS_TARGET, OWLV2_LDS_LIMIT}) {
        for (const auto& t : tiles) {
            const int wh = max_window(S, out_h, t[0], ay.radius), ww = max_window(S, out_w, t[1], ax.radius);
            const long long bytes = filtered_lds_floats(t[0], t[1], wh, ww) * (long long)sizeof(float) + 1024;      // + the 256-entry table
            if (bytes <= limit) {
                p.tile_h = t[0]; p.tile_w = t[1]; p.win_h = wh; p.win_w = ww; p.lds_bytes = (int)bytes;
                p.grid_x = (out_w + t[1] - 1) / t[1]; p.grid_y = (out_h + t[0] - 1) / t[0];
                return p;
            }
        }
    }
    p.error = "owlv2 pre-processing: the source window of a single output pixel does not fit the 160 KiB of LDS (the shrink factor is too large)";
    return p;
}

// ------------------------------------------------------------------------------------------------------------- tables (host)
// numpy's pairwise float64 sum (numpy/_core/src/umath/loops_utils.h DOUBLE_pairwise_sum), which _gaussian_kernel1d's
// phi_x.sum() runs
static double np_pairwise_sum(const double* a, size_t n) {
    if (n < 8) {
        double res = 0.0;
        for (size_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        size_t i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

void free_owlv2_axis_table(Owlv2AxisTable* t) {
    void* ptrs[] = {t->d_i0, t->d_i1, t->d_t, t->d_gw};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    *t = Owlv2AxisTable{};
}

void owlv2_axis_host(int S, int out, std::vector<int>& i0, std::vector<int>& i1, std::vector<double>& tt, std::vector<double>& gw) {
    const Owlv2Axis a = owlv2_axis(S, out);
    i0.resize(out); i1.resize(out); tt.resize(out);
    for (int j = 0; j < out; ++j) owlv2_zoom_tap(S, out, j, &i0[j], &i1[j], &tt[j]);
    const int lw = a.radius > 0 ? a.radius : 0;
    gw.assign(lw + 1, 1.0);
    if (a.radius > 0) {                                     // scipy.ndimage._gaussian_kernel1d(sigma, 0, lw)
        std::vector<double> phi(2 * lw + 1);
        const double e = -0.5 / (a.sigma * a.sigma);
        for (int x = -lw; x <= lw; ++x) phi[x + lw] = exp(e * (double)(x * x));
        const double sum = np_pairwise_sum(phi.data(), phi.size());
        for (int k = 0; k <= lw; ++k) gw[k] = phi[k] / sum;
    }
}

int build_owlv2_axis_table(Owlv2AxisTable* t, int S, int out, const std::vector<double>* gw_given) {
    TSTAR_REQUIRE(S >= 2 && out >= 1, "owlv2 axis table: sizes must be positive");
    const Owlv2Axis a = owlv2_axis(S, out);
    std::vector<int> i0, i1;
    std::vector<double> tt, gw;
    owlv2_axis_host(S, out, i0, i1, tt, gw);
    if (gw_given) {
        TSTAR_REQUIRE(gw_given->size() == gw.size(), "owlv2 axis table: the given Gaussian weights must hold radius + 1 values");
        gw = *gw_given;
    }
    free_owlv2_axis_table(t);
    t->S = S; t->out = out; t->radius = a.radius;
    TSTAR_HIP_CHECK(hipMalloc(&t->d_i0, out * sizeof(int)));
    TSTAR_HIP_CHECK(hipMalloc(&t->d_i1, out * sizeof(int)));
    TSTAR_HIP_CHECK(hipMalloc(&t->d_t, out * sizeof(double)));
    TSTAR_HIP_CHECK(hipMalloc(&t->d_gw, gw.size() * sizeof(double)));
    TSTAR_HIP_CHECK(hipMemcpy(t->d_i0, i0.data(), out * sizeof(int), hipMemcpyHostToDevice));
    TSTAR_HIP_CHECK(hipMemcpy(t->d_i1, i1.data(), out * sizeof(int), hipMemcpyHostToDevice));
    TSTAR_HIP_CHECK(hipMemcpy(t->d_t, tt.data(), out * sizeof(double), hipMemcpyHostToDevice));
    TSTAR_HIP_CHECK(hipMemcpy(t->d_gw, gw.data(), gw.size() * sizeof(double), hipMemcpyHostToDevice));
    return TSTAR_OK;
}

// ------------------------------------------------------------------------------------------------------------------ kernels
struct AxisDev {
    const int* i0;
    const int* i1;
    const double* t;
    const double* gw;
    int radius;                // >= 0 (a skipped axis runs as radius 0, weight 1.0: x * 1.0 is x)
};

__global__ void minmax_init_kernel(int* __restrict__ mm, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { mm[2 * b] = 255; mm[2 * b + 1] = 0; }
}

// mm[b] = (min, max) of the n bytes of image b; gridDim = (blocks per image, B).  16-byte loads on the aligned interior.
__global__ __launch_bounds__(256) void minmax_u8_kernel(const uint8_t* __restrict__ in, size_t n, int* __restrict__ mm) {
    const uint8_t* p = in + (size_t)blockIdx.y * n;
    size_t head = (16 - (size_t)((uintptr_t)p & 15)) & 15;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 16, tail = head + nvec * 16;
    unsigned lo = 255u, hi = 0u;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    const uint4* v = reinterpret_cast<const uint4*>(p + head);
    for (size_t i = tid; i < nvec; i += nthr) {
        const uint4 q = v[i];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int sft = 0; sft < 32; sft += 8) {
                const unsigned u = (w[k] >> sft) & 0xFFu;
                lo = u < lo ? u : lo; hi = u > hi ? u : hi;
            }
    }
    for (size_t i = tid; i < head + (n - tail); i += nthr) {
        const unsigned u = p[i < head ? i : tail + (i - head)];
        lo = u < lo ? u : lo; hi = u > hi ? u : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[2 * blockIdx.y], (int)lo);
        atomicMax(&mm[2 * blockIdx.y + 1], (int)hi);
    }
}

__device__ __forceinline__ int mir(int p, int S) { p = p < 0 ? -p : p; return p > S - 1 ? 2 * (S - 1) - p : p; }

// the four taps in scipy's order, float64, one rounding; then clip and normalise in float32
__device__ __forceinline__ float zoom_finish(float v00, float v01, float v10, float v11, double wy0, double wy1, double wx0, double wx1,
                                             float lo, float hi, float mean, float stdv) {
    double z = ((double)v00 * wy0) * wx0;
    z = z + ((double)v01 * wy0) * wx1;
    z = z + ((double)v10 * wy1) * wx0;
    z = z + ((double)v11 * wy1) * wx1;
    float r = (float)z;
    r = r < lo ? lo : r;
    r = r > hi ? hi : r;
    return (r - mean) / stdv;
}

// Direct form.  One thread per (b, y, four consecutive x); x fastest, so a wave writes 64 x 16 bytes per channel in runs of one
// patch row (64 bytes).  Source samples outside the image (the zero padding of the square) are 0.
__global__ __launch_bounds__(256) void owlv2_direct_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, const int* __restrict__ mm,
                                                           int H, int W, int OH, int OW, AxisDev ay, AxisDev ax,
                                                           const float* __restrict__ norm, size_t total4) {
    __shared__ float slut[256];
    slut[threadIdx.x] = norm[threadIdx.x];
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total4) return;
    const int W4 = OW >> 2, GW = OW >> 4, NP = (OH >> 4) * GW;
    const int x = (int)(gid % W4) * 4;
    const int y = (int)((gid / W4) % OH);
    const size_t b = gid / ((size_t)W4 * OH);
    const float lo = H != W ? 0.0f : slut[mm[2 * b]], hi = slut[mm[2 * b + 1]];
    const int y0 = ay.i0[y], y1 = ay.i1[y];
    const double ty = ay.t[y], wy0 = 1.0 - ty, wy1 = ty;
    const uint8_t* img = in + b * (size_t)H * W * 3;
    const bool in0 = y0 < H, in1 = y1 < H;
    const uint8_t* r0 = img + (size_t)y0 * W * 3;
    const uint8_t* r1 = img + (size_t)y1 * W * 3;
    f32x4 q[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x0 = ax.i0[x + j], x1 = ax.i1[x + j];
        const double tx = ax.t[x + j], wx0 = 1.0 - tx, wx1 = tx;
        const bool c0 = x0 < W, c1 = x1 < W;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v00 = in0 && c0 ? slut[r0[x0 * 3 + c]] : 0.0f, v01 = in0 && c1 ? slut[r0[x1 * 3 + c]] : 0.0f;
            const float v10 = in1 && c0 ? slut[r1[x0 * 3 + c]] : 0.0f, v11 = in1 && c1 ? slut[r1[x1 * 3 + c]] : 0.0f;
            q[c][j] = zoom_finish(v00, v01, v10, v11, wy0, wy1, wx0, wx1, lo, hi, norm[256 + c], norm[259 + c]);
        }
    }
    const size_t row = b * NP + (size_t)(y >> 4) * GW + (x >> 4);
    float* o = out + row * 768 + (y & 15) * 16 + (x & 15);
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * 256) = q[c];
}

// Filtered form.  Block (tile x, tile y, image); one channel at a time through three LDS stages:
//   A [ny][pa]        the tile's source window as float32 (0 outside the image), pa = the plan's win_w;
//   Bq [2 th][pb]     row-axis Gaussian of the two tap rows of every output row of the tile, over the window's columns;
//   C [2 th][pc]      column-axis Gaussian of the two tap columns of every output column, in A's place.
// Bank conflicts (64 banks of 4 bytes): the row pass walks the window columns with consecutive lanes (reads of A and writes of
// Bq at consecutive addresses: conflict-free at any pitch).  The column pass reads Bq along a ROW (column +- k of tap columns
// that lie a factor apart), so consecutive lanes take consecutive ROWS q instead: their addresses differ by pb = win_w | 1,
// which is odd, hence 2 th <= 64 rows fall into distinct banks; the writes of C differ by pc = 2 tw | 1, odd as well.  The zoom
// reads C at stride 2 along a row (a two-way conflict at worst) and is the smallest of the three stages.
__global__ __launch_bounds__(256) void owlv2_filtered_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, const int* __restrict__ mm,
                                                             int H, int W, int S, int OH, int OW, int th, int tw, int pa, int b_off,
                                                             AxisDev ay, AxisDev ax, const float* __restrict__ norm) {
    extern __shared__ float sm[];
    __shared__ float slut[256];
    float* A = sm;
    float* C = sm;
    float* Bq = sm + b_off;
    const int pb = pa | 1, pc = (2 * tw) | 1;
    const int tid = threadIdx.x;
    slut[tid] = norm[tid];
    const int ty0 = blockIdx.y * th, tx0 = blockIdx.x * tw;
    const size_t b = blockIdx.z;
    // the tile's window: its zoom taps, widened by the radius, cut at the square's edges (owlv2_axis_window)
    int ylo = INT_MAX, yhi = -1, xlo = INT_MAX, xhi = -1;
    for (int l = 0; l < th; ++l) {
        const int j = ty0 + l < OH ? ty0 + l : OH - 1;
        const int a = ay.i0[j], c = ay.i1[j];
        ylo = min(ylo, min(a, c)); yhi = max(yhi, max(a, c));
    }
    for (int l = 0; l < tw; ++l) {
        const int j = tx0 + l < OW ? tx0 + l : OW - 1;
        const int a = ax.i0[j], c = ax.i1[j];
        xlo = min(xlo, min(a, c)); xhi = max(xhi, max(a, c));
    }
    const int ry = ay.radius, rx = ax.radius;
    ylo = max(0, ylo - ry); yhi = min(S - 1, yhi + ry);
    xlo = max(0, xlo - rx); xhi = min(S - 1, xhi + rx);
    const int ny = yhi - ylo + 1, nx = xhi - xlo + 1;
    const uint8_t* img = in + b * (size_t)H * W * 3;
    const int GW = OW >> 4, NP = (OH >> 4) * GW;
    for (int ch = 0; ch < 3; ++ch) {
        __syncthreads();                                    // slut ready; the previous channel's C fully read
        // each wave takes eight window rows per step, its lanes the columns: eight independent byte loads in flight per lane
        // (the window load is latency-bound: one load per trip left the workgroup waiting on HBM / L2 most of its life)
        for (int wy0 = (tid >> 6) * 8; wy0 < ny; wy0 += 32) {
            for (int wx = tid & 63; wx < nx; wx += 64) {
                const int gx = xlo + wx;
                unsigned v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int gy = ylo + wy0 + r;
                    v[r] = wy0 + r < ny && gy < H && gx < W ? (unsigned)img[((size_t)gy * W + gx) * 3 + ch] : 256u;
                }
#pragma unroll
                for (int r = 0; r < 8; ++r)
                    if (wy0 + r < ny) A[(wy0 + r) * pa + wx] = v[r] < 256u ? slut[v[r]] : 0.0f;
            }
        }
        __syncthreads();
        for (int i = tid; i < 2 * th * nx; i += 256) {      // row-axis pass
            const int q = i / nx, c = i - q * nx;
            const int j = ty0 + (q >> 1) < OH ? ty0 + (q >> 1) : OH - 1;
            const int R = (q & 1) ? ay.i1[j] : ay.i0[j];
            const float* col = A + (R - ylo) * pa + c;
            double acc = (double)col[0] * ay.gw[ry];
            if (R - ry >= 0 && R + ry <= S - 1) {           // away from the square's edges: no mirroring
                for (int k = ry; k >= 1; --k) acc = acc + ((double)col[-k * pa] + (double)col[k * pa]) * ay.gw[ry - k];
            } else {
                for (int k = ry; k >= 1; --k)
                    acc = acc + ((double)col[(mir(R - k, S) - R) * pa] + (double)col[(mir(R + k, S) - R) * pa]) * ay.gw[ry - k];
            }
            Bq[q * pb + c] = (float)acc;
        }
        __syncthreads();
        for (int i = tid; i < 2 * th * 2 * tw; i += 256) {  // column-axis pass, consecutive lanes on consecutive rows
            const int cc = i / (2 * th), q = i - cc * (2 * th);
            const int j = tx0 + (cc >> 1) < OW ? tx0 + (cc >> 1) : OW - 1;
            const int X = (cc & 1) ? ax.i1[j] : ax.i0[j];
            const float* row = Bq + q * pb - xlo;
            double acc = (double)row[X] * ax.gw[rx];
            if (X - rx >= 0 && X + rx <= S - 1) {
                for (int k = rx; k >= 1; --k) acc = acc + ((double)row[X - k] + (double)row[X + k]) * ax.gw[rx - k];
            } else {
                for (int k = rx; k >= 1; --k)
                    acc = acc + ((double)row[mir(X - k, S)] + (double)row[mir(X + k, S)]) * ax.gw[rx - k];
            }
            C[q * pc + cc] = (float)acc;
        }
        __syncthreads();
        const float lo = H != W ? 0.0f : slut[mm[2 * b]], hi = slut[mm[2 * b + 1]];
        const float mean = norm[256 + ch], stdv = norm[259 + ch];
        for (int i = tid; i < th * tw; i += 256) {
            const int ly = i / tw, lx = i - ly * tw, y = ty0 + ly, x = tx0 + lx;
            if (y >= OH || x >= OW) continue;
            const double tyv = ay.t[y], txv = ax.t[x];
            const float* c0 = C + (2 * ly) * pc + 2 * lx;
            const float* c1 = c0 + pc;
            const float r = zoom_finish(c0[0], c0[1], c1[0], c1[1], 1.0 - tyv, tyv, 1.0 - txv, txv, lo, hi, mean, stdv);
            const size_t prow = b * NP + (size_t)(y >> 4) * GW + (x >> 4);
            out[prow * 768 + ch * 256 + (y & 15) * 16 + (x & 15)] = r;
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- launcher
int owlv2_preprocess(const uint8_t* in, float* out, int* d_minmax, int B, int H, int W, int out_h, int out_w,
                     const Owlv2AxisTable& ty, const Owlv2AxisTable& tx, const float* d_norm, hipStream_t s, int* form_ran) {
    const Owlv2Plan p = plan_owlv2_preprocess(H, W, out_h, out_w);
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    const int S = H > W ? H : W;
    TSTAR_REQUIRE(B >= 1 && in && out && d_minmax && d_norm, "owlv2_preprocess: null argument or empty batch");
    TSTAR_REQUIRE(ty.S == S && tx.S == S && ty.out == out_h && tx.out == out_w, "owlv2_preprocess: the axis tables do not match the image");
    TSTAR_REQUIRE(ty.radius == p.radius_y && tx.radius == p.radius_x, "owlv2_preprocess: the axis tables do not match the plan");
    const size_t n = (size_t)H * W * 3;
    hipLaunchKernelGGL(minmax_init_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, d_minmax, B);
    const size_t per_block = 256 * 16 * 8;                   // eight 16-byte loads per thread
    unsigned nblk = (unsigned)((n + per_block - 1) / per_block);
    nblk = nblk < 1 ? 1 : (nblk > 256 ? 256 : nblk);
    hipLaunchKernelGGL(minmax_u8_kernel, dim3(nblk, B), dim3(256), 0, s, in, n, d_minmax);
    const AxisDev ay{ty.d_i0, ty.d_i1, ty.d_t, ty.d_gw, ty.radius > 0 ? ty.radius : 0};
    const AxisDev ax{tx.d_i0, tx.d_i1, tx.d_t, tx.d_gw, tx.radius > 0 ? tx.radius : 0};
    if (p.form == OWLV2_FORM_DIRECT) {
        const size_t total4 = (size_t)B * out_h * (out_w / 4);
        hipLaunchKernelGGL(owlv2_direct_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, in, out, d_minmax, H, W, out_h, out_w,
                           ay, ax, d_norm, total4);
    } else {
        TSTAR_REQUIRE(B <= 65535, "owlv2_preprocess: at most 65535 images per launch");
        const int dyn = p.lds_bytes - 1024;                  // the plan counts the kernel's static table
        if (dyn > 48 * 1024) { const int rc = ensure_dyn_lds((const void*)owlv2_filtered_kernel, OWLV2_LDS_LIMIT - 1024); if (rc) return rc; }
        const long long a = (long long)p.win_h * p.win_w, c = 2LL * p.tile_h * ((2 * p.tile_w) | 1);
        const int b_off = (int)(a > c ? a : c);
        hipLaunchKernelGGL(owlv2_filtered_kernel, dim3(p.grid_x, p.grid_y, B), dim3(256), (size_t)dyn, s, in, out, d_minmax, H, W, S,
                           out_h, out_w, p.tile_h, p.tile_w, p.win_w, b_off, ay, ax, d_norm);
    }
    TSTAR_HIP_CHECK(hipGetLastError());
    if (form_ran) *form_ran = p.form;
    return TSTAR_OK;
}

}  // namespace tstar
