// Searcher ingest kernels of the T* hot path (byte work, HBM-bound; no MFMA):
//
//  * OpenCV-style INTER_LINEAR 8-bit resize (11-bit coefficients, the
//    HResizeLinear / VResizeLinear<uchar,int,short> fixed-point formulas) for
//    the three cv2.resize call sites of the searcher
//    (the reference's TStar/interface_searcher.py:362 -> 800x380, :186 ->
//    200x95, :403 -> 600x285), fused with the frame gather (decord get_batch,
//    :168-169, replaced by a resident decoded-frame store) and the grid tiling
//    (:187-188).  cv2 is not importable in the build container: this bilinear
//    is the build's own definition ("parity unpinned").
//  * The frame-store conversions next to it: NV12 -> RGB at native resolution
//    and planar I420 -> NV12.
//
// Host side, in this order: ONE statement of the cv2 coefficient loop (linear_tap), ONE cache of device tables keyed by a
// named layout (TabKind), ONE pure function that picks the kernel form (plan_ingest, ingest.h).  The launchers at the end
// only check arguments, ask the plan, fetch the tables its kind needs and launch.
#include "common.h"
#include "ingest.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <compare>
#include <map>
#include <mutex>
#include <vector>

namespace tstar {

// ------------------------------------------------------------------ OpenCV-style bilinear: taps and tables (host)
// Per output index d of an axis: (first source index s0, second source index s1, w0, w1), w in 11-bit fixed point, in the
// same float/double arithmetic as cv::resize's coefficient loop (cvRound = round half even, saturate_cast<short>).  Every
// table below, plain or fused, and the LDS region size are derived from these entries and from nothing else.
static int4 linear_tap(int src, int dst, int d) {
    const double scale = (double)src / dst;
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    auto w11 = [](float v) { const int r = (int)lrintf(v); return r < -32768 ? -32768 : (r > 32767 ? 32767 : r); };
    return make_int4(s, s + 1 < src ? s + 1 : src - 1, w11((1.f - f) * 2048.f), w11(f * 2048.f));
}
static std::vector<int4> linear_taps(int src, int dst) {
    std::vector<int4> h(dst);
    for (int d = 0; d < dst; ++d) h[d] = linear_tap(src, dst, d);
    return h;
}

// v_perm_b32 selector: source byte `lo` into bits 0-7, source byte `hi` into bits 16-23, zeros between
__host__ __device__ constexpr unsigned perm_sel(unsigned lo, unsigned hi) { return lo | 0x0C00u | (hi << 16) | 0x0C000000u; }

// Table layouts.  An X entry describes the two taps of one bilinear sample (fused_x_sample / fused_x_sample_nv12 below); a Y
// entry carries source row offsets in bytes and the vertical weights << 12 (vmix).  Single = one resize src -> dst; two-step
// = src -> mid -> dst (the grid: frame -> 4x cell -> cell): per output index the intermediate samples A, B and the final pair F.
enum TabKind {
    TAB_TAPS,      // one int4 linear_tap per output index (generic kernels, NV12 through LDS)
    TAB_RGB_X,     // single X, RGB: one uint4 {off, sel, w, 0} per column
    // single X, RGB, as THREE ARRAYS (off[], sel[], w[], each padded to a multiple of 4 entries): a lane of the 4-pixel kernel
    // reads its four consecutive entries of one field as ONE 16-byte load, and the 64 lanes of a wave read 1 KB contiguously.
    // The array-of-uint4 layout (TAB_RGB_X) made each of a lane's four entry loads touch a different 64-byte line per lane --
    // 64 lines per wave instruction, 256 per four pixels (round 4: 91.6 -> 74.0 us for 180 verification frames, 2.37 -> 2.93 TB/s)
    TAB_RGB_X3,
    TAB_RGB_Y,     // single Y, RGB: one uint4 {row0 bytes, row1 bytes, b0 << 12, b1 << 12} per row (row pitch 3 W)
    TAB_RGB_X2,    // two-step X, RGB: two uint4 {offA, selA, wA, offB} {selB, wB, wF, 0}
    TAB_RGB_Y2,    // two-step Y, RGB: three uint4 {r0a, r0b, r1a, r1b} {A.b0, A.b1, B.b0, B.b1} {F.b0, F.b1, 0, 0} (weights << 12)
    TAB_NV12_X,    // single X, NV12: one uint4 {oY | oC << 16, selYU.L, selYU.R, w} per column
    TAB_NV12_Y,    // single Y, NV12: two uint4 {luma row 0, luma row 1, chroma row 0, chroma row 1} {b0 << 12, b1 << 12, 0, 0}
    TAB_NV12_X2,   // two-step X, NV12: three uint4 {A as TAB_NV12_X} {B} {wF, 0, 0, 0}
    TAB_NV12_Y2,   // two-step Y, NV12: four uint4: luma rows {r0a, r0b, r1a, r1b}, chroma rows (frame-relative bytes), A | B weights, F weights
};
struct TabKey {
    int kind, src, mid, dst, W, H;
    auto operator<=>(const TabKey&) const = default;
};
static std::map<TabKey, const void*> g_tabs;      // device copies, resident for the life of the process
static std::mutex g_tab_mu;

// the device copy of the table `build` makes on the host, made once per key
template <class T, class Build>
static int cached_table(const TabKey& key, Build&& build, const T** out) {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    auto it = g_tabs.find(key);
    if (it == g_tabs.end()) {
        const std::vector<T> h = build();
        void* d = nullptr;
        TSTAR_HIP_CHECK(hipMalloc(&d, h.size() * sizeof(T)));
        TSTAR_HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        it = g_tabs.emplace(key, d).first;
    }
    *out = static_cast<const T*>(it->second);
    return TSTAR_OK;
}
static int get_lintab(int src, int dst, const int4** out) {
    return cached_table(TabKey{TAB_TAPS, src, 0, dst, 0, 0}, [&] { return linear_taps(src, dst); }, out);
}

// Source pixel fetch.  RGB frames: interleaved u8 [H, W, 3].  NV12 frames: u8 [H*3/2, W] = luma plane
// followed by the interleaved half-resolution UV plane; converted on the fly with the BT.601
// limited-range integer matrix (298/409/100/208/516, >> 8) and nearest chroma (each 2x2 block shares
// one U,V pair) -- the build's own definition (the reference receives RGB from decord/swscale and never
// sees NV12).  NV12 halves the bytes per resident frame (345,600 B vs 691,200 B at 360x640).
struct Rgb { int r, g, b; };
__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// unaligned wide load (the hardware serves it; one instruction instead of six byte loads)
struct __attribute__((packed)) PackedU64 { uint64_t v; };

struct SrcRGB {
    const uint8_t* p; int W, H;
    __device__ __forceinline__ Rgb at(int x, int y) const {
        const uint8_t* q = p + ((size_t)y * W + x) * 3;
        return Rgb{q[0], q[1], q[2]};
    }
    // pixels x and x + 1 of row y from ONE 8-byte load; caller guarantees x <= W - 3 (the load stays inside the row)
    static constexpr bool kWidePair = true;
    __device__ __forceinline__ void pair(int x, int y, Rgb& a, Rgb& b) const {
        const uint64_t v = reinterpret_cast<const PackedU64*>(p + ((size_t)y * W + x) * 3)->v;
        a = Rgb{(int)(v & 0xFF), (int)((v >> 8) & 0xFF), (int)((v >> 16) & 0xFF)};
        b = Rgb{(int)((v >> 24) & 0xFF), (int)((v >> 32) & 0xFF), (int)((v >> 40) & 0xFF)};
    }
    static __device__ __forceinline__ size_t frame_bytes(int H, int W) { return (size_t)H * W * 3; }
};
struct SrcNV12 {
    const uint8_t* p; int W, H;
    __device__ __forceinline__ Rgb at(int x, int y) const {
        const int c = (int)p[(size_t)y * W + x] - 16;
        const uint8_t* uv = p + (size_t)H * W + (size_t)(y >> 1) * W + (x & ~1);
        const int d = (int)uv[0] - 128, e = (int)uv[1] - 128;
        return Rgb{clip255((298 * c + 409 * e + 128) >> 8), clip255((298 * c - 100 * d - 208 * e + 128) >> 8),
                   clip255((298 * c + 516 * d + 128) >> 8)};
    }
    static constexpr bool kWidePair = false;     // measured: a two-pixel form (u16 luma + u32 chroma) is slower here
    __device__ __forceinline__ void pair(int, int, Rgb&, Rgb&) const {}
    static __device__ __forceinline__ size_t frame_bytes(int H, int W) { return (size_t)H * W * 3 / 2; }
};

// ------------------------------------------------------------------ RGB fast path of the two kernels below
// The generic kernels (further down) spend ~500 executed instructions per output pixel, most of them overhead: three runtime integer
// divisions for the index decode, 64-bit address arithmetic per tap, quarter-rate 32-bit multiplies (the compiler cannot
// know the operands are small), byte extraction by shift / mask, two dependent levels of table loads.  For interleaved
// RGB sources the same arithmetic (bit for bit: OpenCV's HResizeLinear / VResizeLinear fixed-point formulas) is restated
// around what the hardware does in one instruction:
//  * the host folds the index tables into one entry per output column / row (FUSED tables): per bilinear sample the BYTE
//    offset of an 8-byte window inside the source row that holds both taps (clamped to the row: the last window ends at
//    the row's last byte, so nothing is read outside the frame), a v_perm_b32 selector that drops the two taps' channel-0
//    bytes into the halves of a dword (channels 1 / 2: selector + 0x00010001 / 0x00020002), the two 11-bit weights packed
//    as u16 pairs, and row byte offsets for the vertical taps;
//  * horizontal mix p0 * w0 + p1 * w1 = v_perm_b32 + v_dot2_u32_u16 per (row, channel);
//  * vertical mix with v_mul_u32_u24 (full rate: operands are 12 and 15 bits) and SDWA word selects for the >> 16;
//  * one frame per blockIdx.y (frame base in SGPRs, 32-bit per-lane offsets), pixel index -> (row, column) by a
//    multiply-high with a host-computed reciprocal.
// frames_to_grid: 8 window loads + ~190 full-rate VALU instructions per output pixel (16 taps x 3 channels through five
// exact fixed-point mixes); bilinear_gather: 4 loads + ~55.  Degenerate sizes (W < 3) keep the generic kernels.

// the two taps of one sample inside an 8-byte window of the source row: {window start, selector, weights, 0}
static uint4 fused_x_sample(const int4 t, int W) {
    const int lim = 3 * W - 8;
    const int o = 3 * t.x < lim ? 3 * t.x : lim;                       // window start (bytes into the row)
    return make_uint4((unsigned)o, perm_sel((unsigned)(3 * t.x - o), (unsigned)(3 * t.y - o)), (unsigned)t.z | ((unsigned)t.w << 16), 0);
}

typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
// p0 * w0 + p1 * w1 for channel c of the two taps inside the 8-byte window {hi, lo}
__device__ __forceinline__ unsigned hmix(unsigned hi, unsigned lo, unsigned sel, unsigned w) {
    const unsigned pair = __builtin_amdgcn_perm(hi, lo, sel);
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, pair), __builtin_bit_cast(u16x2_t, w), 0u, false);
}
// VResizeLinear<uchar, int, short>: (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.
// (b * (S >> 4)) >> 16 == ((b << 12) * (S & ~15)) >> 32 exactly (both factors are below 2^24), which is ONE full-rate
// v_mul_hi_u32_u24 after one AND instead of shift + multiply + shift; the tables carry the weights pre-shifted (B = b << 12).
__device__ __forceinline__ unsigned mulhi24(unsigned a, unsigned b) { unsigned d; asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ unsigned vmix(unsigned h0, unsigned h1, unsigned B0, unsigned B1) {
    return (mulhi24(B0, h0 & ~15u) + mulhi24(B1, h1 & ~15u) + 2u) >> 2;
}
__device__ __forceinline__ uint64_t load_window(const uint8_t* p) { return reinterpret_cast<const PackedU64*>(p)->v; }

// the PX pixels of a lane: one 12-byte store (store_px4, common.h) or three byte stores
__device__ __forceinline__ void store_px1(uint8_t* d, unsigned r, unsigned g, unsigned b) { d[0] = (uint8_t)r; d[1] = (uint8_t)g; d[2] = (uint8_t)b; }
template <int PX>
__device__ __forceinline__ void store_px(uint8_t* d, const unsigned (&v)[PX][3]) {
    if constexpr (PX == 4) store_px4(d, v);
    else store_px1(d, v[0][0], v[0][1], v[0][2]);
}

// PX output pixels of one row per lane (4 when the output width allows it, else 1)
template <int PX>
__global__ __launch_bounds__(256) void bilinear_gather_rgb_kernel(const uint8_t* __restrict__ video, size_t frame_bytes, const int* __restrict__ idx,
                                                                  int ow, int owq, unsigned magic_owq, int nunits, const uint4* __restrict__ fx,
                                                                  const uint4* __restrict__ fy, uint8_t* __restrict__ out) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;               // unit = PX consecutive pixels of a row
    if (u >= (unsigned)nunits) return;
    const int i = blockIdx.y;
    const uint8_t* f = video + (size_t)idx[i] * frame_bytes;          // wave-uniform
    const unsigned oy = __umulhi(u, magic_owq), ox = (u - oy * (unsigned)owq) * PX;
    const uint4 y = fy[oy];
    const unsigned b0 = y.z, b1 = y.w;
    uint4 x[PX];
    uint64_t w0[PX], w1[PX];
    if constexpr (PX == 4) {
        // fx = three arrays of ow entries (TAB_RGB_X3): one coalesced 16-byte load per field
        const unsigned* fa = reinterpret_cast<const unsigned*>(fx);
        const uint4 xo = *reinterpret_cast<const uint4*>(fa + ox), xs = *reinterpret_cast<const uint4*>(fa + ow + ox),
                    xw = *reinterpret_cast<const uint4*>(fa + 2 * ow + ox);
        x[0] = make_uint4(xo.x, xs.x, xw.x, 0); x[1 % PX] = make_uint4(xo.y, xs.y, xw.y, 0);
        x[2 % PX] = make_uint4(xo.z, xs.z, xw.z, 0); x[3 % PX] = make_uint4(xo.w, xs.w, xw.w, 0);
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) x[k] = fx[ox + k];
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) { w0[k] = load_window(f + (size_t)(y.x + x[k].x)); w1[k] = load_window(f + (size_t)(y.y + x[k].x)); }
    unsigned v[PX][3];
#pragma unroll
    for (int k = 0; k < PX; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned sel = x[k].y + 0x00010001u * c;
            v[k][c] = vmix(hmix((unsigned)(w0[k] >> 32), (unsigned)w0[k], sel, x[k].z), hmix((unsigned)(w1[k] >> 32), (unsigned)w1[k], sel, x[k].z), b0, b1);
        }
    uint8_t* d = out + (((size_t)i * (nunits / owq) + oy) * ow + ox) * 3;
    store_px<PX>(d, v);
}

// the shared tail of a grid pixel, per channel: from the horizontal mixes of the four source rows at the two sample columns
// (ha, hb) the four samples of the intermediate image (u8 round trip, interface_searcher.py:362), then the 4 : 1 step (:186)
__device__ __forceinline__ unsigned grid_finish(const unsigned (&ha)[4], const unsigned (&hb)[4], const uint4 yw, const uint4 yf, const unsigned wfx) {
    const unsigned fxa = wfx & 0xFFFFu, fxb = wfx >> 16;
    const unsigned p00 = vmix(ha[0], ha[1], yw.x, yw.y), p01 = vmix(hb[0], hb[1], yw.x, yw.y);
    const unsigned p10 = vmix(ha[2], ha[3], yw.z, yw.w), p11 = vmix(hb[2], hb[3], yw.z, yw.w);
    const unsigned h0 = __umul24(p00, fxa) + __umul24(p01, fxb), h1 = __umul24(p10, fxa) + __umul24(p11, fxb);
    return vmix(h0, h1, yf.x, yf.y);
}

// one output pixel of the grid: 8 (or, when the two intermediate rows share their middle source row, 6) window loads, the
// horizontal mixes, grid_finish
template <bool DUP>
__device__ __forceinline__ void grid_pixel(const uint8_t* f, const uint4 yr, const uint4 yw, const uint4 yf, const uint4 xa, const uint4 xb,
                                           unsigned (&v)[3]) {
    const unsigned rows[4] = {yr.x, yr.y, yr.z, yr.w};               // r0a, r0b | r1a, r1b   (DUP: r1a == r0b)
    uint64_t wa[4], wb[4];                                             // windows: four source rows x columns (A, B)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (DUP && r == 2) { wa[2] = wa[1]; wb[2] = wb[1]; continue; }
        wa[r] = load_window(f + (size_t)(rows[r] + xa.x));             // SGPR base + 32-bit lane offset
        wb[r] = load_window(f + (size_t)(rows[r] + xa.w));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned sa = xa.y + 0x00010001u * c, sb = xb.x + 0x00010001u * c;
        unsigned ha[4], hb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (DUP && r == 2) { ha[2] = ha[1]; hb[2] = hb[1]; continue; }
            ha[r] = hmix((unsigned)(wa[r] >> 32), (unsigned)wa[r], sa, xa.z);
            hb[r] = hmix((unsigned)(wb[r] >> 32), (unsigned)wb[r], sb, xb.y);
        }
        v[c] = grid_finish(ha, hb, yw, yf, xb.z);
    }
}

template <int PX>
__global__ __launch_bounds__(256) void frames_to_grid_rgb_kernel(const uint8_t* __restrict__ video, size_t frame_bytes, const int* __restrict__ idx,
                                                                 int cols, int cw, int ch, int cwq, unsigned magic_cwq, const uint4* __restrict__ fx,
                                                                 const uint4* __restrict__ fy, uint8_t* __restrict__ grid) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)(cwq * ch)) return;
    const int i = blockIdx.y;
    const uint8_t* f = video + (size_t)idx[i] * frame_bytes;          // wave-uniform
    const unsigned oy = __umulhi(u, magic_cwq), ox = (u - oy * (unsigned)cwq) * PX;
    unsigned v[PX][3];
    // A wave covers 64 consecutive pixels of a 200-wide cell row: two waves in three lie inside ONE output row.  Their row
    // table entry then comes through the scalar cache (three s_load_dwordx4 instead of three vector loads per lane), and
    // whether the two intermediate rows share their middle source row -- they do on ~95 % of the rows of a 360 -> 380 -> 95
    // resize -- is a scalar branch that drops two of the eight window loads and a quarter of the horizontal mixes.
    const unsigned oy_u = __builtin_amdgcn_readfirstlane(oy);
    if (PX == 1 && __all(oy == oy_u)) {
        const uint4* q = fy + 3 * oy_u;
        const uint4 yr = q[0], yw = q[1], yf = q[2];
        const uint4 xa = fx[2 * ox], xb = fx[2 * ox + 1];
        if (yr.y == yr.z) grid_pixel<true>(f, yr, yw, yf, xa, xb, v[0]);
        else grid_pixel<false>(f, yr, yw, yf, xa, xb, v[0]);
    } else {
        const uint4 yr = fy[3 * oy], yw = fy[3 * oy + 1], yf = fy[3 * oy + 2];
#pragma unroll
        for (int k = 0; k < PX; ++k) grid_pixel<false>(f, yr, yw, yf, fx[2 * (ox + k)], fx[2 * (ox + k) + 1], v[k]);
    }
    const int gr = i / cols, gc = i - gr * cols;
    uint8_t* d = grid + (((size_t)gr * ch + oy) * ((size_t)cols * cw) + (size_t)gc * cw + ox) * 3;
    store_px<PX>(d, v);
}

// ------------------------------------------------------------------ NV12 fast path of the grid kernel
// Same structure for NV12 frame stores (luma plane + interleaved half-resolution UV plane).  The generic kernel issues
// three byte loads per tap (48 per grid pixel); here a (source row, sample) pair is TWO 4-byte windows -- the luma bytes
// of both taps, and the one or two UV pairs they use -- and every tap is converted with the same BT.601 integer matrix
// (SrcNV12::at, bit for bit) before it is mixed: (Y, V) / (Y, U) / (U, V) pairs are dropped into 16-bit halves with
// v_perm_b32 and each channel is one v_dot2_i32_i16 with the constant folded into the accumulator:
//   R = clip((298 Y + 409 V - 56992) >> 8)    B = clip((298 Y + 516 U - 70688) >> 8)
//   G = clip((R_pre - 100 U - 617 V + 91776) >> 8)            [= 298 Y - 100 U - 208 V + 34784]
// A selector reads {chroma window, luma window} as bytes 4-7 / 0-3: selYU = perm_sel(lumaByte, 4 + uvByte).
// {luma window | chroma window << 16, selYU of the left tap, of the right tap, weights}
static uint4 fused_x_sample_nv12(const int4 t, int W) {
    const int oy = t.x < W - 4 ? t.x : W - 4;                          // 4-byte luma window holding both taps
    const int cx = t.x & ~1, oc = cx < W - 4 ? cx : W - 4;             // 4-byte chroma window holding both taps' UV pairs
    return make_uint4((unsigned)oy | ((unsigned)oc << 16), perm_sel((unsigned)(t.x - oy), 4u + (unsigned)((t.x & ~1) - oc)),
                      perm_sel((unsigned)(t.y - oy), 4u + (unsigned)((t.y & ~1) - oc)), (unsigned)t.z | ((unsigned)t.w << 16));
}

// host copy of a fused table (layouts at TabKind); W, H: the frame, src / mid / dst: the axis the table resamples
static std::vector<uint4> build_table(TabKind kind, int src, int mid, int dst, int W, int H) {
    const bool two = kind == TAB_RGB_X2 || kind == TAB_RGB_Y2 || kind == TAB_NV12_X2 || kind == TAB_NV12_Y2;
    const std::vector<int4> t1 = linear_taps(src, two ? mid : dst), t2 = two ? linear_taps(mid, dst) : std::vector<int4>();
    const unsigned pitch = 3u * W, hw = (unsigned)H * W;
    if (kind == TAB_RGB_X3) {
        const int np = (dst + 3) / 4 * 4;
        std::vector<unsigned> a(3 * (size_t)np, 0u);
        for (int d = 0; d < dst; ++d) { const uint4 e = fused_x_sample(t1[d], W); a[d] = e.x; a[np + d] = e.y; a[2 * np + d] = e.z; }
        std::vector<uint4> h(a.size() / 4);
        memcpy(h.data(), a.data(), a.size() * 4);
        return h;
    }
    auto rows = [](int4 a, int4 b, unsigned pitch, unsigned base, int sh) {
        return make_uint4(base + (unsigned)(a.x >> sh) * pitch, base + (unsigned)(a.y >> sh) * pitch, base + (unsigned)(b.x >> sh) * pitch,
                          base + (unsigned)(b.y >> sh) * pitch);
    };
    auto wts = [](int4 a, int4 b) { return make_uint4((unsigned)a.z << 12, (unsigned)a.w << 12, (unsigned)b.z << 12, (unsigned)b.w << 12); };
    const int4 none = make_int4(0, 0, 0, 0);
    std::vector<uint4> h;
    for (int d = 0; d < dst; ++d) {
        const int4 f = two ? t2[d] : none, a = two ? t1[f.x] : t1[d], b = two ? t1[f.y] : none;      // F, A, B
        const unsigned wf = (unsigned)f.z | ((unsigned)f.w << 16);
        switch (kind) {
        case TAB_RGB_X: h.push_back(fused_x_sample(a, W)); break;
        case TAB_RGB_Y: h.push_back(make_uint4((unsigned)a.x * pitch, (unsigned)a.y * pitch, (unsigned)a.z << 12, (unsigned)a.w << 12)); break;
        case TAB_RGB_X2: {
            const uint4 A = fused_x_sample(a, W), B = fused_x_sample(b, W);
            h.insert(h.end(), {make_uint4(A.x, A.y, A.z, B.x), make_uint4(B.y, B.z, wf, 0)});
        } break;
        case TAB_RGB_Y2: h.insert(h.end(), {rows(a, b, pitch, 0, 0), wts(a, b), wts(f, none)}); break;
        case TAB_NV12_X: h.push_back(fused_x_sample_nv12(a, W)); break;
        case TAB_NV12_Y:
            h.insert(h.end(), {make_uint4((unsigned)a.x * W, (unsigned)a.y * W, hw + (unsigned)(a.x >> 1) * W, hw + (unsigned)(a.y >> 1) * W), wts(a, none)});
            break;
        case TAB_NV12_X2: h.insert(h.end(), {fused_x_sample_nv12(a, W), fused_x_sample_nv12(b, W), make_uint4(wf, 0, 0, 0)}); break;
        case TAB_NV12_Y2: h.insert(h.end(), {rows(a, b, W, 0, 0), rows(a, b, W, hw, 1), wts(a, b), wts(f, none)}); break;
        default: break;
        }
    }
    return h;
}
static int get_table(TabKind kind, int src, int mid, int dst, int W, int H, const uint4** out) {
    return cached_table(TabKey{kind, src, mid, dst, W, H}, [&] { return build_table(kind, src, mid, dst, W, H); }, out);
}

struct __attribute__((packed)) PackedU32 { unsigned v; };
__device__ __forceinline__ unsigned load_window32(const uint8_t* p) { return reinterpret_cast<const PackedU32*>(p)->v; }
typedef short i16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int sdot2(unsigned pair, unsigned coef, int acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2_t, pair), __builtin_bit_cast(i16x2_t, coef), acc, false);
}
__device__ __forceinline__ unsigned clip_s8(int v) { const int t = v >> 8; return (unsigned)(t < 0 ? 0 : (t > 255 ? 255 : t)); }   // v_med3_i32
// one tap of an NV12 frame -> RGB (SrcNV12::at), from the luma / chroma windows and the tap's (Y, U) selector
__device__ __forceinline__ void nv12_tap(unsigned lu, unsigned ch, unsigned sel_yu, unsigned (&rgb)[3]) {
    const unsigned yu = __builtin_amdgcn_perm(ch, lu, sel_yu);                 // Y | U << 16
    const unsigned yv = __builtin_amdgcn_perm(ch, lu, sel_yu + 0x00010000u);   // Y | V << 16
    const unsigned uv = (yu >> 16) | (yv & 0xFFFF0000u);                        // U | V << 16
    const int rp = sdot2(yv, 298u | (409u << 16), -56992);
    const int bp = sdot2(yu, 298u | (516u << 16), -70688);
    const int gp = sdot2(uv, (unsigned)(unsigned short)(-100) | ((unsigned)(unsigned short)(-617) << 16), rp + 91776);
    rgb[0] = clip_s8(rp); rgb[1] = clip_s8(gp); rgb[2] = clip_s8(bp);
}

template <bool DUP>
__device__ __forceinline__ void grid_pixel_nv12(const uint8_t* f, const uint4 yl, const uint4 yc, const uint4 yw, const uint4 yf, const uint4 xa,
                                                const uint4 xb, const unsigned wfx, unsigned (&v)[3]) {
    const unsigned lrow[4] = {yl.x, yl.y, yl.z, yl.w}, crow[4] = {yc.x, yc.y, yc.z, yc.w};
    const unsigned oYa = xa.x & 0xFFFFu, oCa = xa.x >> 16, oYb = xb.x & 0xFFFFu, oCb = xb.x >> 16;
    const unsigned wa0 = xa.w & 0xFFFFu, wa1 = xa.w >> 16, wb0 = xb.w & 0xFFFFu, wb1 = xb.w >> 16;
    unsigned ha[3][4], hb[3][4];                                       // horizontal mixes per channel, source row (samples A, B)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (DUP && r == 2) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { ha[c][2] = ha[c][1]; hb[c][2] = hb[c][1]; }
            continue;
        }
        const unsigned la = load_window32(f + (size_t)(lrow[r] + oYa)), ca = load_window32(f + (size_t)(crow[r] + oCa));
        const unsigned lb = load_window32(f + (size_t)(lrow[r] + oYb)), cb = load_window32(f + (size_t)(crow[r] + oCb));
        unsigned pl[3], pr[3];
        nv12_tap(la, ca, xa.y, pl); nv12_tap(la, ca, xa.z, pr);
#pragma unroll
        for (int c = 0; c < 3; ++c) ha[c][r] = __umul24(pl[c], wa0) + __umul24(pr[c], wa1);
        nv12_tap(lb, cb, xb.y, pl); nv12_tap(lb, cb, xb.z, pr);
#pragma unroll
        for (int c = 0; c < 3; ++c) hb[c][r] = __umul24(pl[c], wb0) + __umul24(pr[c], wb1);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = grid_finish(ha[c], hb[c], yw, yf, wfx);
}

__global__ __launch_bounds__(256) void frames_to_grid_nv12_kernel(const uint8_t* __restrict__ video, size_t frame_bytes, const int* __restrict__ idx,
                                                                  int cols, int cw, int ch, unsigned magic_cw, const uint4* __restrict__ fx,
                                                                  const uint4* __restrict__ fy, uint8_t* __restrict__ grid) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)(cw * ch)) return;
    const int i = blockIdx.y;
    const uint8_t* f = video + (size_t)idx[i] * frame_bytes;          // wave-uniform
    const unsigned oy = __umulhi(u, magic_cw), ox = u - oy * (unsigned)cw;
    const uint4 xa = fx[3 * ox], xb = fx[3 * ox + 1], xf = fx[3 * ox + 2];
    unsigned v[3];
    const unsigned oy_u = __builtin_amdgcn_readfirstlane(oy);
    if (__all(oy == oy_u)) {                                           // the row entry through the scalar cache (see the RGB kernel)
        const uint4* q = fy + 4 * oy_u;
        const uint4 yl = q[0], yc = q[1], yw = q[2], yf = q[3];
        if (yl.y == yl.z) grid_pixel_nv12<true>(f, yl, yc, yw, yf, xa, xb, xf.x, v);
        else grid_pixel_nv12<false>(f, yl, yc, yw, yf, xa, xb, xf.x, v);
    } else {
        grid_pixel_nv12<false>(f, fy[4 * oy], fy[4 * oy + 1], fy[4 * oy + 2], fy[4 * oy + 3], xa, xb, xf.x, v);
    }
    const int gr = i / cols, gc = i - gr * cols;
    uint8_t* d = grid + (((size_t)gr * ch + oy) * ((size_t)cols * cw) + (size_t)gc * cw + ox) * 3;
    store_px1(d, v[0], v[1], v[2]);
}

// NV12 form of the resize kernel: per pixel two rows x (luma window, chroma window), four taps converted, mixed as above
template <int PX>
__global__ __launch_bounds__(256) void bilinear_gather_nv12_kernel(const uint8_t* __restrict__ video, size_t frame_bytes, const int* __restrict__ idx,
                                                                   int ow, int owq, unsigned magic_owq, int nunits, const uint4* __restrict__ fx,
                                                                   const uint4* __restrict__ fy, uint8_t* __restrict__ out) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)nunits) return;
    const int i = blockIdx.y;
    const uint8_t* f = video + (size_t)idx[i] * frame_bytes;          // wave-uniform
    const unsigned oy = __umulhi(u, magic_owq), ox = (u - oy * (unsigned)owq) * PX;
    uint4 yr, yw;
    const unsigned oy_u = __builtin_amdgcn_readfirstlane(oy);
    if (__all(oy == oy_u)) { const uint4* q = fy + 2 * oy_u; yr = q[0]; yw = q[1]; }
    else { yr = fy[2 * oy]; yw = fy[2 * oy + 1]; }
    unsigned v[PX][3];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const uint4 x = fx[ox + k];
        const unsigned oY = x.x & 0xFFFFu, oC = x.x >> 16, w0 = x.w & 0xFFFFu, w1 = x.w >> 16;
        unsigned h[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const unsigned lu = load_window32(f + (size_t)((r ? yr.y : yr.x) + oY)), cc = load_window32(f + (size_t)((r ? yr.w : yr.z) + oC));
            unsigned pl[3], pr[3];
            nv12_tap(lu, cc, x.y, pl); nv12_tap(lu, cc, x.z, pr);
#pragma unroll
            for (int c = 0; c < 3; ++c) h[r][c] = __umul24(pl[c], w0) + __umul24(pr[c], w1);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k][c] = vmix(h[0][c], h[1][c], yw.x, yw.y);
    }
    uint8_t* d = out + (((size_t)i * (nunits / owq) + oy) * ow + ox) * 3;
    store_px<PX>(d, v);
}

// Round 6: the NV12 resize with every SOURCE pixel converted once.  The kernel above converts per tap -- four BT.601 conversions (~13
// VALU each) per output pixel -- although a 360x640 -> 285x600 resize reads only 1.35 source pixels per output pixel.  Here a block
// owns an 8 x 128 tile of the output: it converts the source region the tile's taps fall in (rows ty[first].s0 .. ty[last].s1, columns
// from tx[first].s0 rounded down to a multiple of 4) to packed RGB in LDS -- 4 luma bytes + the 2 UV pairs they share per lane and
// step, one ds_write_b128 -- and then mixes 4 output pixels per lane from LDS with the same fixed-point formulas (v_perm_b32 +
// v_dot2_u32_u16 horizontally, vmix vertically): same bits, ~65 instead of ~110 VALU per output pixel.  Needs W % 4 == 0 and
// ow % 4 == 0 (the launcher falls back to the per-tap kernel otherwise); the region's size is computed on the host per
// (H, W, oh, ow) and bounds the dynamic LDS.
constexpr int NV_TR = 8, NV_TC = 128;
__global__ __launch_bounds__(256) void bilinear_gather_nv12_lds_kernel(const uint8_t* __restrict__ video, size_t frame_bytes, const int* __restrict__ idx,
                                                                       int H, int W, int ow, int oh, int tiles_x, int pitch,
                                                                       const int4* __restrict__ tx, const int4* __restrict__ ty, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned nv_region[];
    const int t = threadIdx.x;
    const int tile = blockIdx.x, tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int oy0 = tyi * NV_TR, ox0 = txi * NV_TC;
    const int oy1 = (oy0 + NV_TR < oh ? oy0 + NV_TR : oh) - 1, ox1 = (ox0 + NV_TC < ow ? ox0 + NV_TC : ow) - 1;
    const uint8_t* f = video + (size_t)idx[blockIdx.y] * frame_bytes;     // block-uniform
    const int ry0 = ty[oy0].x, ry1 = ty[oy1].y;
    const int rx0 = tx[ox0].x & ~3, rx1 = tx[ox1].y;
    const int nrows = ry1 - ry0 + 1, ncols4 = ((rx1 - rx0) >> 2) + 1;
    // ---- phase 1: source region -> packed RGB (r | g << 8 | b << 16) in LDS
    const int items = nrows * ncols4;
    const float inv = 1.0f / (float)ncols4;
    const size_t hw = (size_t)H * W;
    for (int it = t; it < items; it += 256) {
        const int r = (int)(((float)it + 0.5f) * inv);                    // it / ncols4 (exact: it < 2^13, the half keeps clear of the rounding)
        const int c4 = it - r * ncols4;
        const int sy = ry0 + r, sx = rx0 + 4 * c4;
        const unsigned lu = *reinterpret_cast<const unsigned*>(f + (size_t)sy * W + sx);
        const unsigned ch = *reinterpret_cast<const unsigned*>(f + hw + (size_t)(sy >> 1) * W + sx);
        uint4 o;
        unsigned rgb[3];
        nv12_tap(lu, ch, perm_sel(0, 4), rgb); o.x = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
        nv12_tap(lu, ch, perm_sel(1, 4), rgb); o.y = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
        nv12_tap(lu, ch, perm_sel(2, 6), rgb); o.z = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
        nv12_tap(lu, ch, perm_sel(3, 6), rgb); o.w = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
        *reinterpret_cast<uint4*>(nv_region + r * pitch + 4 * c4) = o;
    }
    __syncthreads();
    // ---- phase 2: 4 consecutive output pixels of one row per lane
    const int oy = oy0 + (t >> 5), ox = ox0 + 4 * (t & 31);
    if (oy > oy1 || ox > ox1) return;
    const int4 ye = ty[oy];
    const unsigned* row0 = nv_region + (ye.x - ry0) * pitch - rx0;
    const unsigned* row1 = nv_region + (ye.y - ry0) * pitch - rx0;
    const unsigned b0 = (unsigned)ye.z << 12, b1 = (unsigned)ye.w << 12;
    unsigned v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int4 xe = tx[ox + k];
        const unsigned w = (unsigned)xe.z | ((unsigned)xe.w << 16);
        const unsigned p00 = row0[xe.x], p01 = row0[xe.y], p10 = row1[xe.x], p11 = row1[xe.y];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned sel = perm_sel(c, 4 + c);                                              // byte c of the left tap | byte c of the right tap << 16
            v[k][c] = vmix(hmix(p01, p00, sel, w), hmix(p11, p10, sel, w), b0, b1);
        }
    }
    store_px4(out + (((size_t)blockIdx.y * oh + oy) * ow + ox) * 3, v);
}

// largest source region (rows, 4-pixel column groups) any 8 x 128 output tile of a (H, W) -> (oh, ow) resize needs
static void nv12_lds_region(int H, int W, int oh, int ow, int* max_rows, int* max_cols4) {
    int mr = 0, mc = 0;
    for (int y0 = 0; y0 < oh; y0 += NV_TR) {
        const int rows = linear_tap(H, oh, (y0 + NV_TR < oh ? y0 + NV_TR : oh) - 1).y - linear_tap(H, oh, y0).x + 1;
        if (rows > mr) mr = rows;
    }
    for (int x0 = 0; x0 < ow; x0 += NV_TC) {
        const int n = ((linear_tap(W, ow, (x0 + NV_TC < ow ? x0 + NV_TC : ow) - 1).y - (linear_tap(W, ow, x0).x & ~3)) >> 2) + 1;
        if (n > mc) mc = n;
    }
    *max_rows = mr; *max_cols4 = mc;
}

// ------------------------------------------------------------------ the launch policy
// Everything that decides which kernel form a launch gets, and its grid.  A fast form puts one frame on blockIdx.y (n <= 65535),
// addresses a frame with 32-bit lane offsets (frame bytes < 2^31) and splits the unit index with magic_of(ow / px): ow / px >= 2
// (magic_of(1) would be 2^32, which does not fit the 32-bit multiplier: the row / column split would read past the tap tables)
// and units * ow < 2^32.
IngestPlan plan_ingest(int op, bool nv12, int H, int W, int n, int ow, int oh, bool out_aligned4, bool video_aligned4,
                       const IngestOverrides& o) {
    IngestPlan p{nullptr, INGEST_GENERIC, 1, 0, 1, 0, 0};
    if (op != INGEST_RESIZE && op != INGEST_GRID) { p.error = "plan_ingest: op must be 0 (resize) or 1 (grid)"; return p; }
    if (!(n > 0 && ow > 0 && oh > 0)) { p.error = op == INGEST_GRID ? "frames_to_grid_u8: empty grid" : "bilinear_gather_u8: empty output"; return p; }
    const long long npix = (long long)ow * oh, frame_bytes = (long long)H * W * 3 / (nv12 ? 2 : 1);
    const bool fits = n <= 65535 && frame_bytes < (1ll << 31);
    const bool fast = !o.generic && fits && W >= 3 && ow >= 2 && npix < (1ll << 31) && npix * ow < (1ll << 32);
    // 4 pixels per lane need dword-aligned 12-byte stores: a row of the output must be a multiple of 4 pixels.  The grid takes one
    // pixel per lane unless asked: four measured 63 us against 52 for the 256-frame grid -- 32 window loads and five dependent
    // mix levels per lane leave too few lanes in flight; the grid's stores are 8 % of its bytes anyway.  NV12 grid: always one.
    const bool px4 = ow % 4 == 0 && ow >= 8 && out_aligned4 && (op == INGEST_RESIZE || (o.grid_px == 4 && !nv12));
    if (op == INGEST_RESIZE && nv12 && o.nv12_lds && fits && W % 4 == 0 && H % 2 == 0 && ow % 4 == 0 && ow >= 4 && out_aligned4 && video_aligned4 &&
        frame_bytes % 4 == 0) {
        int mr, mc;
        nv12_lds_region(H, W, oh, ow, &mr, &mc);
        const int pitch = mc * 4 + 4;                                     // dwords; rows stay 16-byte aligned, consecutive rows shifted by 4 banks
        const long long lds = (long long)mr * pitch * 4;
        if (lds <= 64 * 1024 && mr * mc < 8192) {                         // the kernel's it / ncols4 is exact below 2^13 items
            p.kind = INGEST_NV12_LDS; p.px = 4; p.lds_bytes = (int)lds; p.lds_pitch = pitch;
            p.grid_x = (unsigned)(((ow + NV_TC - 1) / NV_TC) * ((oh + NV_TR - 1) / NV_TR)); p.grid_y = (unsigned)n;
            return p;
        }
    }
    if (fast && (!nv12 || (W >= 4 && W <= 65535 && W % 2 == 0 && H % 2 == 0))) {      // NV12 tables pack two 16-bit column offsets
        p.kind = nv12 ? INGEST_NV12_TAP : INGEST_RGB_FAST; p.px = px4 ? 4 : 1;
        p.grid_x = (unsigned)(((long long)(ow / p.px) * oh + 255) / 256); p.grid_y = (unsigned)n;
        return p;
    }
    p.grid_x = (unsigned)(((unsigned long long)n * ow * oh + 255) / 256);
    return p;
}

// TSTAR_INGEST_GENERIC / TSTAR_NV12_LDS / TSTAR_GRID_PX (meanings at IngestOverrides), read once per process
static const IngestOverrides& ingest_overrides() {
    static const IngestOverrides o = [] {
        IngestOverrides v;
        if (const char* e = getenv("TSTAR_INGEST_GENERIC")) v.generic = atoi(e) != 0;
        if (const char* e = getenv("TSTAR_NV12_LDS")) v.nv12_lds = atoi(e) != 0;
        if (const char* e = getenv("TSTAR_GRID_PX")) v.grid_px = atoi(e);
        return v;
    }();
    return o;
}
static unsigned magic_of(int d) { return (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); }   // d >= 2 (plan_ingest)
static bool aligned4(const void* p) { return (reinterpret_cast<size_t>(p) & 3) == 0; }
// the <4> / <1> pair of a kernel template, 256 lanes per block
template <class K, class... A>
static void launch_px(int px, K k4, K k1, dim3 g, hipStream_t s, A... a) { hipLaunchKernelGGL(px == 4 ? k4 : k1, g, dim3(256), 0, s, a...); }

// HResizeLinear + VResizeLinear<uchar, int, short> of one channel in plain integers (the generic kernels' form of hmix + vmix).
// A functor over references to the taps, like the lambdas it replaces: a function taking the taps by value computes the same
// but changed the register allocation of three generic kernels.
struct CvMix {
    const int4& tx; const int4& ty;
    __device__ __forceinline__ int operator()(int p00, int p01, int p10, int p11) const {
        const int h0 = p00 * tx.z + p01 * tx.w;
        const int h1 = p10 * tx.z + p11 * tx.w;
        return (((ty.z * (h0 >> 4)) >> 16) + ((ty.w * (h1 >> 4)) >> 16) + 2) >> 2;
    }
};

// one bilinear sample (all three channels) at output taps tx, ty
template <class SRC>
__device__ __forceinline__ Rgb lin_sample(const SRC& im, const int4 tx, const int4 ty) {
    Rgb a, b, c, d;
    if (SRC::kWidePair && tx.y == tx.x + 1 && tx.x <= im.W - 3) {     // two adjacent source columns, away from the edge
        im.pair(tx.x, ty.x, a, b);
        im.pair(tx.x, ty.y, c, d);
    } else {
        a = im.at(tx.x, ty.x); b = im.at(tx.y, ty.x); c = im.at(tx.x, ty.y); d = im.at(tx.y, ty.y);
    }
    const CvMix mix{tx, ty};
    return Rgb{mix(a.r, b.r, c.r, d.r), mix(a.g, b.g, c.g, d.g), mix(a.b, b.b, c.b, d.b)};
}

template <class SRC>
__global__ __launch_bounds__(256) void bilinear_gather_kernel(const uint8_t* __restrict__ video, int H, int W,
                                                              const int* __restrict__ idx, int ow, int oh,
                                                              const int4* __restrict__ tabx, const int4* __restrict__ taby,
                                                              uint8_t* __restrict__ out, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int ox = (int)(gid % ow);
    const int oy = (int)((gid / ow) % oh);
    const int i = (int)(gid / ((size_t)ow * oh));
    SRC im{video + (size_t)idx[i] * SRC::frame_bytes(H, W), W, H};
    const Rgb v = lin_sample(im, tabx[ox], taby[oy]);
    store_px1(out + gid * 3, v.r, v.g, v.b);
}

int bilinear_gather_u8(const uint8_t* video, int H, int W, const int* d_idx, int n, int ow, int oh, uint8_t* out,
                       int nv12, hipStream_t s) {
    const IngestPlan p = plan_ingest(INGEST_RESIZE, nv12 != 0, H, W, n, ow, oh, aligned4(out), aligned4(video), ingest_overrides());
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    const dim3 g(p.grid_x, p.grid_y);
    const size_t frame_bytes = nv12 ? (size_t)H * W * 3 / 2 : (size_t)H * W * 3;
    const int owq = ow / p.px, nunits = owq * oh;
    const int4 *tx, *ty;
    const uint4 *fx, *fy;
    int rc;
    switch (p.kind) {
    case INGEST_RGB_FAST:
        if ((rc = get_table(p.px == 4 ? TAB_RGB_X3 : TAB_RGB_X, W, 0, ow, W, H, &fx)) || (rc = get_table(TAB_RGB_Y, H, 0, oh, W, H, &fy))) return rc;
        launch_px(p.px, bilinear_gather_rgb_kernel<4>, bilinear_gather_rgb_kernel<1>, g, s, video, frame_bytes, d_idx, ow, owq, magic_of(owq), nunits, fx, fy, out);
        break;
    case INGEST_NV12_TAP:
        if ((rc = get_table(TAB_NV12_X, W, 0, ow, W, H, &fx)) || (rc = get_table(TAB_NV12_Y, H, 0, oh, W, H, &fy))) return rc;
        launch_px(p.px, bilinear_gather_nv12_kernel<4>, bilinear_gather_nv12_kernel<1>, g, s, video, frame_bytes, d_idx, ow, owq, magic_of(owq), nunits, fx, fy, out);
        break;
    case INGEST_NV12_LDS:
        if ((rc = get_lintab(W, ow, &tx)) || (rc = get_lintab(H, oh, &ty))) return rc;
        hipLaunchKernelGGL(bilinear_gather_nv12_lds_kernel, g, dim3(256), (size_t)p.lds_bytes, s, video, frame_bytes, d_idx, H, W, ow, oh,
                           (ow + NV_TC - 1) / NV_TC, p.lds_pitch, tx, ty, out);
        break;
    case INGEST_GENERIC: {
        if ((rc = get_lintab(W, ow, &tx)) || (rc = get_lintab(H, oh, &ty))) return rc;
        const size_t total = (size_t)n * ow * oh;
        if (nv12) hipLaunchKernelGGL(bilinear_gather_kernel<SrcNV12>, g, dim3(256), 0, s, video, H, W, d_idx, ow, oh, tx, ty, out, total);
        else hipLaunchKernelGGL(bilinear_gather_kernel<SrcRGB>, g, dim3(256), 0, s, video, H, W, d_idx, ow, oh, tx, ty, out, total);
    } break;
    }
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

// frame -> (4cw x 4ch) -> (cw x ch), both bilinear with a u8 round trip in between
// (interface_searcher.py:362 then :186), written straight into its grid cell.
template <class SRC>
__global__ __launch_bounds__(256) void frames_to_grid_kernel(const uint8_t* __restrict__ video, int H, int W,
                                                             const int* __restrict__ idx, int cols, int cw, int ch,
                                                             const int4* __restrict__ t1x, const int4* __restrict__ t1y,
                                                             const int4* __restrict__ t2x, const int4* __restrict__ t2y,
                                                             uint8_t* __restrict__ grid, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int ox = (int)(gid % cw);
    const int oy = (int)((gid / cw) % ch);
    const int i = (int)(gid / ((size_t)cw * ch));
    SRC im{video + (size_t)idx[i] * SRC::frame_bytes(H, W), W, H};
    const int4 ax = t2x[ox], ay = t2y[oy];          // taps into the intermediate image
    const int4 x0 = t1x[ax.x], x1 = t1x[ax.y], y0 = t1y[ay.x], y1 = t1y[ay.y];
    const int gr = i / cols, gc = i % cols;
    uint8_t* d = grid + (((size_t)gr * ch + oy) * ((size_t)cols * cw) + (size_t)gc * cw + ox) * 3;
    const Rgb p00 = lin_sample(im, x0, y0), p01 = lin_sample(im, x1, y0);
    const Rgb p10 = lin_sample(im, x0, y1), p11 = lin_sample(im, x1, y1);
    const CvMix mix{ax, ay};
    store_px1(d, mix(p00.r, p01.r, p10.r, p11.r), mix(p00.g, p01.g, p10.g, p11.g), mix(p00.b, p01.b, p10.b, p11.b));
}

int frames_to_grid_u8(const uint8_t* video, int H, int W, const int* d_idx, int rows, int cols, int cw, int ch,
                      uint8_t* grid, int nv12, hipStream_t s) {
    TSTAR_REQUIRE(rows > 0 && cols > 0 && cw > 0 && ch > 0, "frames_to_grid_u8: empty grid");
    const IngestPlan p = plan_ingest(INGEST_GRID, nv12 != 0, H, W, rows * cols, cw, ch, aligned4(grid), aligned4(video), ingest_overrides());
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    const dim3 g(p.grid_x, p.grid_y);
    const size_t frame_bytes = nv12 ? (size_t)H * W * 3 / 2 : (size_t)H * W * 3;
    const int cwq = cw / p.px;
    const uint4 *fx, *fy;
    int rc;
    switch (p.kind) {
    case INGEST_RGB_FAST:
        if ((rc = get_table(TAB_RGB_X2, W, 4 * cw, cw, W, H, &fx)) || (rc = get_table(TAB_RGB_Y2, H, 4 * ch, ch, W, H, &fy))) return rc;
        launch_px(p.px, frames_to_grid_rgb_kernel<4>, frames_to_grid_rgb_kernel<1>, g, s, video, frame_bytes, d_idx, cols, cw, ch, cwq, magic_of(cwq), fx, fy, grid);
        break;
    case INGEST_NV12_TAP:
        if ((rc = get_table(TAB_NV12_X2, W, 4 * cw, cw, W, H, &fx)) || (rc = get_table(TAB_NV12_Y2, H, 4 * ch, ch, W, H, &fy))) return rc;
        hipLaunchKernelGGL(frames_to_grid_nv12_kernel, g, dim3(256), 0, s, video, frame_bytes, d_idx, cols, cw, ch, magic_of(cw), fx, fy, grid);
        break;
    default: {                                                            // INGEST_GENERIC (plan_ingest has no LDS form for the grid)
        const int4 *t1x, *t1y, *t2x, *t2y;
        if ((rc = get_lintab(W, 4 * cw, &t1x)) || (rc = get_lintab(H, 4 * ch, &t1y)) || (rc = get_lintab(4 * cw, cw, &t2x)) || (rc = get_lintab(4 * ch, ch, &t2y))) return rc;
        const size_t total = (size_t)rows * cols * cw * ch;
        if (nv12) hipLaunchKernelGGL(frames_to_grid_kernel<SrcNV12>, g, dim3(256), 0, s, video, H, W, d_idx, cols, cw, ch, t1x, t1y, t2x, t2y, grid, total);
        else hipLaunchKernelGGL(frames_to_grid_kernel<SrcRGB>, g, dim3(256), 0, s, video, H, W, d_idx, cols, cw, ch, t1x, t1y, t2x, t2y, grid, total);
    } break;
    }
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

// native-resolution NV12 -> RGB for the frames handed back to the caller (pop_frames)
__global__ __launch_bounds__(256) void nv12_to_rgb_kernel(const uint8_t* __restrict__ video, int H, int W,
                                                          const int* __restrict__ idx, uint8_t* __restrict__ out, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int x = (int)(gid % W), y = (int)((gid / W) % H), i = (int)(gid / ((size_t)W * H));
    SrcNV12 im{video + (size_t)idx[i] * SrcNV12::frame_bytes(H, W), W, H};
    const Rgb v = im.at(x, y);
    store_px1(out + gid * 3, v.r, v.g, v.b);
}

// planar I420 (Y plane, U plane, V plane: what raw 4:2:0 containers such as YUV4MPEG2 carry) -> NV12 (Y plane + interleaved
// UV plane) for n frames; 16 bytes of luma / 8 chroma pairs per lane.  Pure byte movement, HBM-bound.
__global__ __launch_bounds__(256) void i420_to_nv12_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, size_t total16) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total16) return;
    const size_t fb = (size_t)H * W * 3 / 2, per = fb / 16;            // 16-byte units per frame
    const size_t f = gid / per, u = gid % per;
    const uint8_t* src = in + f * fb;
    uint8_t* dst = out + f * fb;
    const size_t ybytes = (size_t)H * W;
    if (u * 16 < ybytes) {
        *reinterpret_cast<uint4*>(dst + u * 16) = *reinterpret_cast<const uint4*>(src + u * 16);
    } else {
        const size_t c0 = (u * 16 - ybytes) / 2;                        // first chroma sample of this unit
        const uint8_t* pu = src + ybytes + c0;
        const uint8_t* pv = src + ybytes + ybytes / 4 + c0;
        const uint2 uu = *reinterpret_cast<const uint2*>(pu), vv = *reinterpret_cast<const uint2*>(pv);
        const uint8_t* ub = reinterpret_cast<const uint8_t*>(&uu);
        const uint8_t* vb = reinterpret_cast<const uint8_t*>(&vv);
        uint8_t o[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) { o[2 * i] = ub[i]; o[2 * i + 1] = vb[i]; }
        *reinterpret_cast<uint4*>(dst + u * 16) = *reinterpret_cast<const uint4*>(o);
    }
}

int i420_to_nv12_u8(const uint8_t* in, int n, int H, int W, uint8_t* out, hipStream_t s) {
    TSTAR_REQUIRE(n > 0 && H % 2 == 0 && W % 2 == 0 && ((size_t)H * W) % 64 == 0, "i420_to_nv12_u8: needs even dimensions with H * W a multiple of 64");
    const size_t total16 = (size_t)n * H * W * 3 / 2 / 16;
    hipLaunchKernelGGL(i420_to_nv12_kernel, dim3((unsigned)((total16 + 255) / 256)), dim3(256), 0, s, in, out, H, W, total16);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

int nv12_to_rgb_u8(const uint8_t* video, int H, int W, const int* d_idx, int n, uint8_t* out, hipStream_t s) {
    TSTAR_REQUIRE(n > 0 && H % 2 == 0 && W % 2 == 0, "nv12_to_rgb_u8: NV12 needs even dimensions");
    const size_t total = (size_t)n * H * W;
    hipLaunchKernelGGL(nv12_to_rgb_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, video, H, W, d_idx, out, total);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

}  // namespace tstar
