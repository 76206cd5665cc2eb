// Baseline JPEG decode front end, device half: the coefficient blocks the host entropy stage (jpeg_host.cpp) produced
// -> RGB u8 frames in the resident store.  Two kernels per chunk of frames of one geometry:
//   jpeg_idct_kernel   dequantise + libjpeg's accurate integer IDCT + range limit -> u8 component planes (whole blocks)
//   jpeg_color_kernel  "fancy" chroma upsampling + YCbCr -> RGB, written straight into store[s0 : s0 + n]
// The integers are those of jpeg_math.h (shared with the host reference), so the result is byte-equal to libjpeg-turbo.
// Traffic per picture sample: 2 B of coefficients in, 1 B of plane out and in again, 1 B of RGB out.
#include "common.h"
#include "heads.h"
#include "jpeg_host.h"
#include "jpeg_math.h"

namespace tstar {

namespace {

constexpr int kBlocksPerWg = 32;       // 256 threads: 8 lanes per 8x8 block, 8 blocks per wave
constexpr int kRowPitch = 9;           // LDS dwords per block row: with 72 per block, every access below is bank-conflict-free
constexpr int kBlockPitch = 72;

// One workgroup = 32 consecutive blocks of one component (block-raster order, frame after frame).
//   load   lane (block, r) reads coefficient row r as one 16-byte vector -- a wave reads 1 KiB contiguous -- and the matching
//          quantiser row, multiplies, and parks the products in LDS;
//   pass 1 lane (block, c) transforms column c in registers and writes it back in place;
//   pass 2 lane (r, block) transforms row r, limits the range and stores 8 pixels as one 8-byte vector; the 8 lanes of a
//          row r cover 64 contiguous bytes of the plane when the blocks are neighbours.
// LDS word of element (row k, col c) of block b: b * 72 + k * 9 + c.  Bank = that mod 64: for a fixed k (pass 1: lanes
// (b, c)) 8b + c + 9k is distinct over the 64 lanes of a wave; for a fixed c (load / pass 2: lanes (b, r)) 8(b + r) + r + c
// is distinct too.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, size_t coef_frame_stride,
                                                        const uint16_t* __restrict__ quant, uint8_t* __restrict__ planes,
                                                        size_t plane_frame_stride, int nblk, int bw, size_t total_blocks) {
    __shared__ uint32_t ws[kBlocksPerWg * kBlockPitch];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kBlocksPerWg;
    {
        const int bl = t >> 3, r = t & 7;
        const size_t gb = base + bl;
        if (gb < total_blocks) {
            const size_t f = gb / nblk, g = gb % nblk;
            const uint4 cv = *reinterpret_cast<const uint4*>(coef + f * coef_frame_stride + g * 64 + r * 8);
            const uint4 qv = *reinterpret_cast<const uint4*>(quant + f * 192 + r * 8);
            const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
            uint32_t* dst = ws + bl * kBlockPitch + r * kRowPitch;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c0 = (int16_t)(cw[k] & 0xffff), c1 = (int16_t)(cw[k] >> 16);
                dst[2 * k] = (uint32_t)(c0 * (int)(qw[k] & 0xffff));
                dst[2 * k + 1] = (uint32_t)(c1 * (int)(qw[k] >> 16));
            }
        }
    }
    __syncthreads();
    {
        const int bl = t >> 3, c = t & 7;
        uint32_t* col = ws + bl * kBlockPitch + c;
        uint32_t x[8];
        int32_t o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = col[k * kRowPitch];
        jpegmath::idct8(x, o, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) col[k * kRowPitch] = (uint32_t)o[k];
    }
    __syncthreads();
    {
        const int lane = t & 63, bl = (t >> 6) * 8 + (lane & 7), r = lane >> 3;
        const size_t gb = base + bl;
        if (gb < total_blocks) {
            const uint32_t* row = ws + bl * kBlockPitch + r * kRowPitch;
            uint32_t x[8];
            int32_t o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = row[k];
            jpegmath::idct8(x, o, 18);
            uint2 px;
            px.x = (uint32_t)jpegmath::range_limit(o[0]) | ((uint32_t)jpegmath::range_limit(o[1]) << 8) |
                   ((uint32_t)jpegmath::range_limit(o[2]) << 16) | ((uint32_t)jpegmath::range_limit(o[3]) << 24);
            px.y = (uint32_t)jpegmath::range_limit(o[4]) | ((uint32_t)jpegmath::range_limit(o[5]) << 8) |
                   ((uint32_t)jpegmath::range_limit(o[6]) << 16) | ((uint32_t)jpegmath::range_limit(o[7]) << 24);
            const size_t f = gb / nblk, g = gb % nblk;
            const size_t by = g / bw, bx = g % bw;
            *reinterpret_cast<uint2*>(planes + f * plane_frame_stride + (by * 8 + r) * ((size_t)bw * 8) + bx * 8) = px;
        }
    }
}

// The reduced forms for a decode at 1/2, 1/4, 1/8 size (jpeg_host.h JpegScaledGeom): K x K pixels per block from its low-frequency
// corner, K = 4 or 2 (jpeg_math.h idct4 / idct2).  The same workgroup, loads and LDS layout as above.  The blocks are counted over
// rows padded to bwp = bw rounded up to a multiple of 4 / K blocks (the lanes of the padding idle), so that the row pieces of 4 / K
// neighbouring lanes always start a dword of the plane (rows of `pitch` bytes, a multiple of 4).
//   load   as above, every row (a block is one 128-byte line whichever rows are read);
//   pass 1 lane (block, c) transforms column c, for the columns the row pass reads, and writes K values back;
//   pass 2 lane (block, r), r < K, transforms row r.  K = 4: the four pixels are one dword store.  K = 2: the lane of the even block
//          takes the odd neighbour's two pixels from lane + 8 and stores the dword; a last block without a neighbour stores 2 bytes.
// LDS accesses are dwords: banks are words mod 32 within each half of a wave.  A half is lanes (b, i) of 4 consecutive blocks,
// i = 0 .. 7: for a fixed k (pass 1) 8b + i + 9k, for a fixed c (load / pass 2) 8b + 9i + c are distinct mod 32 over them.
template <int K>
__global__ __launch_bounds__(256) void jpeg_idct_reduced_kernel(const int16_t* __restrict__ coef, size_t coef_frame_stride,
                                                                const uint16_t* __restrict__ quant, uint8_t* __restrict__ planes,
                                                                size_t plane_frame_stride, int bw, int bh, int pitch, size_t total_blocks) {
    static_assert(K == 4 || K == 2, "block sizes 8 and 1 have kernels of their own");
    __shared__ uint32_t ws[kBlocksPerWg * kBlockPitch];
    const int t = threadIdx.x, bl = t >> 3, i = t & 7;
    const int bwp = (bw + 4 / K - 1) & ~(4 / K - 1);
    const size_t vb = (size_t)blockIdx.x * kBlocksPerWg + bl, per = (size_t)bh * bwp;
    const size_t f = vb / per;
    const int by = (int)(vb % per / bwp), bx = (int)(vb % per % bwp);
    const bool live = vb < total_blocks && bx < bw;
    uint32_t* blk = ws + bl * kBlockPitch;
    if (live) {
        const uint4 cv = *reinterpret_cast<const uint4*>(coef + f * coef_frame_stride + ((size_t)by * bw + bx) * 64 + i * 8);
        const uint4 qv = *reinterpret_cast<const uint4*>(quant + f * 192 + i * 8);
        const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
        uint32_t* dst = blk + i * kRowPitch;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c0 = (int16_t)(cw[k] & 0xffff), c1 = (int16_t)(cw[k] >> 16);
            dst[2 * k] = (uint32_t)(c0 * (int)(qw[k] & 0xffff));
            dst[2 * k + 1] = (uint32_t)(c1 * (int)(qw[k] >> 16));
        }
    }
    __syncthreads();
    if (live && jpegmath::idct_reads(K, i)) {
        uint32_t* col = blk + i;
        uint32_t x[8];
        int32_t o[K];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = col[k * kRowPitch];
        if (K == 4) jpegmath::idct4(x, o, 12);
        else jpegmath::idct2(x, o, 13);
#pragma unroll
        for (int k = 0; k < K; ++k) col[k * kRowPitch] = (uint32_t)o[k];
    }
    __syncthreads();
    uint32_t px = 0;
    const bool row = live && i < K;
    if (row) {
        const uint32_t* src = blk + i * kRowPitch;
        uint32_t x[8];
        int32_t o[K];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = src[k];
        if (K == 4) jpegmath::idct4(x, o, 19);
        else jpegmath::idct2(x, o, 20);
#pragma unroll
        for (int k = 0; k < K; ++k) px |= (uint32_t)jpegmath::range_limit(o[k]) << (8 * k);
    }
    uint8_t* dst = planes + f * plane_frame_stride + ((size_t)by * K + i) * pitch + (size_t)bx * K;
    if (K == 4) {
        if (row) *reinterpret_cast<uint32_t*>(dst) = px;
    } else {
        const uint32_t right = (uint32_t)__shfl_xor((int)px, 8);       // block bl ^ 1, the same row: every lane of the wave takes part
        if (row && !(bx & 1)) {
            if (bx + 1 < bw) *reinterpret_cast<uint32_t*>(dst) = px | (right << 16);
            else *reinterpret_cast<uint16_t*>(dst) = (uint16_t)px;
        }
    }
}

// K = 1: the dequantised DC term alone, no LDS.  One lane per four neighbouring blocks of a plane row (rows of `pitch` bytes, a
// multiple of 4) -> one dword store; the last lane of a row stores the 1 .. 3 bytes that are left.  The four 2-byte loads sit 128
// bytes apart: a block costs the memory system its line whatever is read of it.
__global__ __launch_bounds__(256) void jpeg_idct_dc_kernel(const int16_t* __restrict__ coef, size_t coef_frame_stride,
                                                           const uint16_t* __restrict__ quant, uint8_t* __restrict__ planes,
                                                           size_t plane_frame_stride, int bw, int bh, int pitch, size_t total_quads) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total_quads) return;
    const int bwq = (bw + 3) >> 2;
    const size_t per = (size_t)bh * bwq, f = q / per;
    const int by = (int)(q % per / bwq), bx = (int)(q % per % bwq) * 4;
    const int nb = bw - bx < 4 ? bw - bx : 4;
    const int16_t* src = coef + f * coef_frame_stride + ((size_t)by * bw + bx) * 64;
    const int q0 = quant[f * 192];
    uint32_t px = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < nb) px |= (uint32_t)jpegmath::range_limit(jpegmath::idct1((uint32_t)(src[j * 64] * q0))) << (8 * j);
    uint8_t* dst = planes + f * plane_frame_stride + (size_t)by * pitch + bx;
    if (nb == 4) *reinterpret_cast<uint32_t*>(dst) = px;
    else
        for (int j = 0; j < nb; ++j) dst[j] = (uint8_t)(px >> (8 * j));
}

// W, H: the size of the picture the stage writes; cw, ch: the true size of a chroma plane.  replicate: chroma of half width is read
// as p[x >> 1] (the scaled decode's 4:2:2 at block size 1) instead of through the triangle filter.
struct ColorArgs {
    size_t plane_frame_stride, off1, off2;       // byte offsets of the Cb / Cr planes inside a frame's planes
    int pitch0, pitch1, W, H, ncomp, hs, vs, cw, ch, replicate;
};

// R | G << 8 | B << 16 of pixel (x, y) of the frame whose planes start at fp.
__device__ inline uint32_t color_pixel(const uint8_t* __restrict__ fp, const ColorArgs& a, int x, int y) {
    const int yy = fp[(size_t)y * a.pitch0 + x];
    uint8_t t[3] = {(uint8_t)yy, (uint8_t)yy, (uint8_t)yy};
    if (a.ncomp == 3) {
        const int hs = a.replicate ? 1 : a.hs, cx = a.replicate ? x >> 1 : x;
        const int cb = jpegmath::upsample_at(fp + a.off1, a.pitch1, a.cw, a.ch, hs, a.vs, cx, y);
        const int cr = jpegmath::upsample_at(fp + a.off2, a.pitch1, a.cw, a.ch, hs, a.vs, cx, y);
        jpegmath::ycc_to_rgb(yy, cb, cr, t);
    }
    return (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16);
}

// npx <= 4 pixels -> 3 * npx bytes at dst: three dword stores for a full, 4-byte-aligned quad, else bytes.
template <bool DWORDS>
__device__ inline void store_pixels(uint8_t* __restrict__ dst, const uint32_t (&px)[4], int npx) {
    if (DWORDS && npx == 4) {
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
        d4[0] = px[0] | (px[1] << 24);
        d4[1] = (px[1] >> 8) | (px[2] << 16);
        d4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < npx) {
                dst[3 * j] = (uint8_t)px[j];
                dst[3 * j + 1] = (uint8_t)(px[j] >> 8);
                dst[3 * j + 2] = (uint8_t)(px[j] >> 16);
            }
    }
}

// Four consecutive pixels of the chunk (flat index over [n, H, W]) per lane -> 12 bytes = three dword stores.  A chroma
// sample is read by the (up to four) pixels it feeds from L1 / L2; HBM sees every plane byte once.
// DWORDS = false: the byte-store form for a destination that is not 4-byte aligned (odd W * H * s0).
template <bool DWORDS>
__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ planes, ColorArgs a, uint8_t* __restrict__ rgb,
                                                         size_t total_px) {
    const size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (q >= total_px) return;
    const size_t per = (size_t)a.W * a.H;
    size_t f = q / per;
    const size_t rem = q % per;
    int y = (int)(rem / a.W), x = (int)(rem % a.W);
    const int npx = total_px - q < 4 ? (int)(total_px - q) : 4;
    uint32_t px[4] = {0, 0, 0, 0};                                 // kept in registers
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < npx) {
            px[j] = color_pixel(planes + f * a.plane_frame_stride, a, x, y);
            if (++x == a.W) {
                x = 0;
                if (++y == a.H) { y = 0; ++f; }
            }
        }
    }
    store_pixels<DWORDS>(rgb + q * 3, px, npx);
}

// The same pixels for frames that go to NAMED slots of a pool: frame blockIdx.y -> pool[slots[blockIdx.y]], four consecutive
// pixels of the frame per lane (a quad never crosses into another frame: slots need not be neighbours).  A slot outside
// 0 .. pool_frames - 1 is skipped.  DWORDS: the pool and a frame's bytes are multiples of 4.
template <bool DWORDS>
__global__ __launch_bounds__(256) void jpeg_color_slots_kernel(const uint8_t* __restrict__ planes, ColorArgs a, uint8_t* __restrict__ pool,
                                                               int pool_frames, const int32_t* __restrict__ slots) {
    const int f = blockIdx.y, slot = slots[f];
    if (slot < 0 || slot >= pool_frames) return;
    const size_t per = (size_t)a.W * a.H;
    const size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (q >= per) return;
    int y = (int)(q / a.W), x = (int)(q % a.W);
    const int npx = per - q < 4 ? (int)(per - q) : 4;
    uint32_t px[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < npx) {
            px[j] = color_pixel(planes + (size_t)f * a.plane_frame_stride, a, x, y);
            if (++x == a.W) { x = 0; ++y; }
        }
    }
    store_pixels<DWORDS>(pool + ((size_t)slot * per + q) * 3, px, npx);
}

}  // namespace

// dequantise + IDCT of n frames into their planes, and the colour stage's arguments
static int jpeg_idct_planes(const int16_t* coef, const uint16_t* quant, int n, const JpegGeom& g, uint8_t* planes, ColorArgs* a,
                            hipStream_t s, const char* fn) {
    TSTAR_REQUIRE(n > 0 && g.valid(), std::string(fn) + ": n <= 0 or unsupported geometry");
    TSTAR_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)quant % 16 == 0 && (uintptr_t)planes % 8 == 0,
                  std::string(fn) + ": coefficient / table buffers need 16-byte, the plane workspace 8-byte alignment");
    const size_t blocks = g.blocks();
    TSTAR_REQUIRE(blocks * (size_t)n / kBlocksPerWg + 1 < 0x7fffffffull && (size_t)n * g.W * g.H / 1024 + 1 < 0x7fffffffull,
                  std::string(fn) + ": chunk too large for one launch");
    for (int c = 0; c < g.ncomp; ++c) {
        const int nblk = g.bw(c) * g.bh(c);
        const size_t total = (size_t)nblk * n;
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((total + kBlocksPerWg - 1) / kBlocksPerWg)), dim3(256), 0, s,
                           coef + g.block_offset(c) * 64, blocks * 64, quant + 64 * c, planes + g.block_offset(c) * 64,
                           g.plane_bytes(), nblk, g.bw(c), total);
        TSTAR_HIP_CHECK(hipGetLastError());
    }
    a->plane_frame_stride = g.plane_bytes();
    a->off1 = g.ncomp == 3 ? g.block_offset(1) * 64 : 0;
    a->off2 = g.ncomp == 3 ? g.block_offset(2) * 64 : 0;
    a->pitch0 = g.bw(0) * 8;
    a->pitch1 = g.ncomp == 3 ? g.bw(1) * 8 : 0;
    a->W = g.W; a->H = g.H; a->ncomp = g.ncomp; a->hs = g.hs; a->vs = g.vs;
    a->cw = g.cw(1); a->ch = g.ch(1);
    a->replicate = 0;
    return TSTAR_OK;
}

// the same at 1 / sg.scale size: every component through the kernel of its block size
static int jpeg_idct_scaled_planes(const int16_t* coef, const uint16_t* quant, int n, const JpegScaledGeom& sg, uint8_t* planes, ColorArgs* a,
                                   hipStream_t s, const char* fn) {
    const JpegGeom& g = sg.g;
    TSTAR_REQUIRE(n > 0 && sg.scale > 1 && sg.covered(),
                  std::string(fn) + ": n <= 0, a scale other than 2, 4, 8 or a geometry that is not covered at this scale");
    TSTAR_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)quant % 16 == 0 && (uintptr_t)planes % 8 == 0,
                  std::string(fn) + ": coefficient / table buffers need 16-byte, the plane workspace 8-byte alignment");
    const size_t blocks = g.blocks(), stride = sg.plane_bytes();
    TSTAR_REQUIRE((blocks + 3 * (size_t)g.bh(0)) * (size_t)n / kBlocksPerWg + 1 < 0x7fffffffull &&
                      (size_t)n * sg.ow() * sg.oh() / 1024 + 1 < 0x7fffffffull,
                  std::string(fn) + ": chunk too large for one launch");
    for (int c = 0; c < g.ncomp; ++c) {
        const int bw = g.bw(c), bh = g.bh(c), kc = sg.kc(c), pitch = sg.pitch(c);
        const int16_t* cc = coef + g.block_offset(c) * 64;
        const uint16_t* qc = quant + 64 * c;
        uint8_t* pc = planes + sg.plane_offset(c);
        if (kc == 8) {                                   // 4:2:0 chroma at scale 2: the full transform (pitch = bw * 8)
            const size_t total = (size_t)bw * bh * n;
            hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((total + kBlocksPerWg - 1) / kBlocksPerWg)), dim3(256), 0, s, cc,
                               blocks * 64, qc, pc, stride, bw * bh, bw, total);
        } else if (kc == 1) {
            const size_t total = (size_t)((bw + 3) / 4) * bh * n;
            hipLaunchKernelGGL(jpeg_idct_dc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cc, blocks * 64, qc, pc, stride,
                               bw, bh, pitch, total);
        } else {
            const size_t total = (size_t)(kc == 4 ? bw : (bw + 1) & ~1) * bh * n;
            const dim3 grid((unsigned)((total + kBlocksPerWg - 1) / kBlocksPerWg));
            if (kc == 4)
                hipLaunchKernelGGL(jpeg_idct_reduced_kernel<4>, grid, dim3(256), 0, s, cc, blocks * 64, qc, pc, stride, bw, bh, pitch, total);
            else
                hipLaunchKernelGGL(jpeg_idct_reduced_kernel<2>, grid, dim3(256), 0, s, cc, blocks * 64, qc, pc, stride, bw, bh, pitch, total);
        }
        TSTAR_HIP_CHECK(hipGetLastError());
    }
    const int mode = sg.chroma_mode();
    a->plane_frame_stride = stride;
    a->off1 = g.ncomp == 3 ? sg.plane_offset(1) : 0;
    a->off2 = g.ncomp == 3 ? sg.plane_offset(2) : 0;
    a->pitch0 = sg.pitch(0);
    a->pitch1 = g.ncomp == 3 ? sg.pitch(1) : 0;
    a->W = sg.ow(); a->H = sg.oh(); a->ncomp = g.ncomp;
    a->hs = mode == JPEG_CHROMA_FULL ? 1 : 2; a->vs = 1;
    a->cw = sg.cw(1); a->ch = sg.ch(1);
    a->replicate = mode == JPEG_CHROMA_REPLICATE_H2V1;
    return TSTAR_OK;
}

// the colour stage over n consecutive frames / over m frames into named slots of a pool
static int jpeg_color_frames(const uint8_t* planes, const ColorArgs& a, int n, uint8_t* rgb, hipStream_t s) {
    const size_t total_px = (size_t)n * a.W * a.H;
    const dim3 grid((unsigned)((total_px + 1023) / 1024));
    if ((uintptr_t)rgb % 4 == 0) hipLaunchKernelGGL(jpeg_color_kernel<true>, grid, dim3(256), 0, s, planes, a, rgb, total_px);
    else hipLaunchKernelGGL(jpeg_color_kernel<false>, grid, dim3(256), 0, s, planes, a, rgb, total_px);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

static int jpeg_color_slots(const uint8_t* planes, const ColorArgs& a, int m, uint8_t* pool, int pool_frames, const int32_t* slots,
                            hipStream_t s) {
    const size_t per = (size_t)a.W * a.H;
    const dim3 grid((unsigned)((per + 1023) / 1024), (unsigned)m);
    if ((uintptr_t)pool % 4 == 0 && per * 3 % 4 == 0)
        hipLaunchKernelGGL(jpeg_color_slots_kernel<true>, grid, dim3(256), 0, s, planes, a, pool, pool_frames, slots);
    else hipLaunchKernelGGL(jpeg_color_slots_kernel<false>, grid, dim3(256), 0, s, planes, a, pool, pool_frames, slots);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

int jpeg_reconstruct_u8(const int16_t* coef, const uint16_t* quant, int n, const JpegGeom& g, uint8_t* planes, uint8_t* rgb,
                        hipStream_t s) {
    ColorArgs a;
    if (const int rc = jpeg_idct_planes(coef, quant, n, g, planes, &a, s, "jpeg_reconstruct_u8")) return rc;
    return jpeg_color_frames(planes, a, n, rgb, s);
}

int jpeg_reconstruct_scaled_u8(const int16_t* coef, const uint16_t* quant, int n, const JpegScaledGeom& sg, uint8_t* planes, uint8_t* rgb,
                               hipStream_t s) {
    ColorArgs a;
    if (const int rc = jpeg_idct_scaled_planes(coef, quant, n, sg, planes, &a, s, "jpeg_reconstruct_scaled_u8")) return rc;
    return jpeg_color_frames(planes, a, n, rgb, s);
}

int jpeg_reconstruct_slots_u8(const int16_t* coef, const uint16_t* quant, int m, const JpegGeom& g, uint8_t* planes, uint8_t* pool,
                              int pool_frames, const int32_t* slots, hipStream_t s) {
    TSTAR_REQUIRE(pool_frames > 0 && m <= 65535, "jpeg_reconstruct_slots_u8: pool_frames <= 0 or more than 65535 frames");
    TSTAR_REQUIRE((uintptr_t)slots % 4 == 0, "jpeg_reconstruct_slots_u8: misaligned slot list");
    ColorArgs a;
    if (const int rc = jpeg_idct_planes(coef, quant, m, g, planes, &a, s, "jpeg_reconstruct_slots_u8")) return rc;
    return jpeg_color_slots(planes, a, m, pool, pool_frames, slots, s);
}

int jpeg_reconstruct_slots_scaled_u8(const int16_t* coef, const uint16_t* quant, int m, const JpegScaledGeom& sg, uint8_t* planes,
                                     uint8_t* pool, int pool_frames, const int32_t* slots, hipStream_t s) {
    TSTAR_REQUIRE(pool_frames > 0 && m <= 65535, "jpeg_reconstruct_slots_scaled_u8: pool_frames <= 0 or more than 65535 frames");
    TSTAR_REQUIRE((uintptr_t)slots % 4 == 0, "jpeg_reconstruct_slots_scaled_u8: misaligned slot list");
    ColorArgs a;
    if (const int rc = jpeg_idct_scaled_planes(coef, quant, m, sg, planes, &a, s, "jpeg_reconstruct_slots_scaled_u8")) return rc;
    return jpeg_color_slots(planes, a, m, pool, pool_frames, slots, s);
}

}  // namespace tstar
