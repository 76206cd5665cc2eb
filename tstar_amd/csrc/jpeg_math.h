// The integer arithmetic of the JPEG reconstruction, stated once for the host reference (jpeg_host.cpp) and the
// kernels (jpeg.hip): libjpeg's accurate integer IDCT (Loeffler-Ligtenberg-Moschytz, constants x 2^13), "fancy"
// triangle chroma upsampling and the 16-bit fixed-point YCbCr -> RGB map.  Bit-equal to libjpeg-turbo as Pillow
// drives it; every product wraps in uint32 so that a corrupt stream's huge coefficients are defined behaviour.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TSTAR_JHD __host__ __device__ __forceinline__
#else
#define TSTAR_JHD inline
#endif

namespace tstar {
namespace jpegmath {

// (v + 2^(n-1)) >> n, arithmetic shift, on a wrapped 32-bit value
TSTAR_JHD int32_t descale(uint32_t v, int n) { return (int32_t)(v + (1u << (n - 1))) >> n; }

// One 8-point pass.  in / out: eight 32-bit values (two's complement in uint32); shift 11 after the column pass, 18 after
// the row pass.
TSTAR_JHD void idct8(const uint32_t x[8], int32_t out[8], int shift) {
    uint32_t z1 = (x[2] + x[6]) * 4433u;
    uint32_t t2 = z1 - x[6] * 15137u;
    uint32_t t3 = z1 + x[2] * 6270u;
    uint32_t t0 = (x[0] + x[4]) << 13;
    uint32_t t1 = (x[0] - x[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = x[7]; t1 = x[5]; t2 = x[3]; t3 = x[1];
    z1 = t0 + t3;
    uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 *= (uint32_t)-16069; z4 *= (uint32_t)-3196;
    z3 += z5; z4 += z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    out[0] = descale(t10 + t3, shift); out[7] = descale(t10 - t3, shift);
    out[1] = descale(t11 + t2, shift); out[6] = descale(t11 - t2, shift);
    out[2] = descale(t12 + t1, shift); out[5] = descale(t12 - t1, shift);
    out[3] = descale(t13 + t0, shift); out[4] = descale(t13 - t0, shift);
}

// The reduced-size passes of a decode at 1/2, 1/4 and 1/8 scale (libjpeg's jidctred.c, constants x 2^13): the same 1-D routine
// over the columns (pass 1), then over the rows (pass 2) of the low-frequency corner of the block, x = the eight values of the
// column / row.  Unread elements may hold anything.
// 4 outputs; x[4] is never read, and pass 1 leaves column 4 out.  shift 12 after the column pass, 19 after the row pass.
TSTAR_JHD void idct4(const uint32_t x[8], int32_t out[4], int shift) {
    const uint32_t t0 = x[0] << 14;
    const uint32_t t2 = x[2] * 15137u - x[6] * 6270u;
    const uint32_t t10 = t0 + t2, t12 = t0 - t2;
    const uint32_t a = x[7] * (uint32_t)-1730 + x[5] * 11893u + x[3] * (uint32_t)-17799 + x[1] * 8697u;
    const uint32_t b = x[7] * (uint32_t)-4176 + x[5] * (uint32_t)-4926 + x[3] * 7373u + x[1] * 20995u;
    out[0] = descale(t10 + b, shift); out[3] = descale(t10 - b, shift);
    out[1] = descale(t12 + a, shift); out[2] = descale(t12 - a, shift);
}

// 2 outputs; reads x[0], x[1], x[3], x[5], x[7], and pass 1 runs over those columns only.  shift 13 after the column pass, 20
// after the row pass.
TSTAR_JHD void idct2(const uint32_t x[8], int32_t out[2], int shift) {
    const uint32_t t10 = x[0] << 15;
    const uint32_t t = x[7] * (uint32_t)-5906 + x[5] * 6967u + x[3] * (uint32_t)-10426 + x[1] * 29692u;
    out[0] = descale(t10 + t, shift); out[1] = descale(t10 - t, shift);
}

// 1 output: the dequantised DC term alone
TSTAR_JHD int32_t idct1(uint32_t dc) { return descale(dc, 3); }

// does a pass of output size k (8, 4, 2) read element / column i of the block?
TSTAR_JHD bool idct_reads(int k, int i) { return k == 8 || (k == 4 ? i != 4 : (i < 2 || (i & 1))); }

TSTAR_JHD int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
TSTAR_JHD uint8_t range_limit(int32_t v) { return (uint8_t)clamp255(v + 128); }
TSTAR_JHD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Chroma sample for output pixel (x, y) from a plane of true size cw x ch (row pitch `pitch`; never reads beyond cw / ch,
// the MCU padding right of / below them holds no picture).  hs, vs: the luma sampling factors.
TSTAR_JHD int upsample_at(const uint8_t* p, int pitch, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * pitch + x];
    const int i = x >> 1, il = i > 0 ? i - 1 : 0, ir = i < cw - 1 ? i + 1 : cw - 1;
    const int in = (x & 1) ? ir : il;                              // odd output leans right, even leans left
    if (vs == 1) {
        const uint8_t* r = p + (size_t)y * pitch;
        return (3 * r[i] + r[in] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int j = y >> 1;
    const int jn = (y & 1) ? (j < ch - 1 ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);   // lower output row takes the row below
    const uint8_t* r0 = p + (size_t)j * pitch;
    const uint8_t* r1 = p + (size_t)jn * pitch;
    const int a = 3 * r0[i] + r1[i], b = 3 * r0[in] + r1[in];
    return (3 * a + b + ((x & 1) ? 7 : 8)) >> 4;
}

// Chroma sample for output pixel (x, y) of a scaled decode (jpeg_host.h JpegScaledGeom): mode 0 the plane is as large as the
// picture, 1 half width through the triangle filter above, 2 half width, every sample twice.
TSTAR_JHD int chroma_at(const uint8_t* p, int pitch, int cw, int ch, int mode, int x, int y) {
    if (mode == 2) return p[(size_t)y * pitch + (x >> 1)];
    return upsample_at(p, pitch, cw, ch, mode == 1 ? 2 : 1, 1, x, y);
}

// F(x) = int(x * 65536 + 0.5)
TSTAR_JHD void ycc_to_rgb(int y, int cb, int cr, uint8_t* rgb) {
    cb -= 128; cr -= 128;
    rgb[0] = (uint8_t)clamp255(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = (uint8_t)clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    rgb[2] = (uint8_t)clamp255(y + ((116130 * cb + 32768) >> 16));
}

}  // namespace jpegmath
}  // namespace tstar
