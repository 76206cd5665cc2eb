// 16-byte copies between byte ranges of any alignment, for the kernels that move compressed JPEG bytes (jpeg_resident.hip,
// jpeg_recode.hip).  Device code only.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace tstar {
namespace jpegvec {

// bytes [a, a + 16) of the 32 bytes lo | hi, 0 < a < 16
__device__ inline uint4 funnel(const uint4& lo, const uint4& hi, uint32_t a) {
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t q = a >> 2, r = (a & 3) * 8;
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t x = 0, y = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)                  // q is uniform over the frame: selects, no indexed registers
            if (q == (uint32_t)k) { x = w[k + i]; y = w[k + i + 1]; }
        o[i] = (uint32_t)((((uint64_t)y << 32) | x) >> r);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// dst[0 .. n) = src[0 .. n) by the lanes t, t + stride, ... of a workgroup: single bytes up to dst's first 16-byte boundary
// and behind its last, 16-byte stores between them.  A store's 16 source bytes are one aligned load (source aligned with the
// destination), two aligned loads shifted together where both lie wholly inside [lo, hi) -- the memory around src that may be
// read -- or 16 single bytes.  No load leaves [lo, hi) or [src, src + n) otherwise; no store leaves [dst, dst + n).
__device__ inline void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t n, const uint8_t* lo, const uint8_t* hi, uint32_t t,
                                  uint32_t stride) {
    const uint32_t gap = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    const uint32_t head = gap < n ? gap : n;
    for (uint32_t i = t; i < head; i += stride) dst[i] = src[i];
    const uint32_t nvec = (n - head) / 16;
    const uint8_t* s = src + head;
    uint4* d = reinterpret_cast<uint4*>(dst + head);
    const uint32_t mis = (uint32_t)((uintptr_t)s & 15);
    for (uint32_t k = t; k < nvec; k += stride) {
        const uint8_t* at = s + 16 * (size_t)k;
        uint4 v;
        if (mis == 0) {
            v = *reinterpret_cast<const uint4*>(at);
        } else if (at - mis >= lo && at - mis + 32 <= hi) {
            const uint4* p = reinterpret_cast<const uint4*>(at - mis);
            v = funnel(p[0], p[1], mis);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t i = 0; i < 16; ++i) w[i >> 2] |= (uint32_t)at[i] << (8 * (i & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        d[k] = v;
    }
    for (uint32_t i = head + 16 * nvec + t; i < n; i += stride) dst[i] = src[i];
}

}  // namespace jpegvec
}  // namespace tstar
