// Shared helpers for the tstar_hip C-ABI library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

namespace tstar {

// last error string, thread-local; returned by tstar_last_error()
void set_error(const std::string& msg);

#define TSTAR_HIP_CHECK(expr)                                                        \
    do {                                                                             \
        hipError_t _e = (expr);                                                      \
        if (_e != hipSuccess) {                                                      \
            ::tstar::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));   \
            return TSTAR_ERR_HIP;                                                    \
        }                                                                            \
    } while (0)

#define TSTAR_REQUIRE(cond, msg)                                                     \
    do {                                                                             \
        if (!(cond)) {                                                               \
            ::tstar::set_error(std::string(msg) + " (" #cond ")");                  \
            return TSTAR_ERR_ARG;                                                    \
        }                                                                            \
    } while (0)

#define RC(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

// a query-set slot of either detector handle (fn: the entry's name, a literal or a std::string)
#define TSTAR_CHECK_SET(set, fn) TSTAR_REQUIRE((set) >= 0 && (set) < TSTAR_OWL_MAX_SETS, std::string(fn) + ": query_set must be in 0..63")

// hipFuncAttributeMaxDynamicSharedMemorySize for kernels that need more than 64 KB of dynamic LDS: set once per
// (kernel, device) under a mutex -- launches may come from several host threads and a process may use more than
// one device (the attribute is applied to the kernel's code object of the CURRENT device).  Returns TSTAR_OK / TSTAR_ERR_HIP.
int ensure_dyn_lds(const void* kernel, int bytes);

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Bijective XCD-aware remap of a 1-D block id: the dispatcher places block b on
// XCD b % 8 (observed, speed only); give each XCD a contiguous chunk of the
// tile space so neighbouring tiles share that XCD's private L2.
__host__ __device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int nx = 8;
    int xcd = bid % nx, idx = bid / nx;
    int q = nwg / nx, r = nwg % nx;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// The same remap for blocks that come in GROUPS of gsize which share operands (the query tiles of one (image, head)): the whole
// group must sit on ONE XCD, which no permutation of ngroups * gsize ids can give unless every XCD's share is a multiple of gsize.
// So the grid is padded to xcd_groups_grid() blocks: XCD x runs its blocks bid = 8 idx + x in order, gsize consecutive idx are one
// group, group slot (idx / gsize) * 8 + x goes through xcd_remap over the groups, and the slots past ngroups (fewer than 8 groups'
// worth of blocks) return -1: they exit at once.  The live blocks map one-to-one onto 0 .. ngroups * gsize - 1.
static inline int xcd_groups_grid(int ngroups, int gsize) { return (ngroups + 7) / 8 * 8 * gsize; }
__host__ __device__ __forceinline__ int xcd_remap_groups(int bid, int ngroups, int gsize) {
    const int xcd = bid % 8, idx = bid / 8;
    const int slot = (idx / gsize) * 8 + xcd;
    return slot < ngroups ? xcd_remap(slot, ngroups) * gsize + idx % gsize : -1;
}

// 12 bytes of 4 consecutive RGB pixels -> three aligned dword stores (d dword-aligned: rows are multiples of 4 pixels;
// byte stores of single channels were the resize kernel's limiter: 3 strided store instructions per pixel)
__device__ __forceinline__ void store_px4(uint8_t* d, const unsigned (&v)[4][3]) {
    uint3 o;
    o.x = v[0][0] | (v[0][1] << 8) | (v[0][2] << 16) | (v[1][0] << 24);
    o.y = v[1][1] | (v[1][2] << 8) | (v[2][0] << 16) | (v[2][1] << 24);
    o.z = v[2][2] | (v[3][0] << 8) | (v[3][1] << 16) | (v[3][2] << 24);
    *reinterpret_cast<uint3*>(d) = o;
}

// numpy's float64 floor_divide (npy_divmod: fmod-based) for a >= 0, b > 0 -- what `np.float32 // Python float` is under the
// reference's pinned numpy 1.26.  floor(a / b) is NOT the same number when b is a rounded quotient (800 / 6) and a sits on a
// multiple of it: 400.0 / 133.33333333333334 rounds to 3.0, while 400.0 holds only two whole 133.33333333333334s.
__device__ __forceinline__ double np_floor_divide(double a, double b) {
    const double mod = fmod(a, b);
    const double div = (a - mod) / b;
    const double f = floor(div);
    return div - f > 0.5 ? f + 1.0 : f;
}

}  // namespace tstar

#define TSTAR_OK 0
#define TSTAR_ERR_ARG 1
#define TSTAR_ERR_HIP 2
#define TSTAR_ERR_STATE 3
