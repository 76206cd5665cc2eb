// The convolutions of the YOLO-World backend (BASELINE configs[3]: "CSPDarknet conv path, no MFMA"): kernels, the per-layer
// launch policy and the launcher.  yolo.hip interprets the layer program and calls launch_conv; yolo_program.h holds what
// the program checker and the policy decide in common.
//   conv_valu_kernel     implicit-GEMM convolution on the f32 VALU (fmaf, no MFMA): 128 pixels x 64 channels per
//                        workgroup, 8 x 4 outputs per lane, K = (ky, kx, ci) staged through LDS in slices of 16 with
//                        ds_read_b128 fragment reads; fused bias / SiLU / residual / attention-gate epilogue; reads and
//                        writes at channel offsets so torch.cat never copies.  Bound: f32 VALU issue (157.3 TFLOP/s
//                        spec; tools/lab/pkfma_rate.hip measures 140 for a pure v_pk_fma_f32 stream at 8 waves / SIMD and
//                        108 at the 2 waves / SIMD a 128-accumulator tile leaves) shared with the LDS pipe.
//   conv_sw_kernel       the same convolution with the weights as SCALAR operands (s_load_dwordx16 rows of the transposed
//                        matrix feeding v_pk_fma_f32 from SGPRs): a quarter of the LDS traffic per FMA; used for the
//                        layers with >= 400 workgroups of 512 pixels x 64 channels (see the kernel's comment).
//   conv_halo_kernel     its form for 3x3 / stride-1 layers: an 8 x 40 output patch per workgroup, the 10 x 42 halo patch of a
//                        16-channel slice staged once and read by all nine taps.
//   conv_direct_kernel   small K (the 3-channel stem): the whole weight matrix in LDS.
//   transpose_w_kernel   the transposed weight copies, once per model.
#include "../../include/tstar_hip.h"
#include "yolo_conv.h"
#include "prof.h"
#include <math.h>
#include <stdlib.h>

namespace tstar {

// K is walked in slices of 16 input channels, the ks*ks taps of a slice back to back (the nine shifted reads of one
// 16-channel activation slice then hit the CU's L1: +2 % over tap-major order).  Every conv kernel uses this order, so
// their outputs are bit-identical.  Returns the (tap, first input channel) of slice k0 / 16; the weight row of its first
// k is tap * cin + ci.
template <int KS>
__device__ __forceinline__ void slice_pos(int k0, int& tap, int& ci) {
    const int sl = k0 / 16;
    tap = sl % (KS * KS);
    ci = (sl / (KS * KS)) * 16;
}

__device__ __forceinline__ float silu(float v) { return v / (1.0f + __expf(-v)); }

// ------------------------------------------------------------------ implicit-GEMM conv on the VALU
// Workgroup tile 16 TM pixels x BN channels (TM = 8 or 4: 128 or 64 pixels; BN = 64 or 128), K slices of 16; a lane owns
// TM pixels x TN channels (TN = 4 or 8).  The 64-pixel tile serves layers with fewer than 512 128-pixel tiles (small maps,
// small batches): twice the workgroups, so CUs hold two that overlap each other's barriers and load latency (L model
// forward: B = 1 15.7 -> 10.1 ms, B = 4 19.3 -> 16.2 ms).  Per k the lane reads 2 + TN/4 LDS quads for 8 TN FMAs: with TN = 8 the LDS pipe (shared by the CU's four
// SIMDs) carries 4 reads per 64 FMAs instead of 3 per 32, which is what keeps the VALU fed on the >= 128-channel layers.
// LDS rows k >= 8 are rotated by 8 floats: the transposing ds_write_b32 of lanes with k-quad 0 / 2 (and 1 / 3) would
// otherwise land on the same banks (row stride = 16 mod 32 banks); the b128 fragment reads stay 16-byte aligned.
template <int KS, int TN, int TM>
__global__ __launch_bounds__(256) void conv_valu_kernel(ConvArgs a, int mt, int nt) {
    constexpr int BN = 16 * TN, CLD_W = BN + 4, NWQ = BN / 64;       // NWQ weight float4 per thread per slice
    constexpr int CBM = 16 * TM, CLD_A = CBM + 4, NAQ = CBM / 64;    // TM = 8 (4): 128 (64) pixels per workgroup, NAQ activation float4 per thread
    constexpr int DEPTH = TN == 8 ? 1 : 3;                           // register prefetch depth in slices (the 8 x 8 tile has no registers to spare)
    __shared__ __attribute__((aligned(16))) float As[CBK][CLD_A];
    __shared__ __attribute__((aligned(16))) float Ws[CBK][CLD_W];
    const int tid = threadIdx.x;
    // 1-D grid, XCD-aware: an XCD gets a contiguous run of tiles, the channel tiles of one pixel tile adjacent (shared L2)
    const int tile = xcd_remap(blockIdx.x, mt * nt);
    const int m0 = (tile / nt) * CBM, n0 = (tile % nt) * BN;
    // staging roles: A tile 128 x 16 = 512 float4 -> 2 per thread (rows tid/4 and tid/4 + 64, k quad tid%4);
    //                W tile  BN x 16 -> NWQ per thread (rows tid/4 (+64))
    const int kq = (tid & 3) * 4;
    const int rot = (kq >> 3) * 8;                                   // column rotation of LDS rows k >= 8
    const int ar0 = tid >> 2;
    int ab[NAQ], ay[NAQ], ax[NAQ];
    bool aval[NAQ];
#pragma unroll
    for (int r = 0; r < NAQ; ++r) {
        const int m = m0 + ar0 + r * 64;
        aval[r] = m < a.M;
        const int mm = aval[r] ? m : 0;
        const int hw = a.Ho * a.Wo;
        ab[r] = mm / hw;
        const int rem = mm - ab[r] * hw;
        ay[r] = (rem / a.Wo) * a.stride - (KS >> 1);
        ax[r] = (rem % a.Wo) * a.stride - (KS >> 1);
    }
    const int K = KS * KS * a.cin;
    const float* wrow[NWQ];
#pragma unroll
    for (int r = 0; r < NWQ; ++r) {
        const int wn = n0 + ar0 + r * 64;
        wrow[r] = a.w + (size_t)(wn < a.cout ? wn : 0) * K + kq;   // rows >= cout read row 0: their outputs are never stored
    }

    // compute roles: 8 rows x TN cols per lane
    const int tx = tid & 15, ty = tid >> 4;                          // cols tx*4 (+64).., rows ty*8..
    float acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = 0.f;

    // global -> register staging, DEPTH = three slices deep (one for the 8 x 8 tile): a small layer runs one workgroup (or none) per CU, so nothing else hides
    // the L2 latency of a slice's loads; issued three slices ahead they have ~1.5 us to land.  Loads are unconditional
    // (a padded tap / out-of-range row reads a valid dummy address and is zeroed when the slice is stored; past the last
    // slice, slice 0 is re-read and dropped), which keeps them back to back and lets the in-order vmcnt wait be exact.
    struct Stage { f32x4 ra[NAQ], rw[NWQ]; unsigned ok; };
    auto load_tile = [&](Stage& st, int k0) {
        // k0 is a multiple of 16 and cin % 16 == 0, so the 16-wide slice stays inside one (ky, kx) tap
        if (k0 >= K) k0 = 0;
        int tap, ci0;
        slice_pos<KS>(k0, tap, ci0);
        const int ci = ci0 + kq, krow = tap * a.cin + ci0;
        const int ky = KS == 1 ? 0 : tap / KS, kx = KS == 1 ? 0 : tap - ky * KS;
        st.ok = 0;
#pragma unroll
        for (int r = 0; r < NAQ; ++r) {
            const int iy = ay[r] + ky, ix = ax[r] + kx;
            const bool ok = aval[r] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const size_t off = ok ? ((size_t)(ab[r] * a.H + iy) * a.W + ix) * a.src_ld + a.src_off + ci : (size_t)0;
            st.ra[r] = *reinterpret_cast<const f32x4*>(a.src + off);
            st.ok |= ok ? 1u << r : 0u;
        }
#pragma unroll
        for (int r = 0; r < NWQ; ++r) st.rw[r] = *reinterpret_cast<const f32x4*>(wrow[r] + krow);   // rows >= cout read row 0: their outputs are never stored
    };
    auto store_tile = [&](const Stage& st) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < NAQ; ++r) {
            const f32x4 v = ((st.ok >> r) & 1) ? st.ra[r] : z;
#pragma unroll
            for (int e = 0; e < 4; ++e) As[kq + e][(ar0 + r * 64 + rot) & (CBM - 1)] = v[e];
        }
#pragma unroll
        for (int r = 0; r < NWQ; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) Ws[kq + e][(ar0 + r * 64 + rot) & (BN - 1)] = st.rw[r][e];
    };
    auto step = [&](Stage& st, int k0) {
        __syncthreads();
        store_tile(st);
        __syncthreads();
        load_tile(st, k0 + DEPTH * CBK);
#pragma unroll
        for (int k = 0; k < CBK; ++k) {
            const int rk = (k >> 3) * 8;                             // compile-time after unrolling
            f32x4 av[TM / 4];
#pragma unroll
            for (int h2 = 0; h2 < TM / 4; ++h2) av[h2] = *reinterpret_cast<const f32x4*>(&As[k][(ty * TM + 4 * h2 + rk) & (CBM - 1)]);
            f32x4 w4[TN / 4];
#pragma unroll
            for (int q = 0; q < TN / 4; ++q) w4[q] = *reinterpret_cast<const f32x4*>(&Ws[k][(tx * 4 + q * 64 + rk) & (BN - 1)]);
#pragma unroll
            for (int q = 0; q < TN / 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
#pragma unroll
                        for (int h2 = 0; h2 < TM / 4; ++h2) acc[4 * h2 + i][q * 4 + j] = fmaf(av[h2][i], w4[q][j], acc[4 * h2 + i][q * 4 + j]);
                    }
                }
        }
    };
    if constexpr (DEPTH == 3) {
        Stage s0, s1, s2;
        load_tile(s0, 0);
        load_tile(s1, CBK);
        load_tile(s2, 2 * CBK);
        for (int k0 = 0;;) {                                         // the back edge always follows step(s2, ..)
            step(s0, k0); k0 += CBK; if (k0 >= K) break;
            step(s1, k0); k0 += CBK; if (k0 >= K) break;
            step(s2, k0); k0 += CBK; if (k0 >= K) break;
        }
    } else {
        Stage s0;
        load_tile(s0, 0);
        for (int k0 = 0; k0 < K; k0 += CBK) step(s0, k0);
    }
    // epilogue: bias, activation, residual (after the activation: DarknetBottleneck adds the identity last) or the
    // max-sigmoid attention gate (after project_conv's BatchNorm, no activation)
    const int ch_per_head = a.mode == MODE_ATTN_MUL ? a.cout / a.heads : 1;
#pragma unroll
    for (int q = 0; q < TN / 4; ++q) {
        const int nb = n0 + tx * 4 + q * 64;
        if (nb >= a.cout) continue;
        f32x4 bias = {0.f, 0.f, 0.f, 0.f};
        if (a.bias) bias = *reinterpret_cast<const f32x4*>(a.bias + nb);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + ty * TM + i;
            if (m >= a.M) continue;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = acc[i][q * 4 + j] + bias[j];
                if (a.act == YACT_SILU) t = silu(t);
                v[j] = t;
            }
            if (a.mode == MODE_RESIDUAL) {
                const f32x4 r = *reinterpret_cast<const f32x4*>(a.aux + (size_t)m * a.aux_ld + a.aux_off + nb);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] += r[j];
            } else if (a.mode == MODE_ATTN_MUL) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] *= a.aux[(size_t)m * a.aux_ld + a.aux_off + (nb + j) / ch_per_head];
            }
            *reinterpret_cast<f32x4*>(a.dst + (size_t)m * a.dst_ld + a.dst_off + nb) = v;
        }
    }
}

// ------------------------------------------------------------------ scalar-weight conv on the VALU
// The tile kernel above needs 16 LDS floats (8 pixels + 8 weights) per 64 FMAs and a lane; with the CU's four SIMDs on
// one LDS pipe that is as many LDS cycles as packed-FMA cycles, and neither pipe gets past half rate.  Here the weights
// never touch LDS or VGPRs: every lane of a wave works on the SAME 16 output channels, so the weight row of a k is
// wave-uniform -- one s_load_dwordx16 from the transposed matrix [K][cout] into SGPRs -- and feeds v_pk_fma_f32 as its
// scalar operand (channel pairs are the packed halves, the pixel value is broadcast with op_sel).  A lane owns P = 8 (or
// 4) pixels x 16 channels (128 / 64 accumulators: 2 / 4 waves per SIMD); the four waves of a workgroup share one 64 P-pixel
// x 16-k activation tile in LDS and take one 16-channel group each.  Per k and wave (P = 8): 2 ds_read_b128 + 1 s_load for 64
// v_pk_fma_f32, a quarter of the LDS traffic per FMA of the tile kernel.  Scalar loads are issued in batches of two k with the
// (out-of-order, hence lgkmcnt(0)) wait placed before the next batch; padded taps read a zero quad kept behind every
// activation buffer instead of branching.  The accumulation order over k is the same
// sequential fmaf chain (slice_pos), so all conv kernels give bit-identical outputs (tested).  Measured on the way (L model,
// B = 32 forward, ms): tile kernel only 80.5; + this kernel 73.3 (8 pixels per lane) / 70.0 (per-layer 4 or 8); DMA staging
// + slice-major K 68.3; 32-bit saddr addressing 67.0.  No gain: a second register stage of global prefetch, touching the
// next batch's weight rows to pre-load the scalar cache, 64-byte aligned rows alone.
constexpr int SWK = 16, SWN = 64;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
// acc.xy += a.x * w.xy  /  acc.xy += a.y * w.xy   (w in an SGPR pair)
__device__ __forceinline__ void pkfma_lo(f32x2& acc, f32x2 av, f32x2 w) { asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(av), "s"(w)); }
__device__ __forceinline__ void pkfma_hi(f32x2& acc, f32x2 av, f32x2 w) { asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(av), "s"(w)); }

template <int P>
__device__ __forceinline__ void conv_sw_epilogue(const ConvArgs& a, f32x2 (&acc)[P][8], int m0, int cg0, int lane) {
    // as in the tile kernel; a lane writes 16 consecutive channels of each of its P pixels
    const int ch_per_head = a.mode == MODE_ATTN_MUL ? a.cout / a.heads : 1;
    float bias[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) bias[c] = a.bias ? a.bias[cg0 + c] : 0.f;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int m = m0 + lane + 64 * j;
        if (m >= a.M) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = acc[j][2 * q + (e >> 1)][e & 1] + bias[4 * q + e];
                if (a.act == YACT_SILU) t = silu(t);
                v[e] = t;
            }
            const int nb = cg0 + 4 * q;
            if (a.mode == MODE_RESIDUAL) {
                const f32x4 r = *reinterpret_cast<const f32x4*>(a.aux + (size_t)m * a.aux_ld + a.aux_off + nb);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += r[e];
            } else if (a.mode == MODE_ATTN_MUL) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= a.aux[(size_t)m * a.aux_ld + a.aux_off + (nb + e) / ch_per_head];
            }
            *reinterpret_cast<f32x4*>(a.dst + (size_t)m * a.dst_ld + a.dst_off + nb) = v;
        }
    }
}

// The activation tile is staged by direct global -> LDS DMA (global_load_lds_dwordx4: no staging VGPRs, no ds_write
// phase) into a double-buffered tile: ONE barrier per slice, and the loads of slice s+1 land in the other
// buffer while slice s is computed.  A wave instruction fills 1 KB of LDS contiguously (lane L at byte 16 L), so tile rows
// are un-padded 64-byte pixel rows and the bank-conflict swizzle is applied on the GLOBAL side: slot q of pixel p holds
// k-quad q ^ ((p >> 2) & 3); the fragment read of k-quad kq then takes slot kq ^ ((lane >> 2) & 3), and the 16 lanes of a
// ds_read_b128 group (16 consecutive pixels) hit 16 distinct 16-byte slots.
template <int KS, int P>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(P == 8 ? 2 : 4, P == 8 ? 2 : 4))) void conv_sw_kernel(ConvArgs a, int mt, int nt) {
    constexpr int SWM = 64 * P;
    __shared__ __attribute__((aligned(16))) float As[2][SWM][SWK];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = xcd_remap(blockIdx.x, mt * nt);
    const int m0 = (tile / nt) * SWM;
    const int cg0 = (tile % nt) * SWN + wave * 16;
    const bool active = cg0 < a.cout;
    // staging roles: DMA instruction i of wave w fills pixels (4 i + w) 16 .. +15; lane L -> pixel (L >> 2), slot L & 3
    unsigned poff[P], pval[P];
    {
        const int hw = a.Ho * a.Wo;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int pl = (4 * i + wave) * 16 + (lane >> 2);              // pixel within the tile
            const int kq = (lane & 3) ^ ((pl >> 2) & 3);                   // the k-quad this slot holds
            const int m = m0 + pl;
            const bool ok = m < a.M;
            const int mm = ok ? m : 0;
            const int b = mm / hw, rem = mm - b * hw;
            const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
            const int y0 = oy * a.stride - (KS >> 1), x0 = ox * a.stride - (KS >> 1);
            poff[i] = 4u * (unsigned)(((b * a.H + y0) * a.W + x0) * a.src_ld + a.src_off + 4 * kq);   // BYTE offset from a.src; wraps for y0 / x0 = -1, only used with a valid tap
            unsigned v = 0;
#pragma unroll
            for (int t = 0; t < KS * KS; ++t) {
                const int iy = y0 + t / KS, ix = x0 + t % KS;
                v |= (unsigned)(ok && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) << t;
            }
            pval[i] = v;
        }
    }
    const int K = KS * KS * a.cin;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    auto stage = [&](int k0, int buf) {
        int tap, ci;
        slice_pos<KS>(k0, tap, ci);
        const int ky = KS == 1 ? 0 : tap / KS, kx = KS == 1 ? 0 : tap - ky * KS;
        const unsigned toff = 4u * (unsigned)((ky * a.W + kx) * a.src_ld + ci), tbit = 1u << tap, zoffb = 4u * a.zoff;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            // scalar base + 32-bit byte offset (zoff < 2^30 elements, launcher): bit test, add, select per load
            const unsigned off = (pval[i] & tbit) ? poff[i] + toff : zoffb;
            const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr)&As[buf][(4 * i + wave) * 16][0]);
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(off), "s"(a.src), "s"(la) : "memory");
        }
    };
    f32x2 acc[P][8];
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[j][c] = f32x2{0.f, 0.f};
    typedef __attribute__((address_space(4))) const f32x16 cw16;
    const float* wcol = a.wt + (active ? cg0 : 0);
    const int xs = ((lane >> 2) & 3) * 4;                                  // read-side swizzle, in floats

    stage(0, 0);
    int cur = 0;
    for (int k0 = 0; k0 < K; k0 += SWK) {
        int wtap, wci;
        slice_pos<KS>(k0, wtap, wci);
        const float* wrow0 = wcol + (size_t)(wtap * a.cin + wci) * a.cout;   // weight row of the slice's first k
        f32x16 wna = *(const cw16*)(unsigned long long)(wrow0);
        f32x16 wnb = *(const cw16*)(unsigned long long)(wrow0 + a.cout);
        __builtin_amdgcn_s_waitcnt(0x0F70);                                // vmcnt(0): this wave's DMA of slice k0 has landed
        __syncthreads();                                                    // everyone's has, and nobody still reads the other buffer
        if (k0 + SWK < K) stage(k0 + SWK, cur ^ 1);
        if (active) {
            const float* ab = &As[cur][lane][0];
            f32x4 av[P], an[P];
#pragma unroll
            for (int j = 0; j < P; ++j) av[j] = *reinterpret_cast<const f32x4*>(ab + j * 64 * SWK + (0 ^ xs));
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
#pragma unroll
                for (int kp = 0; kp < 2; ++kp) {
                    asm volatile("" :: "s"(wna[0]), "s"(wnb[0]));
                    __builtin_amdgcn_sched_barrier(0);
                    const f32x16 wa = wna, wb = wnb;
                    const int kn = kq * 4 + kp * 2 + 2;
                    if (kn < SWK) {
                        wna = *(const cw16*)(unsigned long long)(wrow0 + (size_t)kn * a.cout);
                        wnb = *(const cw16*)(unsigned long long)(wrow0 + (size_t)(kn + 1) * a.cout);
                    }
                    if (kp == 0 && kq < 3) {
#pragma unroll
                        for (int j = 0; j < P; ++j) an[j] = *reinterpret_cast<const f32x4*>(ab + j * 64 * SWK + ((4 * (kq + 1)) ^ xs));
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const f32x2 w2 = {wa[2 * c], wa[2 * c + 1]};
#pragma unroll
                        for (int j = 0; j < P; ++j) pkfma_lo(acc[j][c], kp ? f32x2{av[j][2], av[j][3]} : f32x2{av[j][0], av[j][1]}, w2);
                    }
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const f32x2 w2 = {wb[2 * c], wb[2 * c + 1]};
#pragma unroll
                        for (int j = 0; j < P; ++j) pkfma_hi(acc[j][c], kp ? f32x2{av[j][2], av[j][3]} : f32x2{av[j][0], av[j][1]}, w2);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (kq < 3) {
#pragma unroll
                    for (int j = 0; j < P; ++j) av[j] = an[j];
                }
            }
        }
        cur ^= 1;
    }
    if (!active) return;
    conv_sw_epilogue<P>(a, acc, m0, cg0, lane);
}

// ------------------------------------------------------------------ scalar-weight 3x3 conv with a halo tile
// For 3x3 / stride-1 layers: a workgroup owns a TH x TW patch of output pixels (320 of them: 8 x 40 on the 160-, 80- and
// 40-wide maps of a 640 x 640 input, 16 x 20 on the 20-wide maps) and stages the patch's halo of a 16-channel slice ONCE
// (9 DMA instructions per wave, out-of-image pixels from the zero quad); the nine taps then read shifted windows of it --
// every shift is an immediate ds_read offset -- instead of re-loading a shifted tile per tap as conv_sw_kernel does: 6.5x
// fewer DMA loads and two barriers per 144 k instead of one per 16.  Halo pixels are 80-byte rows (16 floats + one pad
// quad, filled by a fifth dummy lane so that a DMA instruction still writes 1 KB contiguously): consecutive pixels at an
// 80-byte stride make the ds_read_b128 of a 16-lane group conflict-free.  A lane owns 5 pixels x NCH channels.
//
// Patches are cut from the batch's images STACKED row-wise (row R = b * H + y; NHWC makes pixel (R, x) element R * W + x), so
// a map whose height is not a multiple of TH (20 rows under 16-row patches) still tiles without ragged patches: a patch may
// then span the boundary between two images, and the LDS halo gets ONE extra all-zero row at that boundary (XROW) -- it is the
// bottom padding of the upper image and the top padding of the lower one at once; the output rows below it just sit one
// halo row lower (a per-lane constant folded into the lane's base offset), so the tap loop is unchanged.
//
// NCH = 16 (3 waves per SIMD) is the form for layers with enough workgroups; NCH = 8 halves a wave's channel group (a
// workgroup covers 32 channels: twice the workgroups, 40 accumulators: 4 waves per SIMD) for the small layers and small
// batches, where 16-channel waves leave most SIMDs with one wave or none.  Same (ci slice, tap, k) fmaf order as every other
// conv kernel: bit-identical outputs.
constexpr int HLD = SWK + 4;
template <int TH, int TW, bool XROW> struct HaloGeom {
    static constexpr int HW2 = TW + 2, NROW = TH + 2 + (XROW ? 1 : 0), NP = NROW * HW2, P = TH * TW / 64;
    // LDS row pitch: HW2 pixels of 5 quads (4 data + 1 pad) plus 6 pad quads = 96 B.  A lane group of a ds_read_b128 covers 16
    // CONSECUTIVE patch pixels, which wrap from one patch row into the next (TW = 40 or 20 pixels per row); 16 pixels at 80 B
    // cover the 64 banks exactly once only if pixel 0 of the next row sits where pixel TW of this row would, i.e. the pitch is
    // TW * 80 B modulo the 256-B bank period: (TW + 2) * 80 + 96 (round 3 measured SQ_LDS_BANK_CONFLICT / SQ_BUSY_CYCLES = 0.51
    // on this kernel with the unpadded rows: every group that straddled two rows collided on two banks)
    static constexpr int RQ = HW2 * 5 + 6, RPF = RQ * 4;
    static constexpr int NDMA = (NROW * RQ + 63) / 64, NIT = (NDMA + 3) / 4, LDSF = NDMA * 256 + HLD;
    static_assert(TH * TW % 64 == 0, "a halo patch is a whole number of pixels per lane");
};
template <int N> struct WRow;
template <> struct WRow<16> { typedef f32x16 T; };
template <> struct WRow<8> { typedef float T __attribute__((ext_vector_type(8))); };

template <int TH, int TW, int NCH, bool XROW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NCH == 16 ? 3 : 4, NCH == 16 ? 3 : 4))) void conv_halo_kernel(ConvArgs a, int mt, int nt) {
    using G = HaloGeom<TH, TW, XROW>;
    constexpr int HW2 = G::HW2, HP = G::P, NIT = G::NIT, NDMA = G::NDMA, NC2 = NCH / 2;
    constexpr int RQ = G::RQ, RPF = G::RPF;
    __shared__ __attribute__((aligned(16))) float Hs[G::LDSF];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = xcd_remap(blockIdx.x, mt * nt);
    const int cg0 = (tile % nt) * (4 * NCH) + wave * NCH;
    const bool active = cg0 < a.cout;
    const int tpr = a.W / TW;
    const int rows_total = a.M / a.W;                                 // B * H stacked rows
    const int pt = tile / nt, row0 = (pt / tpr) * TH, x0 = (pt % tpr) * TW;
    // image boundary strictly inside the patch (XROW only; the launcher guarantees H >= TH, so there is at most one):
    // local row rb is the first row of the next image
    int rb = 1 << 20;
    if (XROW) {
        const int rem = row0 % a.H;
        if (rem != 0 && a.H - rem < TH) rb = a.H - rem;
    }
    const bool nb = XROW && rb < TH;
    const int last = TH + 1 + (nb ? 1 : 0);                           // LDS row of the bottom halo
    // staging roles: DMA instruction i = wave + 4 it fills LDS quads 64 i .. 64 i + 63; quad s = halo row s / RQ, and inside the row
    // pixel (s % RQ) / 5, quad (s % RQ) % 5 (quad 4 of a pixel and the six quads behind the last pixel are padding)
    unsigned hoff[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int sidx = (wave + 4 * it) * 64 + lane;
        const int hy = sidx / RQ, rem = sidx - hy * RQ;
        const int hx = rem / 5, q = rem - hx * 5;
        const int sr = row0 + hy - 1 - ((nb && hy > rb + 1) ? 1 : 0);  // stacked source row of LDS row hy
        const int ix = x0 + hx - 1;
        bool ok = hy < G::NROW && hx < HW2 && q < 4 && hy <= last && ix >= 0 && ix < a.W && sr >= 0 && sr < rows_total;
        if (nb && hy == rb + 1) ok = false;                            // the zero row between two images
        if (hy == 0 && row0 % a.H == 0) ok = false;                    // top halo above an image's first row
        if (hy == last && (row0 + TH) % a.H == 0) ok = false;          // bottom halo below an image's last row
        hoff[it] = ok ? 4u * (unsigned)((sr * a.W + ix) * a.src_ld + a.src_off + 4 * q) : 0xffffffffu;
    }
    typedef __attribute__((address_space(3))) void* lds_ptr;
    const unsigned zoffb = 4u * a.zoff;
    auto stage = [&](int ci0) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (wave + 4 * it < NDMA) {                                    // wave-uniform
                const unsigned off = hoff[it] == 0xffffffffu ? zoffb : hoff[it] + 4u * (unsigned)ci0;
                const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr)&Hs[0]) + (unsigned)(wave + 4 * it) * 1024u;
                asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(off), "s"(a.src), "s"(la) : "memory");
            }
        }
    };
    // compute roles: lane -> pixels p = lane + 64 j of the patch; hb[j] = its top-left tap in the halo patch (floats)
    int hb[HP];
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        const int p = lane + 64 * j, r = p / TW, c = p - r * TW;
        hb[j] = (r + ((nb && r >= rb) ? 1 : 0)) * RPF + c * HLD;
    }
    f32x2 acc[HP][NC2];
#pragma unroll
    for (int j = 0; j < HP; ++j)
#pragma unroll
        for (int c = 0; c < NC2; ++c) acc[j][c] = f32x2{0.f, 0.f};
    typedef typename WRow<NCH>::T wrow_t;
    typedef __attribute__((address_space(4))) const wrow_t cwrow;
    const float* wcol = a.wt + (active ? cg0 : 0);
    const float* hs = &Hs[0];

    for (int ci0 = 0; ci0 < a.cin; ci0 += SWK) {
        __syncthreads();                                                    // everybody is done with the previous slice's patch
        stage(ci0);
        __builtin_amdgcn_s_waitcnt(0x0F70);                                // vmcnt(0)
        __syncthreads();
        if (!active) continue;
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const int toff = ky * RPF + kx * HLD;                            // floats
            const float* wrow0 = wcol + (size_t)(tap * a.cin + ci0) * a.cout;
            wrow_t wna = *(cwrow*)(unsigned long long)(wrow0);
            wrow_t wnb = *(cwrow*)(unsigned long long)(wrow0 + a.cout);
            f32x4 av[HP], an[HP];
#pragma unroll
            for (int j = 0; j < HP; ++j) av[j] = *reinterpret_cast<const f32x4*>(hs + hb[j] + toff);
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
#pragma unroll
                for (int kp = 0; kp < 2; ++kp) {
                    asm volatile("" :: "s"(wna[0]), "s"(wnb[0]));
                    __builtin_amdgcn_sched_barrier(0);
                    const wrow_t wa = wna, wb = wnb;
                    const int kn = kq * 4 + kp * 2 + 2;
                    if (kn < SWK) {
                        wna = *(cwrow*)(unsigned long long)(wrow0 + (size_t)kn * a.cout);
                        wnb = *(cwrow*)(unsigned long long)(wrow0 + (size_t)(kn + 1) * a.cout);
                    }
                    if (kp == 0 && kq < 3) {
#pragma unroll
                        for (int j = 0; j < HP; ++j) an[j] = *reinterpret_cast<const f32x4*>(hs + hb[j] + toff + 4 * (kq + 1));
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c = 0; c < NC2; ++c) {
                        const f32x2 w2 = {wa[2 * c], wa[2 * c + 1]};
#pragma unroll
                        for (int j = 0; j < HP; ++j) pkfma_lo(acc[j][c], kp ? f32x2{av[j][2], av[j][3]} : f32x2{av[j][0], av[j][1]}, w2);
                    }
#pragma unroll
                    for (int c = 0; c < NC2; ++c) {
                        const f32x2 w2 = {wb[2 * c], wb[2 * c + 1]};
#pragma unroll
                        for (int j = 0; j < HP; ++j) pkfma_hi(acc[j][c], kp ? f32x2{av[j][2], av[j][3]} : f32x2{av[j][0], av[j][1]}, w2);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (kq < 3) {
#pragma unroll
                    for (int j = 0; j < HP; ++j) av[j] = an[j];
                }
            }
        }
    }
    if (!active) return;
    // epilogue (as conv_sw_epilogue, with the patch's pixel mapping)
    const int ch_per_head = a.mode == MODE_ATTN_MUL ? a.cout / a.heads : 1;
    float bias[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) bias[c] = a.bias ? a.bias[cg0 + c] : 0.f;
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        const int p = lane + 64 * j, r = p / TW, c0 = p - r * TW;
        if (row0 + r >= rows_total) continue;                              // ragged last patch of the stacked rows
        const size_t m = (size_t)(row0 + r) * a.W + x0 + c0;
#pragma unroll
        for (int q = 0; q < NCH / 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = acc[j][2 * q + (e >> 1)][e & 1] + bias[4 * q + e];
                if (a.act == YACT_SILU) t = silu(t);
                v[e] = t;
            }
            const int nb4 = cg0 + 4 * q;
            if (a.mode == MODE_RESIDUAL) {
                const f32x4 rr = *reinterpret_cast<const f32x4*>(a.aux + m * a.aux_ld + a.aux_off + nb4);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += rr[e];
            } else if (a.mode == MODE_ATTN_MUL) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= a.aux[m * a.aux_ld + a.aux_off + (nb4 + e) / ch_per_head];
            }
            *reinterpret_cast<f32x4*>(a.dst + m * a.dst_ld + a.dst_off + nb4) = v;
        }
    }
}

// W [cout][K] -> Wt [K][cout], once per model at tstar_yolo_create
__global__ __launch_bounds__(256) void transpose_w_kernel(const float* __restrict__ w, float* __restrict__ wt, int cout, int K) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)cout * K) return;
    const int n = (int)(i % cout), k = (int)(i / cout);
    wt[i] = w[(size_t)n * K + k];
}

// direct form for small K = ks*ks*cin (the 3-channel stem: K = 27): the whole weight matrix sits in LDS as [K][cout];
// a lane computes 4 neighbouring pixels x 16 output channels, so every weight quad read from LDS feeds 16 FMAs and the
// 64-channel output row of a pixel is written as 16-byte stores.  HBM-bound by its output (64 channels x 4 B per pixel).
constexpr int DPIX = 4;                                            // DCH: yolo_program.h
__global__ __launch_bounds__(256) void conv_direct_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wl[];      // [K][cout]
    const int K = a.ks * a.ks * a.cin;
    for (int i = threadIdx.x; i < K * a.cout; i += blockDim.x) {
        const int n = i % a.cout, k = i / a.cout;
        wl[i] = a.w[(size_t)n * K + k];
    }
    __syncthreads();
    const int ncg = a.cout / DCH;
    const int pq = threadIdx.x / ncg, cg = threadIdx.x % ncg;
    const int ppb = (blockDim.x / ncg) * DPIX;                       // pixels per block
    const int mbase = blockIdx.x * ppb + pq * DPIX;
    if (pq >= blockDim.x / ncg) return;
    float acc[DPIX][DCH];
#pragma unroll
    for (int i = 0; i < DPIX; ++i)
#pragma unroll
        for (int j = 0; j < DCH; ++j) acc[i][j] = 0.f;
    int pb[DPIX], py[DPIX], px[DPIX];
    const int hw = a.Ho * a.Wo;
#pragma unroll
    for (int i = 0; i < DPIX; ++i) {
        const int m = mbase + i < a.M ? mbase + i : a.M - 1;
        pb[i] = m / hw;
        const int rem = m - pb[i] * hw;
        py[i] = (rem / a.Wo) * a.stride - (a.ks >> 1);
        px[i] = (rem % a.Wo) * a.stride - (a.ks >> 1);
    }
    for (int ky = 0; ky < a.ks; ++ky)
        for (int kx = 0; kx < a.ks; ++kx)
            for (int c = 0; c < a.cin; ++c) {
                const float* wr = wl + (size_t)((ky * a.ks + kx) * a.cin + c) * a.cout + cg * DCH;
                f32x4 w4[DCH / 4];
#pragma unroll
                for (int q = 0; q < DCH / 4; ++q) w4[q] = *reinterpret_cast<const f32x4*>(wr + 4 * q);
#pragma unroll
                for (int i = 0; i < DPIX; ++i) {
                    const int iy = py[i] + ky, ix = px[i] + kx;
                    float v = 0.f;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = a.src[((size_t)(pb[i] * a.H + iy) * a.W + ix) * a.src_ld + a.src_off + c];
#pragma unroll
                    for (int q = 0; q < DCH / 4; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][4 * q + e] = fmaf(v, w4[q][e], acc[i][4 * q + e]);
                }
            }
#pragma unroll
    for (int i = 0; i < DPIX; ++i) {
        const int m = mbase + i;
        if (m >= a.M) continue;
        float* o = a.dst + (size_t)m * a.dst_ld + a.dst_off + cg * DCH;
#pragma unroll
        for (int q = 0; q < DCH / 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = acc[i][4 * q + e] + (a.bias ? a.bias[cg * DCH + 4 * q + e] : 0.f);
                if (a.act == YACT_SILU) t = silu(t);
                v[e] = t;
            }
            *reinterpret_cast<f32x4*>(o + 4 * q) = v;
        }
    }
}

// algorithmic HBM bytes of one conv launch: the input channels it reads (every input pixel once), the output channels it
// writes, the weights and bias, the residual / attention-gate tensor when fused
static double conv_algorithmic_bytes(const ConvArgs& a) {
    const double B = (double)a.M / ((double)a.Ho * a.Wo);
    double b = 4.0 * B * a.H * a.W * a.cin + 4.0 * a.M * a.cout + 4.0 * a.cout * a.ks * a.ks * a.cin + 4.0 * a.cout;
    if (a.mode == MODE_RESIDUAL) b += 4.0 * a.M * a.cout;
    else if (a.mode == MODE_ATTN_MUL) b += 4.0 * a.M * a.heads;
    return b;
}

// The launch policy's environment overrides (defaults in the initialisers); read once per process by conv_policy_env().
struct ConvPolicy {
    int sw = -1, sw_min = 400, sw_p = 0;                                   // TSTAR_YOLO_SW, _SW_MIN, _SW_P
    int halo = -1, halo_nch = 0, halo8_max = 600, halo8_min = 600;         // TSTAR_YOLO_HALO, _HALO_NCH, _HALO8_MAX, _HALO8_MIN
    int tn = 0, tm = 0, tm_min = 512;                                      // TSTAR_YOLO_TN, _TM, _TM_MIN
};

static const ConvPolicy& conv_policy_env() {
    static const ConvPolicy p = [] {
        ConvPolicy q;
        auto rd = [](const char* name, int& v) { const char* e = getenv(name); if (e) v = atoi(e); };
        rd("TSTAR_YOLO_SW", q.sw); rd("TSTAR_YOLO_SW_MIN", q.sw_min); rd("TSTAR_YOLO_SW_P", q.sw_p);
        rd("TSTAR_YOLO_HALO", q.halo); rd("TSTAR_YOLO_HALO_NCH", q.halo_nch); rd("TSTAR_YOLO_HALO8_MAX", q.halo8_max); rd("TSTAR_YOLO_HALO8_MIN", q.halo8_min);
        rd("TSTAR_YOLO_TN", q.tn); rd("TSTAR_YOLO_TM", q.tm); rd("TSTAR_YOLO_TM_MIN", q.tm_min);
        return q;
    }();
    return p;
}

// The per-layer policy: pure (dimensions, pointer PRESENCE and policy in, plan out; no HIP call), so it is testable without a GPU
// (tstar_yolo_conv_plan).  Only a.wt != null, a.zoff and the integers of `a` are read.
static ConvPlan plan_conv(const ConvArgs& a, const ConvPolicy& pol) {
    ConvPlan p;
    if (!(a.cout % 4 == 0 && a.dst_ld % 4 == 0 && a.dst_off % 4 == 0)) { p.error = "yolo conv: output channels must be 16-byte aligned"; return p; }
    const bool tiled = conv_tiled(a.cin, a.src_ld, a.src_off, a.ks);
    // scalar-weight form, chosen per layer from its size in 512-pixel x 64-channel blocks (per-layer timings of the L model
    // at B = 32, tools/rocpd_conv_align.py -> profiles/r02_yolo_conv_kernels_by_layer.md): >= 800 blocks: 4 pixels per lane
    // (256-pixel workgroups, 4 waves / SIMD); 400..799: 8 pixels per lane (one round of the chip's 512 two-per-CU slots);
    // below that the 128-pixel tiles of the tile kernel spread the layer over more CUs and win by up to 2x
    const int sw_env = pol.sw;
    const long long sw_blocks = (long long)cdiv(a.M, 512) * cdiv(a.cout, SWN);
    const bool sw_ok = tiled && a.wt && a.cout % 16 == 0 && a.zoff != 0 && a.zoff < (1u << 30);   // byte offsets fit 32 bits
    const int sw_min = pol.sw_min;
    const int sw_p_env = pol.sw_p;
    // halo form of the scalar-weight kernel for 3x3 / stride-1 layers.  Patch 8 x 40 on maps that tile by it (the 160-, 80-
    // and 40-wide ones), 16 x 20 over the row-stacked batch on 20-wide maps (H >= 16; one zero row at image boundaries).
    // From 320 workgroups of 16-channel waves up that form beats both other kernels on every such layer (B = 32: 10-15 %
    // per layer; B = 8: 221 vs 266 us at 320 workgroups, 445 vs 272 at 160 -- profiles/r02_yolo_conv_halo_by_layer_b*.md);
    // below HALO8_MAX (600) such workgroups the 8-channel-per-wave form takes over (twice the workgroups, 4 waves per SIMD: the
    // small maps and small batches, where 16-channel waves leave SIMDs empty), down to HALO8_MIN (600) of ITS workgroups: a
    // halo workgroup walks all of K, so a launch that does not fill the chip once still lasts one workgroup's ~430 us (256
    // input channels) and the tile kernel's many small workgroups win (B = 8, 40x40: 278 vs 426 us at 320 workgroups; B = 16,
    // 640: 440 vs 543) -- thresholds from profiles/r03_yolo_halo_forms_by_layer_*.md.  TSTAR_YOLO_HALO = 0 never / 2 always (when eligible);
    // TSTAR_YOLO_HALO_NCH = 8 / 16 forces the channel form.
    const int halo_env = pol.halo;
    const int nch_env = pol.halo_nch;
    const int halo8_max = pol.halo8_max;
    const int halo8_min = pol.halo8_min;
    const bool halo_3x3 = sw_ok && a.ks == 3 && a.stride == 1 && a.Ho == a.H && a.Wo == a.W;
    const bool halo_a = halo_3x3 && a.H % 8 == 0 && a.W % 40 == 0;                         // 8 x 40 patches, never across images
    const bool halo_b = halo_3x3 && !halo_a && a.W % 20 == 0 && a.H >= 16;                  // 16 x 20 patches over stacked rows
    const int rows_total = a.M / (a.W > 0 ? a.W : 1);
    const long long halo_mt = halo_a ? (long long)(rows_total / 8) * (a.W / 40) : halo_b ? (long long)cdiv(rows_total, 16) * (a.W / 20) : 0;
    const long long wgs16 = halo_mt * cdiv(a.cout, 64), wgs8 = halo_mt * cdiv(a.cout, 32);
    int halo_nch = 0;                                                                       // 0 = not the halo form
    if ((halo_a || halo_b) && halo_env != 0) {
        if (nch_env == 8 || nch_env == 16) halo_nch = (halo_env > 1 || (nch_env == 16 ? wgs16 >= 320 : wgs8 >= halo8_min)) ? nch_env : 0;
        else if (wgs16 >= halo8_max) halo_nch = 16;
        else if (wgs8 >= halo8_min || halo_env > 1) halo_nch = 8;
    }
    if (halo_nch) {
        p.mt = (int)halo_mt; p.nt = cdiv(a.cout, 4 * halo_nch);
        p.form = halo_a ? (halo_nch == 16 ? TSTAR_YOLO_FORM_HALO_A16 : TSTAR_YOLO_FORM_HALO_A8) : (halo_nch == 16 ? TSTAR_YOLO_FORM_HALO_B16 : TSTAR_YOLO_FORM_HALO_B8);
    } else if (sw_ok && (sw_env < 0 ? sw_blocks >= sw_min : sw_env > 0)) {
        const int sw_p = sw_p_env ? sw_p_env : (sw_blocks >= 800 ? 4 : 8);
        p.mt = cdiv(a.M, 64 * sw_p); p.nt = cdiv(a.cout, SWN);
        p.form = sw_p == 8 ? TSTAR_YOLO_FORM_SW8 : TSTAR_YOLO_FORM_SW4;
    } else if (tiled) {
        // 128-channel tiles (8 x 8 outputs per lane) when the layer has the channels and enough pixels to fill the chip;
        // 64-pixel tiles (4 x 4 per lane) when 128-pixel tiles would leave CUs without a workgroup to overlap with
        const int tn_env = pol.tn;
        const int tm_env = pol.tm;
        const int tm_min = pol.tm_min;
        const bool wide = tn_env ? tn_env == 8 : (a.cout % 128 == 0 && (long long)cdiv(a.M, 128) * (a.cout / 128) >= 512);
        const bool small = !wide && (tm_env ? tm_env == 4 : (long long)cdiv(a.M, 128) * cdiv(a.cout, 64) < tm_min);
        p.mt = cdiv(a.M, small ? 64 : 128); p.nt = cdiv(a.cout, wide ? 128 : 64);
        p.form = wide ? TSTAR_YOLO_FORM_WIDE : small ? TSTAR_YOLO_FORM_TILE64 : TSTAR_YOLO_FORM_TILE128;
    } else {
        if (const DirectRefusal* r = direct_form_error(a.cin, a.ks, a.cout, a.mode)) { p.error = r->in_plan; return p; }
        const int ncg = a.cout / DCH, nthreads = (256 / ncg) * ncg, ppb = (nthreads / ncg) * DPIX;
        p.mt = cdiv(a.M, ppb); p.nt = nthreads;
        p.form = TSTAR_YOLO_FORM_DIRECT;
    }
    return p;
}

int launch_conv(const ConvArgs& a, hipStream_t s, int* form_out) {
    const ConvPlan p = plan_conv(a, conv_policy_env());
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    if (form_out) *form_out = p.form;
    const int mt = p.mt, nt = p.nt;
    const dim3 grid(mt * nt);
    const bool prof = p.form != TSTAR_YOLO_FORM_DIRECT && prof_enabled();
    if (prof) prof_start(PROF_CONV, s, 2.0 * a.M * a.cout * a.ks * a.ks * a.cin, conv_algorithmic_bytes(a));
    switch (p.form) {
    case TSTAR_YOLO_FORM_HALO_A16: hipLaunchKernelGGL((conv_halo_kernel<8, 40, 16, false>), grid, dim3(256), 0, s, a, mt, nt); break;
    case TSTAR_YOLO_FORM_HALO_A8: hipLaunchKernelGGL((conv_halo_kernel<8, 40, 8, false>), grid, dim3(256), 0, s, a, mt, nt); break;
    case TSTAR_YOLO_FORM_HALO_B16: hipLaunchKernelGGL((conv_halo_kernel<16, 20, 16, true>), grid, dim3(256), 0, s, a, mt, nt); break;
    case TSTAR_YOLO_FORM_HALO_B8: hipLaunchKernelGGL((conv_halo_kernel<16, 20, 8, true>), grid, dim3(256), 0, s, a, mt, nt); break;
    case TSTAR_YOLO_FORM_SW8:
        if (a.ks == 1) hipLaunchKernelGGL((conv_sw_kernel<1, 8>), grid, dim3(256), 0, s, a, mt, nt);
        else hipLaunchKernelGGL((conv_sw_kernel<3, 8>), grid, dim3(256), 0, s, a, mt, nt);
        break;
    case TSTAR_YOLO_FORM_SW4:
        if (a.ks == 1) hipLaunchKernelGGL((conv_sw_kernel<1, 4>), grid, dim3(256), 0, s, a, mt, nt);
        else hipLaunchKernelGGL((conv_sw_kernel<3, 4>), grid, dim3(256), 0, s, a, mt, nt);
        break;
    case TSTAR_YOLO_FORM_WIDE:
        if (a.ks == 1) hipLaunchKernelGGL((conv_valu_kernel<1, 8, 8>), grid, dim3(256), 0, s, a, mt, nt);
        else hipLaunchKernelGGL((conv_valu_kernel<3, 8, 8>), grid, dim3(256), 0, s, a, mt, nt);
        break;
    case TSTAR_YOLO_FORM_TILE64:
        if (a.ks == 1) hipLaunchKernelGGL((conv_valu_kernel<1, 4, 4>), grid, dim3(256), 0, s, a, mt, nt);
        else hipLaunchKernelGGL((conv_valu_kernel<3, 4, 4>), grid, dim3(256), 0, s, a, mt, nt);
        break;
    case TSTAR_YOLO_FORM_TILE128:
        if (a.ks == 1) hipLaunchKernelGGL((conv_valu_kernel<1, 4, 8>), grid, dim3(256), 0, s, a, mt, nt);
        else hipLaunchKernelGGL((conv_valu_kernel<3, 4, 8>), grid, dim3(256), 0, s, a, mt, nt);
        break;
    default:                                                                                // TSTAR_YOLO_FORM_DIRECT: mt blocks of nt threads
        hipLaunchKernelGGL(conv_direct_kernel, dim3(mt), dim3(nt), (size_t)a.ks * a.ks * a.cin * a.cout * 4, s, a);
        break;
    }
    if (prof) prof_stop(PROF_CONV, s);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

// element offset of the zero quad behind a source buffer of max_batch images; 0 = beyond the 32-bit byte offsets of the scalar-weight forms
static unsigned conv_zoff(int max_batch, int H, int W, int ld) {
    const size_t zo = (size_t)max_batch * H * W * ld;
    return zo < (1ull << 30) ? (unsigned)zo : 0;
}

ConvArgs conv_args(const YoloProgram& p, const YoloConvOp& c, int B, int max_batch) {
    const YoloBuf &src = p.bufs[c.src], &dst = p.bufs[c.dst];
    ConvArgs a{};
    a.src_ld = src.C; a.src_off = c.src_off; a.cin = c.cin; a.H = src.H; a.W = src.W;
    a.dst_ld = dst.C; a.dst_off = c.dst_off; a.cout = c.cout; a.Ho = dst.H; a.Wo = dst.W;
    a.ks = c.ks; a.stride = c.stride; a.act = c.act; a.mode = c.mode;
    if (c.mode != MODE_PLAIN) { a.aux_ld = p.bufs[c.aux].C; a.aux_off = c.aux_off; a.heads = p.bufs[c.aux].C; }
    a.M = B * a.Ho * a.Wo;
    a.zoff = conv_zoff(max_batch, a.H, a.W, a.src_ld);
    return a;
}

int launch_transpose_w(const float* w, float* wt, int cout, int K, hipStream_t s) {
    hipLaunchKernelGGL(transpose_w_kernel, dim3(cdiv(cout * K, 256)), dim3(256), 0, s, w, wt, cout, K);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

}  // namespace tstar

using namespace tstar;

extern "C" {

int tstar_yolo_conv_plan(int cin, int src_ld, int src_off, int H, int W, int cout, int dst_ld, int dst_off, int ks, int stride, int mode, int B,
                         int max_batch, int env_policy, int* plan3) {
    TSTAR_REQUIRE(plan3, "tstar_yolo_conv_plan: null argument");
    TSTAR_REQUIRE(cin >= 1 && cout >= 1 && H >= 1 && W >= 1 && src_ld >= 1 && dst_ld >= 1 && src_off >= 0 && dst_off >= 0 && (ks == 1 || ks == 3) &&
                  (stride == 1 || stride == 2) && B >= 1 && B <= max_batch && max_batch <= 1024,
                  "tstar_yolo_conv_plan: not a conv op tstar_yolo_create accepts");
    // the arguments run_program derives from the op of a one-op program (buffer 0 -> buffer 1, which is also the residual / gate
    // buffer) of a handle with max_batch images per buffer; every conv op has a transposed matrix
    YoloProgram p;
    p.bufs = {{H, W, src_ld}, {conv_out_size(H, ks, stride), conv_out_size(W, ks, stride), dst_ld}};
    const YoloConvOp c{0, src_off, cin, 1, dst_off, cout, ks, stride, YACT_NONE, 0, -1, mode, 1, 0};
    ConvArgs a = conv_args(p, c, B, max_batch);
    static const float wt_present = 0.f;
    a.wt = &wt_present;
    const ConvPlan pl = plan_conv(a, env_policy ? conv_policy_env() : ConvPolicy{});
    if (pl.error) { set_error(pl.error); return TSTAR_ERR_ARG; }
    plan3[0] = pl.form; plan3[1] = pl.mt; plan3[2] = pl.nt;
    return TSTAR_OK;
}

}  // extern "C"
