// YOLO-World-v2 image path on gfx950 WITHOUT the matrix cores (BASELINE configs[3]: "CSPDarknet conv path, no
// MFMA"): the second detector backend behind the reference's heuristic plug-in surface.
//
// Replaces YoloWorldInterface.inference_detector (/root/reference/TStar/interface_heuristic.py:136-168: mmdet test
// pipeline on images[0], model.test_step, score > 0.12, top-50) and, for the searcher's fast path, the
// detection -> grid-cell loop of TStarSearcher.imageGridScoreFunction (interface_searcher.py:129-150).  The model
// source is NOT part of the reference tree (dangling symlink; mmdet/mmyolo absent): the architecture is restated from
// the published YOLO-World-v2 design and its parity is UNPINNED -- see oracle/yolo_ref.py; tests compare this file
// against that independent CPU statement on seeded weights.
//
// The network is data: tstar_amd/yolo_world.py flattens it into a float32 blob (BatchNorm folded) and a table of ops
// over NHWC activation buffers.  yolo_program.h defines that table and checks it (pure, no HIP); this file holds the handle,
// interprets the decoded program and runs the test pipeline and the tail; the convolutions are in yolo_conv.hip.
//   pool5 / upcopy / attn / letterbox / head_decode  HBM-bound elementwise & small reductions (wave shuffles).
//   sort_nms_kernel      per image: bitonic sort of the (score, anchor, class) candidates, class-aware greedy NMS run by
//                        ONE wavefront (kept boxes in LDS, lanes test them in parallel, __ballot decides), top-k.
#include "../../include/tstar_hip.h"
#include "common.h"
#include "device_buf.h"
#include "heads.h"
#include "ingest.h"
#include "yolo_conv.h"
#include "yolo_program.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace tstar {

constexpr int YOLO_SETS = TSTAR_OWL_MAX_SETS;
constexpr int YOLO_NMS_PRE = 30000, YOLO_MAX_PER_IMG = 300;
constexpr float YOLO_IOU_THR = 0.7f, YOLO_SCORE_THR = 0.001f;

// ------------------------------------------------------------------ elementwise ops
// SPPF: dst[.., doff + c] = max over the 5x5 window (stride 1, pad 2, -inf padding) of src[.., soff + c]
__global__ __launch_bounds__(256) void pool5_kernel(const float* __restrict__ buf, int ld, int soff, int doff, int C, int H, int W, float* __restrict__ out, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int cq = C / 4;
    const int c = (int)(gid % cq) * 4;
    const size_t p = gid / cq;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const size_t img = p / ((size_t)W * H);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(buf + ((img * H + yy) * W + xx) * ld + soff + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], v[j]);
        }
    }
    *reinterpret_cast<f32x4*>(out + p * ld + doff + c) = m;
}

// dst[b, y, x, doff + c] = src[b, y / f, x / f, soff + c]   (f = 1: channel-offset copy; f = 2: nearest upsample)
__global__ __launch_bounds__(256) void upcopy_kernel(const float* __restrict__ src, int sld, int soff, int C, int Hs, int Ws, int f,
                                                     float* __restrict__ dst, int dld, int doff, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int cq = C / 4;
    const int c = (int)(gid % cq) * 4;
    const size_t p = gid / cq;
    const int Wd = Ws * f, Hd = Hs * f;
    const int x = (int)(p % Wd), y = (int)((p / Wd) % Hd);
    const size_t img = p / ((size_t)Wd * Hd);
    *reinterpret_cast<f32x4*>(dst + p * dld + doff + c) =
        *reinterpret_cast<const f32x4*>(src + ((img * Hs + y / f) * Ws + x / f) * sld + soff + c);
}

// MaxSigmoidAttnBlock gate: attn[p, m] = sigmoid(max_n <embed[p, m, :], guide[n, m, :]> / sqrt(hc) + bias[m]);
// guide = guide_fc(text) of the image's query set, [Q][embed] per set, staged in LDS
__global__ __launch_bounds__(256) void attn_kernel(const float* __restrict__ emb, int ld, int off, int embed, int heads, int HW,
                                                   const float* __restrict__ guide_all, const int* __restrict__ setQ,
                                                   const int* __restrict__ image_set, const float* __restrict__ bias,
                                                   float* __restrict__ attn, int P) {
    extern __shared__ __attribute__((aligned(16))) float g[];   // [Q][embed]
    const int img = blockIdx.y;
    const int set = image_set ? image_set[img] : 0;
    const int Q = setQ[set];
    const float* gs = guide_all + (size_t)set * YOLO_MAX_Q * embed;
    for (int i = threadIdx.x; i < Q * embed; i += blockDim.x) g[i] = gs[i];
    __syncthreads();
    const int hc = embed / heads;
    const float inv = 1.0f / sqrtf((float)hc);
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < HW * heads; t += gridDim.x * blockDim.x) {
        const int pix = t / heads, m = t - pix * heads;
        const size_t p = (size_t)img * HW + pix;
        const float* e = emb + p * ld + off + m * hc;
        float best = -INFINITY;
        if (hc == 32 && ((ld | off) & 3) == 0) {
            // the pixel's 32 head channels once, as eight 16-byte loads (every published scale has 32 channels per head); the
            // guide vectors come from LDS as float4 too.  Same sequential fmaf order as the scalar loop.
            f32x4 ev[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) ev[q] = *reinterpret_cast<const f32x4*>(e + 4 * q);
            for (int n = 0; n < Q; ++n) {
                const f32x4* gv = reinterpret_cast<const f32x4*>(g + n * embed + m * 32);
                float d = 0.f;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const f32x4 w = gv[q];
                    d = fmaf(ev[q][0], w[0], d); d = fmaf(ev[q][1], w[1], d); d = fmaf(ev[q][2], w[2], d); d = fmaf(ev[q][3], w[3], d);
                }
                best = fmaxf(best, d);
            }
        } else {
            for (int n = 0; n < Q; ++n) {
                const float* gv = g + n * embed + m * hc;
                float d = 0.f;
                for (int c = 0; c < hc; ++c) d = fmaf(e[c], gv[c], d);
                best = fmaxf(best, d);
            }
        }
        const float v = best * inv + bias[m];
        attn[p * heads + m] = 1.0f / (1.0f + __expf(-v));
    }
}

// guide[set][n][e] = guide_fc(text_n) = W[e,:] . t_n + b[e]
__global__ void guide_fc_kernel(const float* __restrict__ text, int Q, const float* __restrict__ W, const float* __restrict__ b,
                                int embed, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q * embed) return;
    const int n = i / embed, e = i - n * embed;
    const float* t = text + (size_t)n * YOLO_TEXT;
    const float* w = W + (size_t)e * YOLO_TEXT;
    float d = 0.f;
    for (int c = 0; c < YOLO_TEXT; ++c) d = fmaf(t[c], w[c], d);
    out[i] = d + b[e];
}

// F.normalize(text, dim=-1): t / max(||t||, 1e-12); one wave per query
__global__ void text_normalize_kernel(const float* __restrict__ in, float* __restrict__ out) {
    const int q = blockIdx.x, lane = threadIdx.x;
    float v[8], s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = in[(size_t)q * YOLO_TEXT + i * 64 + lane]; s += v[i] * v[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float den = fmaxf(sqrtf(s), 1e-12f);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[(size_t)q * YOLO_TEXT + i * 64 + lane] = v[i] / den;
}

// ------------------------------------------------------------------ test pipeline
// INTER_AREA-style down-scale (the build's definition: exact-footprint box average in integers): per axis, output o
// covers source units [o*n_in, (o+1)*n_in) of 1/n_out pixel.  u8 [B,H,W,3] -> u8 [B,oh,ow,3]
__global__ __launch_bounds__(256) void area_resize_kernel(const uint8_t* __restrict__ in, int H, int W, uint8_t* __restrict__ out, int oh, int ow, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int ox = (int)(gid % ow), oy = (int)((gid / ow) % oh);
    const size_t img = gid / ((size_t)ow * oh);
    const long long xlo = (long long)ox * W, xhi = xlo + W, ylo = (long long)oy * H, yhi = ylo + H;
    const int px0 = (int)(xlo / ow), px1 = (int)((xhi - 1) / ow), py0 = (int)(ylo / oh), py1 = (int)((yhi - 1) / oh);
    long long acc[3] = {0, 0, 0};
    for (int py = py0; py <= py1; ++py) {
        const long long a = (long long)py * oh, b = a + oh;
        const long long wy = (yhi < b ? yhi : b) - (ylo > a ? ylo : a);
        long long row[3] = {0, 0, 0};
        for (int px = px0; px <= px1; ++px) {
            const long long c = (long long)px * ow, d = c + ow;
            const long long wx = (xhi < d ? xhi : d) - (xlo > c ? xlo : c);
            const uint8_t* q = in + ((img * H + py) * W + px) * 3;
            row[0] += wx * q[0]; row[1] += wx * q[1]; row[2] += wx * q[2];
        }
        acc[0] += wy * row[0]; acc[1] += wy * row[1]; acc[2] += wy * row[2];
    }
    const long long den = (long long)W * H;
    uint8_t* o = out + gid * 3;
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((2 * acc[c] + den) / (2 * den));
}

// u8 [B,nh,nw,3] RGB -> f32 NHWC [B,640,640,3]: pad 114, channels REVERSED (the reference feeds RGB arrays to a BGR
// pipeline whose preprocessor then swaps them, interface_heuristic.py:137), / 255
__global__ __launch_bounds__(256) void letterbox_pack_kernel(const uint8_t* __restrict__ in, int nh, int nw, int top, int left,
                                                             float* __restrict__ out, size_t total) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int x = (int)(gid % YOLO_IMG), y = (int)((gid / YOLO_IMG) % YOLO_IMG);
    const size_t img = gid / ((size_t)YOLO_IMG * YOLO_IMG);
    int r = 114, g = 114, b = 114;
    const int sy = y - top, sx = x - left;
    if (sy >= 0 && sy < nh && sx >= 0 && sx < nw) {
        const uint8_t* q = in + ((img * nh + sy) * nw + sx) * 3;
        r = q[0]; g = q[1]; b = q[2];
    }
    float* o = out + gid * 3;
    o[0] = (float)b / 255.0f; o[1] = (float)g / 255.0f; o[2] = (float)r / 255.0f;
}

// ------------------------------------------------------------------ head
struct DecodeArgs {
    const float* E; const float* R;                           // [B*HW, 512], [B*HW, 64]
    int HW, Wl, stride, anchor0, n_anchor;                    // level geometry; anchor index base inside the image
    float logit_scale, bias;
    const float* textn;                                       // [sets][32][512] F.normalize'd text
    const int* setQ; const int* image_set;
    float pad_left, pad_top, sf_w, sf_h;
    float cand_thr;
    float* boxes;                                             // [B, n_anchor, 4] un-letterboxed, unclamped
    unsigned long long* cand; int cand_cap; int* cand_count;  // per image
    float* dense_scores; int dense_q;                         // optional [B, n_anchor, dense_q]
};

// 16 anchors of ONE image per workgroup (4 per wave, one after the other): DFL expectation + decode + un-letterbox;
// scores against every query of the image's set; (score, anchor, class) pairs above the candidate threshold are
// collected in LDS and appended to the image's list with ONE global atomic per workgroup (every anchor appending on its
// own serialised ~8 x 10^5 atomics on a few counters: 9 ms of a 100 ms forward)
constexpr int HD_APB = 16;                                          // anchors per block
__global__ __launch_bounds__(256) void head_decode_kernel(DecodeArgs a, int rows) {
    __shared__ unsigned long long s_cand[HD_APB * YOLO_MAX_Q];
    __shared__ int s_n, s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int row0 = blockIdx.x * HD_APB;
    const int img = row0 / a.HW;                                     // HW % 16 == 0: a block never straddles two images
    const int set = a.image_set ? a.image_set[img] : 0;
    const int Q = a.setQ[set];
    for (int ai = 0; ai < HD_APB / 4; ++ai) {
        const int row = row0 + wave * (HD_APB / 4) + ai;
        if (row >= rows) break;
        const int p = row - img * a.HW;
        const int anchor = a.anchor0 + p;
        // DFL: lane = side * 16 + bin
        const float r = a.R[(size_t)row * 64 + lane];
        float mx = r;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        const float e = expf(r - mx);
        float se = e, sw = e * (float)(lane & 15);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { se += __shfl_xor(se, o); sw += __shfl_xor(sw, o); }
        const float dist = (sw / se) * (float)a.stride;
        const float d0 = __shfl(dist, 0), d1 = __shfl(dist, 16), d2 = __shfl(dist, 32), d3 = __shfl(dist, 48);
        const float px = ((float)(p % a.Wl) + 0.5f) * (float)a.stride, py = ((float)(p / a.Wl) + 0.5f) * (float)a.stride;
        if (lane == 0) {
            f32x4 bx;
            bx[0] = (px - d0 - a.pad_left) / a.sf_w; bx[1] = (py - d1 - a.pad_top) / a.sf_h;
            bx[2] = (px + d2 - a.pad_left) / a.sf_w; bx[3] = (py + d3 - a.pad_top) / a.sf_h;
            *reinterpret_cast<f32x4*>(a.boxes + ((size_t)img * a.n_anchor + anchor) * 4) = bx;
        }
        // classification: <E[row], textn[k]> * exp(logit_scale) + bias -> sigmoid
        const float* er = a.E + (size_t)row * YOLO_TEXT;
        float ev[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ev[i] = er[i * 64 + lane];
        for (int k = 0; k < Q; ++k) {
            const float* t = a.textn + ((size_t)set * YOLO_MAX_Q + k) * YOLO_TEXT;
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) d = fmaf(ev[i], t[i * 64 + lane], d);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
            if (lane == 0) {
                const float logit = d * a.logit_scale + a.bias;
                const float sc = 1.0f / (1.0f + expf(-logit));
                if (a.dense_scores) a.dense_scores[((size_t)img * a.n_anchor + anchor) * a.dense_q + k] = sc;
                if (sc > a.cand_thr) {
                    const unsigned id = (unsigned)anchor * YOLO_MAX_Q + (unsigned)k;
                    s_cand[atomicAdd(&s_n, 1)] = ((unsigned long long)__float_as_uint(sc) << 32) | (0xFFFFFFFFu - id);
                }
            }
        }
    }
    __syncthreads();
    const int n = s_n;
    if (threadIdx.x == 0 && n > 0) s_base = atomicAdd(&a.cand_count[img], n);
    __syncthreads();
    if (n > 0) {
        const int base = s_base;
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            if (base + i < a.cand_cap) a.cand[(size_t)img * a.cand_cap + base + i] = s_cand[i];
    }
}

// One workgroup per image.  mmyolo's order of business -- every (anchor, class) pair with score > 0.001 is a candidate,
// sorted by descending score, the first nms_pre = 30000 kept, class-aware NMS with mmcv's coordinate-offset trick (the offset
// is the largest coordinate among ALL kept candidates + 1), max_per_img = 300, clamp -- followed by the reference wrapper
// (score > 0.12, top max_dets).  Only candidates above the wrapper threshold can ever be output, and a candidate can only
// be suppressed by a higher-scoring survivor, so the full sort is not needed:
//   1. if there are more than nms_pre candidates, an 8-pass radix select finds the nms_pre-th largest key (keys are unique);
//   2. the largest coordinate is reduced over the candidates at or above that key;
//   3. the candidates above the wrapper threshold (and the cut) are compacted into LDS (up to 16384 keys = 128 KB) and
//      bitonic-sorted there -- a global-memory sort of all 8400 x Q keys took 3.6 ms per batch; beyond 16384 the kernel
//      falls back to sorting the whole list in global memory;
//   4. greedy NMS by ONE wavefront (survivors in LDS, lanes test them in parallel, __ballot decides), cut, clamp, top-k.
constexpr int NMS_LDS_KEYS = 16384;
__global__ __launch_bounds__(1024) void sort_nms_kernel(unsigned long long* __restrict__ cand_all, int cand_cap, const int* __restrict__ cand_count,
                                                        const float* __restrict__ boxes_all, int n_anchor, float img_w, float img_h,
                                                        float wrapper_thr, int max_dets, float* __restrict__ det_scores,
                                                        int* __restrict__ det_labels, float* __restrict__ det_boxes, int* __restrict__ n_det) {
    extern __shared__ unsigned long long s_keys[];             // NMS_LDS_KEYS
    __shared__ float k_box[YOLO_MAX_PER_IMG][4];               // offset boxes of the survivors
    __shared__ float k_area[YOLO_MAX_PER_IMG];
    __shared__ unsigned k_id[YOLO_MAX_PER_IMG];
    __shared__ float k_score[YOLO_MAX_PER_IMG];
    __shared__ float s_red[1024 / 64];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned long long s_pref[2];
    __shared__ int s_kept, s_m;
    const int img = blockIdx.x, t = threadIdx.x;
    unsigned long long* cand = cand_all + (size_t)img * cand_cap;
    const float* boxes = boxes_all + (size_t)img * n_anchor * 4;
    int n = cand_count[img];
    n = n < cand_cap ? n : cand_cap;
    // ---- 1. the nms_pre cut: key of rank nms_pre - 1 in descending order (0 = no cut)
    unsigned long long kth = 0ull;
    if (n > YOLO_NMS_PRE) {
        unsigned long long prefix = 0ull, mask = 0ull;
        int kk = YOLO_NMS_PRE - 1;                             // rank from the top
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int i = t; i < 256; i += 1024) s_hist[i] = 0u;
            __syncthreads();
            for (int i = t; i < n; i += 1024) {
                const unsigned long long c = cand[i];
                if ((c & mask) == prefix) atomicAdd(&s_hist[(c >> shift) & 0xFF], 1u);
            }
            __syncthreads();
            if (t == 0) {
                int acc = 0, d = 255;
                for (; d >= 0; --d) { if (acc + (int)s_hist[d] > kk) break; acc += s_hist[d]; }
                s_pref[0] = prefix | ((unsigned long long)d << shift);
                s_pref[1] = (unsigned long long)(kk - acc);
            }
            __syncthreads();
            prefix = s_pref[0];
            kk = (int)s_pref[1];
            mask |= 0xFFULL << shift;
            __syncthreads();
        }
        kth = prefix;
    }
    // ---- 2. mmcv batched_nms: boxes + label * (max coordinate + 1), in float32; 3. compaction into LDS
    if (t == 0) { s_kept = 0; s_m = 0; }
    __syncthreads();
    float mx = -INFINITY;
    for (int i = t; i < n; i += 1024) {
        const unsigned long long c = cand[i];
        if (c < kth) continue;
        const unsigned id = 0xFFFFFFFFu - (unsigned)(c & 0xFFFFFFFFu);
        const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + (size_t)(id / YOLO_MAX_Q) * 4);
        mx = fmaxf(fmaxf(fmaxf(mx, b[0]), fmaxf(b[1], b[2])), b[3]);
        if (__uint_as_float((unsigned)(c >> 32)) > wrapper_thr) {
            const int slot = atomicAdd(&s_m, 1);
            if (slot < NMS_LDS_KEYS) s_keys[slot] = c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) s_red[t >> 6] = mx;
    __syncthreads();
    float maxc = s_red[0];
    for (int i = 1; i < 1024 / 64; ++i) maxc = fmaxf(maxc, s_red[i]);
    const float off_unit = maxc + 1.0f;
    int m = s_m;
    unsigned long long* keys = s_keys;
    if (m > NMS_LDS_KEYS) {                                    // rare: sort the whole list in global memory instead
        keys = cand;
        int n2 = 1;
        while (n2 < n) n2 <<= 1;
        for (int i = n + t; i < n2; i += 1024) cand[i] = 0ull;
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = t; i < n2; i += 1024) {
                    const int l = i ^ j;
                    if (l > i) {
                        const unsigned long long x = cand[i], y = cand[l];
                        if (((i & k) == 0) ? x < y : x > y) { cand[i] = y; cand[l] = x; }
                    }
                }
                __syncthreads();
            }
        m = n < YOLO_NMS_PRE ? n : YOLO_NMS_PRE;
    } else {
        int n2 = 1;
        while (n2 < m) n2 <<= 1;
        for (int i = m + t; i < n2; i += 1024) s_keys[i] = 0ull;          // padding sorts last (score bits 0)
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1)                                   // bitonic sort in LDS, descending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = t; i < n2; i += 1024) {
                    const int l = i ^ j;
                    if (l > i) {
                        const unsigned long long x = s_keys[i], y = s_keys[l];
                        if (((i & k) == 0) ? x < y : x > y) { s_keys[i] = y; s_keys[l] = x; }
                    }
                }
                __syncthreads();
            }
    }
    if (t < 64) {                                              // ---- 4. ONE wave: lock-step, no barriers
        // candidates are taken 64 at a time: every lane fetches one candidate's key and box (64 independent loads in flight),
        // then the wave walks them in order with v_readlane broadcasts -- a dependent global load per candidate cost ~1.5 us
        int kept = 0;
        bool done = false;
        for (int base = 0; base < m && kept < YOLO_MAX_PER_IMG && !done; base += 64) {
            const int mine = base + t;
            const unsigned long long cm = mine < m ? keys[mine] : 0ull;
            const unsigned idm = 0xFFFFFFFFu - (unsigned)(cm & 0xFFFFFFFFu);
            f32x4 bm = {0.f, 0.f, 0.f, 0.f};
            if (mine < m) bm = *reinterpret_cast<const f32x4*>(boxes + (size_t)(idm / YOLO_MAX_Q) * 4);
            const int scm = (int)(unsigned)(cm >> 32);
            const int cnt = (m - base) < 64 ? (m - base) : 64;
            for (int j = 0; j < cnt && kept < YOLO_MAX_PER_IMG; ++j) {
                const float sc = __int_as_float(__builtin_amdgcn_readlane(scm, j));
                // the wrapper drops survivors at or below its threshold, and they cannot suppress anything before them
                if (!(sc > wrapper_thr)) { done = true; break; }
                const unsigned id = (unsigned)__builtin_amdgcn_readlane((int)idm, j);
                const int label = (int)(id % YOLO_MAX_Q);
                const float o = (float)label * off_unit;
                const float x0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bm[0]), j)) + o;
                const float y0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bm[1]), j)) + o;
                const float x1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bm[2]), j)) + o;
                const float y1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bm[3]), j)) + o;
                const float area = (x1 - x0) * (y1 - y0);
                bool sup = false;
                for (int q = t; q < kept; q += 64) {
                    const float iw = fmaxf(fminf(x1, k_box[q][2]) - fmaxf(x0, k_box[q][0]), 0.f);
                    const float ih = fmaxf(fminf(y1, k_box[q][3]) - fmaxf(y0, k_box[q][1]), 0.f);
                    const float inter = iw * ih;
                    sup |= inter / (area + k_area[q] - inter) > YOLO_IOU_THR;
                }
                if (__ballot(sup) == 0ull) {
                    if (t == 0) {
                        k_box[kept][0] = x0; k_box[kept][1] = y0; k_box[kept][2] = x1; k_box[kept][3] = y1;
                        k_area[kept] = area; k_id[kept] = id; k_score[kept] = sc;
                    }
                    // lane 0's survivor must be visible to every lane's LDS reads of the next candidate: a wavefront-scope
                    // release fence + wave barrier pins the order for the compiler too (no load may be hoisted above it)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    ++kept;
                }
            }
        }
        if (t == 0) s_kept = kept;
    }
    __syncthreads();
    // survivors are in descending score order and all above the wrapper threshold: the output is a prefix
    const int kept = s_kept;
    const int nd = kept < max_dets ? kept : max_dets;
    if (t < max_dets) {
        float* b = det_boxes + ((size_t)img * max_dets + t) * 4;
        if (t < nd) {
            const unsigned id = k_id[t];
            const f32x4 rb = *reinterpret_cast<const f32x4*>(boxes + (size_t)(id / YOLO_MAX_Q) * 4);
            b[0] = fminf(fmaxf(rb[0], 0.f), img_w); b[1] = fminf(fmaxf(rb[1], 0.f), img_h);
            b[2] = fminf(fmaxf(rb[2], 0.f), img_w); b[3] = fminf(fmaxf(rb[3], 0.f), img_h);
            det_scores[(size_t)img * max_dets + t] = k_score[t];
            det_labels[(size_t)img * max_dets + t] = (int)(id % YOLO_MAX_Q);
        } else {
            b[0] = b[1] = b[2] = b[3] = 0.f;
            det_scores[(size_t)img * max_dets + t] = 0.f;
            det_labels[(size_t)img * max_dets + t] = -1;
        }
    }
    if (t == 0) n_det[img] = nd;
}

// imageGridScoreFunction's loop (interface_searcher.py:129-150) over the <= max_dets detections of each image
__global__ __launch_bounds__(64) void det_cells_kernel(const float* __restrict__ det_scores, const int* __restrict__ det_labels,
                                                       const float* __restrict__ det_boxes, const int* __restrict__ n_det, int max_dets,
                                                       const double* __restrict__ qweight_all, const int* __restrict__ image_set,
                                                       int img_w, int img_h, int grows, int gcols, double* __restrict__ cell_conf,
                                                       uint32_t* __restrict__ cell_mask) {
    extern __shared__ unsigned long long sm[];
    const int ncell = grows * gcols, b = blockIdx.x;
    unsigned long long* cbits = sm;
    uint32_t* cmask = reinterpret_cast<uint32_t*>(sm + ncell);
    const double* qweight = qweight_all + (image_set ? image_set[b] : 0) * YOLO_MAX_Q;
    for (int i = threadIdx.x; i < ncell; i += blockDim.x) { cbits[i] = 0ull; cmask[i] = 0u; }
    __syncthreads();
    const double cw = (double)img_w / (double)gcols, ch = (double)img_h / (double)grows;
    for (int d = threadIdx.x; d < n_det[b]; d += blockDim.x) {
        const size_t r = (size_t)b * max_dets + d;
        const int lab = det_labels[r];
        const double conf = (double)det_scores[r] * qweight[lab];
        const float* bb = det_boxes + r * 4;
        const float cx = (bb[0] + bb[2]) * 0.5f, cy = (bb[1] + bb[3]) * 0.5f;
        int gx = (int)np_floor_divide((double)cx, cw), gy = (int)np_floor_divide((double)cy, ch);
        gx = gx < gcols - 1 ? gx : gcols - 1; gy = gy < grows - 1 ? gy : grows - 1;
        gx = gx < 0 ? 0 : gx; gy = gy < 0 ? 0 : gy;
        atomicMax(&cbits[gy * gcols + gx], (unsigned long long)__double_as_longlong(conf));
        atomicOr(&cmask[gy * gcols + gx], 1u << lab);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ncell; i += blockDim.x) {
        cell_conf[(size_t)b * ncell + i] = __longlong_as_double((long long)cbits[i]);
        cell_mask[(size_t)b * ncell + i] = cmask[i];
    }
}

}  // namespace tstar

using namespace tstar;

struct tstar_yolo {
    YoloProgram prog;                                         // the checked program (yolo_program.h)
    int input_buf = 0, max_batch = 0;
    DeviceBuf<float> d_blob;
    DeviceBuf<float> d_blob_t;                                // conv matrices transposed to [K][cout], each at a 64-byte aligned offset
    std::vector<size_t> wt_off;                               // ... wt_off[op] (floats), one entry per op
    std::vector<DeviceBuf<float>> act;                        // activation buffers [max_batch, H, W, C] + the zero quad padded conv taps read
    std::vector<float*> bufs;                                 // ... their pointers, as the launches take them
    std::vector<DeviceBuf<float>> d_guide;                    // per attention layer [sets][32][embed]
    int Q[YOLO_SETS] = {0};
    DeviceBuf<float> d_text, d_textn;                         // [sets][32][512] raw / normalised
    DeviceBuf<double> d_qweight;
    DeviceBuf<int> d_setQ, d_iota, d_cand_count;
    DeviceBuf<int> image_set;                                 // the image -> query set array of a call
    DeviceBuf<uint8_t> tmp_u8;                                // the chunk's images at the letterbox's inner size
    DeviceBuf<float> d_boxes;                                 // [max_batch, n_anchor, 4]
    DeviceBuf<unsigned long long> cand;                       // [max_batch, cand_cap()]
    int cand_cap() const { return (int)(cand.cap / max_batch); }
};

static size_t pow2_at_least(size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; }

// create, step 3: the blob, and the transposed copies for the scalar-weight kernel (a weight row of 16 channels is one 64-byte
// scalar-cache line).  Null stream; returns after the device has finished.
static int yolo_upload(tstar_yolo* h, const float* h_blob, size_t n_blob) {
    RC(h->d_blob.reserve(n_blob, 0));
    TSTAR_HIP_CHECK(hipMemcpy(h->d_blob.p, h_blob, n_blob * sizeof(float), hipMemcpyHostToDevice));
    size_t n_t = 0;
    for (const YoloOp& op : h->prog.ops) {
        h->wt_off.push_back(n_t);
        if (op.kind == OP_CONV) n_t += round_up((size_t)op.conv.cout * op.conv.ks * op.conv.ks * op.conv.cin, 16);
    }
    RC(h->d_blob_t.reserve(n_t + 16, 0));
    for (size_t i = 0; i < h->prog.ops.size(); ++i) {
        if (h->prog.ops[i].kind != OP_CONV) continue;
        const YoloConvOp& c = h->prog.ops[i].conv;
        RC(launch_transpose_w(h->d_blob.p + c.w_off, h->d_blob_t.p + h->wt_off[i], c.cout, c.ks * c.ks * c.cin, 0));
    }
    TSTAR_HIP_CHECK(hipDeviceSynchronize());
    return TSTAR_OK;
}

// create, step 4: everything whose size the program and max_batch fix
static int yolo_allocate(tstar_yolo* h) {
    const int max_batch = h->max_batch;
    h->d_guide.resize(h->prog.guides.size());
    for (size_t i = 0; i < h->d_guide.size(); ++i) RC(h->d_guide[i].reserve((size_t)YOLO_SETS * YOLO_MAX_Q * h->prog.guides[i].embed, 0));
    h->act.resize(h->prog.bufs.size());
    for (size_t i = 0; i < h->act.size(); ++i) {
        const YoloBuf& b = h->prog.bufs[i];
        const size_t n = (size_t)max_batch * b.H * b.W * b.C;
        RC(h->act[i].reserve(n + 4, 0));                            // + the zero quad padded conv taps read (conv_sw_kernel)
        TSTAR_HIP_CHECK(hipMemset(h->act[i].p + n, 0, 4 * sizeof(float)));
        h->bufs.push_back(h->act[i].p);
    }
    const size_t nsq = (size_t)YOLO_SETS * YOLO_MAX_Q;
    RC(h->d_text.reserve(nsq * YOLO_TEXT, 0));
    RC(h->d_textn.reserve(nsq * YOLO_TEXT, 0));
    RC(h->d_qweight.reserve(nsq, 0));
    TSTAR_HIP_CHECK(hipMemset(h->d_qweight.p, 0, nsq * sizeof(double)));
    RC(h->d_setQ.reserve(YOLO_SETS, 0));
    TSTAR_HIP_CHECK(hipMemset(h->d_setQ.p, 0, YOLO_SETS * sizeof(int)));
    RC(h->d_iota.reserve(max_batch, 0));
    RC(h->d_cand_count.reserve(max_batch, 0));
    RC(h->d_boxes.reserve((size_t)max_batch * h->prog.n_anchor * 4, 0));
    std::vector<int> io(max_batch);
    for (int i = 0; i < max_batch; ++i) io[i] = i;
    TSTAR_HIP_CHECK(hipMemcpy(h->d_iota.p, io.data(), max_batch * sizeof(int), hipMemcpyHostToDevice));
    return TSTAR_OK;
}

extern "C" {

int tstar_yolo_destroy(tstar_yolo* h) {
    if (!h) return TSTAR_OK;
    delete h;                                                 // every device array is a DeviceBuf member: its destructor frees it
    return TSTAR_OK;
}

int tstar_yolo_check_program(const float* h_blob, size_t n_blob, const int32_t* h_ops, int n_ops, int op_words, const int32_t* h_bufs, int n_bufs,
                             const int32_t* h_guides, int n_guides, const int32_t* h_levels, int n_levels, int input_buf, int max_batch) {
    YoloProgram prog;
    const std::string err = decode_program(h_blob, n_blob, h_ops, n_ops, op_words, h_bufs, n_bufs, h_guides, n_guides, h_levels, n_levels, input_buf,
                                           max_batch, &prog);
    if (!err.empty()) { set_error(err); return TSTAR_ERR_ARG; }
    return TSTAR_OK;
}

int tstar_yolo_create(tstar_yolo** out, const float* h_blob, size_t n_blob, const int32_t* h_ops, int n_ops, int op_words,
                      const int32_t* h_bufs, int n_bufs, const int32_t* h_guides, int n_guides, const int32_t* h_levels,
                      int n_levels, int input_buf, int max_batch) {
    TSTAR_REQUIRE(out, "tstar_yolo_create: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("tstar_yolo_create: no HIP device visible (this library has no CPU path)");
        return TSTAR_ERR_HIP;
    }
    tstar_yolo* h = new tstar_yolo();
    const std::string err = decode_program(h_blob, n_blob, h_ops, n_ops, op_words, h_bufs, n_bufs, h_guides, n_guides, h_levels, n_levels, input_buf,
                                           max_batch, &h->prog);
    if (!err.empty()) { delete h; set_error(err); return TSTAR_ERR_ARG; }
    h->max_batch = max_batch; h->input_buf = input_buf;
    int rc = yolo_upload(h, h_blob, n_blob);
    if (rc == TSTAR_OK) rc = yolo_allocate(h);
    if (rc != TSTAR_OK) {
        set_error(std::string("tstar_yolo_create: allocation failed: ") + tstar_last_error());
        tstar_yolo_destroy(h);
        return rc;
    }
    *out = h;
    return TSTAR_OK;
}

int tstar_yolo_set_text_feats(tstar_yolo* h, int query_set, const float* h_text, const double* h_class_weight, int Q, void* stream) {
    TSTAR_REQUIRE(h && h_text && h_class_weight, "tstar_yolo_set_text_feats: null argument");
    TSTAR_CHECK_SET(query_set, "tstar_yolo_set_text_feats");
    TSTAR_REQUIRE(Q >= 1 && Q <= YOLO_MAX_Q, "tstar_yolo_set_text_feats: Q must be in 1..32");
    hipStream_t s = (hipStream_t)stream;
    const size_t qo = (size_t)query_set * YOLO_MAX_Q;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_text.p + qo * YOLO_TEXT, h_text, (size_t)Q * YOLO_TEXT * sizeof(float), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_qweight.p + qo, h_class_weight, Q * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(text_normalize_kernel, dim3(Q), dim3(64), 0, s, h->d_text.p + qo * YOLO_TEXT, h->d_textn.p + qo * YOLO_TEXT);
    for (size_t i = 0; i < h->prog.guides.size(); ++i) {
        const YoloGuide& g = h->prog.guides[i];
        hipLaunchKernelGGL(guide_fc_kernel, dim3(cdiv(Q * g.embed, 256)), dim3(256), 0, s, h->d_text.p + qo * YOLO_TEXT, Q,
                           h->d_blob.p + g.w_off, h->d_blob.p + g.b_off, g.embed, h->d_guide[i].p + qo * g.embed);
    }
    TSTAR_HIP_CHECK(hipGetLastError());
    h->Q[query_set] = Q;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_setQ.p, h->Q, sizeof(h->Q), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

int tstar_yolo_set_class_weights(tstar_yolo* h, int query_set, const double* h_class_weight, int Q, void* stream) {
    TSTAR_REQUIRE(h && h_class_weight, "tstar_yolo_set_class_weights: null argument");
    TSTAR_CHECK_SET(query_set, "tstar_yolo_set_class_weights");
    TSTAR_REQUIRE(Q == h->Q[query_set] && Q >= 1, "tstar_yolo_set_class_weights: Q does not match the installed text features");
    hipStream_t s = (hipStream_t)stream;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_qweight.p + (size_t)query_set * YOLO_MAX_Q, h_class_weight, Q * sizeof(double), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ the program interpreter
static void launch_pool5(tstar_yolo* h, const YoloPoolOp& q, int B, hipStream_t s) {
    const YoloBuf& b = h->prog.bufs[q.buf];
    const size_t total = (size_t)B * b.H * b.W * (q.C / 4);
    hipLaunchKernelGGL(pool5_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, h->bufs[q.buf], b.C, q.src_off, q.dst_off, q.C, b.H, b.W,
                       h->bufs[q.buf], total);
}

static void launch_upcopy(tstar_yolo* h, const YoloUpcopyOp& u, int B, hipStream_t s) {
    const YoloBuf& src = h->prog.bufs[u.src];
    const size_t total = (size_t)B * src.H * u.factor * src.W * u.factor * (u.C / 4);
    hipLaunchKernelGGL(upcopy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, h->bufs[u.src], src.C, u.src_off, u.C, src.H, src.W,
                       u.factor, h->bufs[u.dst], h->prog.bufs[u.dst].C, u.dst_off, total);
}

static int launch_attn(tstar_yolo* h, const YoloAttnOp& a, int B, const int* d_image_set, hipStream_t s) {
    const YoloGuide& g = h->prog.guides[a.guide];
    const YoloBuf& src = h->prog.bufs[a.src];
    const int HW = src.H * src.W;
    const int bx = cdiv(HW * g.heads, 256);               // one (pixel, head) per thread (the cap of 64 blocks per image left the 80x80 maps at a quarter of the threads they need)
    const size_t lds = (size_t)YOLO_MAX_Q * g.embed * sizeof(float);
    RC(ensure_dyn_lds(reinterpret_cast<const void*>(attn_kernel), (int)YOLO_GUIDE_LDS_BYTES));
    hipLaunchKernelGGL(attn_kernel, dim3(bx, B), dim3(256), lds, s, h->bufs[a.src], src.C, a.src_off, g.embed, g.heads, HW, h->d_guide[a.guide].p,
                       h->d_setQ.p, d_image_set, h->d_blob.p + g.bias_off, h->bufs[a.dst], B * HW);
    return TSTAR_OK;
}

// h_forms (optional, one int per op): the kernel form every conv op launched (TSTAR_YOLO_FORM_*), -1 for the other ops
static int run_program(tstar_yolo* h, int B, const int* d_image_set, hipStream_t s, int32_t* h_forms = nullptr) {
    for (size_t oi = 0; oi < h->prog.ops.size(); ++oi) {
        const YoloOp& op = h->prog.ops[oi];
        if (h_forms) h_forms[oi] = -1;
        switch (op.kind) {
        case OP_CONV: {
            const YoloConvOp& c = op.conv;
            ConvArgs a = conv_args(h->prog, c, B, h->max_batch);
            a.src = h->bufs[c.src]; a.dst = h->bufs[c.dst];
            a.w = h->d_blob.p + c.w_off; a.wt = h->d_blob_t.p + h->wt_off[oi]; a.bias = c.b_off >= 0 ? h->d_blob.p + c.b_off : nullptr;
            if (c.mode != MODE_PLAIN) a.aux = h->bufs[c.aux];
            int form = -1;
            RC(launch_conv(a, s, &form));
            if (h_forms) h_forms[oi] = form;
            break;
        }
        case OP_POOL5: launch_pool5(h, op.pool, B, s); break;
        case OP_UPCOPY: launch_upcopy(h, op.up, B, s); break;
        default: RC(launch_attn(h, op.attn, B, d_image_set, s)); break;
        }
        TSTAR_HIP_CHECK(hipGetLastError());
    }
    return TSTAR_OK;
}

// mmyolo test pipeline geometry: YOLOv5KeepRatioResize(640) then LetterResize(640, allow_scale_up=False, pad 114)
struct YoloGeom { double ratio, sfw, sfh; int rw, rh, top, left; };

static const char* const NO_TEXT_FEATS = "no text features installed in the requested query set (call tstar_yolo_set_text_feats first)";

// What tstar_yolo_detect and tstar_yolo_postprocess share before the first launch: argument checks, the per-image query
// sets (uploaded to image_set), the candidate lists' capacity and the letterbox geometry of an H x W image.
static int yolo_prepare(tstar_yolo* h, const char* fn, int B, int H, int W, int grid_rows, int grid_cols, const int32_t* h_image_query_set,
                        int max_dets, const double* d_cell_conf, const uint32_t* d_cell_mask, const float* d_dense_scores, hipStream_t s,
                        int* q_uniform_out, YoloGeom* g) {
    const std::string f(fn);
    TSTAR_REQUIRE(B >= 1 && H >= 2 && W >= 2, f + ": empty batch or image");
    TSTAR_REQUIRE(max_dets >= 1 && max_dets <= YOLO_MAX_PER_IMG, f + ": max_dets must be in 1..300");
    TSTAR_REQUIRE(!d_cell_conf == !d_cell_mask, f + ": cell_conf and cell_mask go together");
    TSTAR_REQUIRE(!d_cell_conf || (grid_rows >= 1 && grid_cols >= 1 && grid_rows * grid_cols <= 4096), f + ": grid must have 1..4096 cells");
    int q_uniform = -1, q_max = 0;
    RC(check_query_sets(f, NO_TEXT_FEATS, h->Q, h_image_query_set, B, h->image_set, s, &q_uniform, &q_max));
    TSTAR_REQUIRE(!d_dense_scores || q_uniform > 0, f + ": dense scores need the same query count for every image");
    // candidate lists: every (anchor, class) pair can qualify
    RC(h->cand.reserve((size_t)h->max_batch * pow2_at_least((size_t)h->prog.n_anchor * q_max), s));
    g->ratio = fmin(640.0 / (H > W ? H : W), 640.0 / (H < W ? H : W));
    g->rw = g->ratio != 1.0 ? (int)(W * g->ratio) : W; g->rh = g->ratio != 1.0 ? (int)(H * g->ratio) : H;
    TSTAR_REQUIRE(g->rw >= 1 && g->rh >= 1 && g->rw <= YOLO_IMG && g->rh <= YOLO_IMG, f + ": image shape outside the letterbox geometry");
    g->sfw = (double)g->rw / W; g->sfh = (double)g->rh / H;
    // LetterResize: top = int(round(padding_h // 2 - 0.1)) = padding_h // 2 (the -0.1 only breaks the .5 tie of a float half)
    g->top = (YOLO_IMG - g->rh) / 2; g->left = (YOLO_IMG - g->rw) / 2;
    *q_uniform_out = q_uniform;
    return TSTAR_OK;
}

// The post-process of images b0 .. b0 + Bc - 1 (one chunk, Bc <= max_batch) from the head tensors of the chunk: per level
// E[l] [Bc * size_l^2, 512] and R[l] [Bc * size_l^2, 64].  The output pointers are those of the whole batch.
static int yolo_tail(tstar_yolo* h, const float* const* E, const float* const* R, int b0, int Bc, int H, int W, const YoloGeom& g,
                     const int* d_sets, int q_uniform, int grid_rows, int grid_cols, float score_threshold, int max_dets,
                     float* d_det_scores, int32_t* d_det_labels, float* d_det_boxes, int32_t* d_n_det, double* d_cell_conf,
                     uint32_t* d_cell_mask, float* d_dense_scores, float* d_dense_boxes, hipStream_t s) {
    // candidates exactly as mmyolo's predict_by_feat forms them (multi_label, score > score_thr = 0.001): the class-aware
    // NMS offsets depend on the largest coordinate among ALL of them, so the wrapper's 0.12 is not applied early
    const float cand_thr = YOLO_SCORE_THR;
    TSTAR_HIP_CHECK(hipMemsetAsync(h->d_cand_count.p, 0, Bc * sizeof(int), s));
    int anchor0 = 0;
    for (size_t li = 0; li < h->prog.levels.size(); ++li) {
        const YoloLevel& l = h->prog.levels[li];
        DecodeArgs a{};
        a.E = E[li]; a.R = R[li]; a.HW = l.size * l.size; a.Wl = l.size; a.stride = l.stride;
        a.anchor0 = anchor0; a.n_anchor = h->prog.n_anchor; a.logit_scale = l.logit_scale; a.bias = l.bias;
        a.textn = h->d_textn.p; a.setQ = h->d_setQ.p; a.image_set = d_sets;
        a.pad_left = (float)g.left; a.pad_top = (float)g.top; a.sf_w = (float)g.sfw; a.sf_h = (float)g.sfh; a.cand_thr = cand_thr;
        a.boxes = h->d_boxes.p; a.cand = h->cand.p; a.cand_cap = h->cand_cap(); a.cand_count = h->d_cand_count.p;
        a.dense_scores = d_dense_scores ? d_dense_scores + (size_t)b0 * h->prog.n_anchor * q_uniform : nullptr; a.dense_q = q_uniform;
        const int rows = Bc * a.HW;
        hipLaunchKernelGGL(head_decode_kernel, dim3(cdiv(rows, HD_APB)), dim3(256), 0, s, a, rows);
        TSTAR_HIP_CHECK(hipGetLastError());
        anchor0 += a.HW;
    }
    RC(ensure_dyn_lds(reinterpret_cast<const void*>(sort_nms_kernel), NMS_LDS_KEYS * 8));
    hipLaunchKernelGGL(sort_nms_kernel, dim3(Bc), dim3(1024), (size_t)NMS_LDS_KEYS * 8, s, h->cand.p, h->cand_cap(), h->d_cand_count.p, h->d_boxes.p, h->prog.n_anchor,
                       (float)W, (float)H, score_threshold, max_dets, d_det_scores + (size_t)b0 * max_dets, d_det_labels + (size_t)b0 * max_dets,
                       d_det_boxes + (size_t)b0 * max_dets * 4, d_n_det + b0);
    TSTAR_HIP_CHECK(hipGetLastError());
    if (d_dense_boxes)
        TSTAR_HIP_CHECK(hipMemcpyAsync(d_dense_boxes + (size_t)b0 * h->prog.n_anchor * 4, h->d_boxes.p, (size_t)Bc * h->prog.n_anchor * 4 * sizeof(float),
                                       hipMemcpyDeviceToDevice, s));
    if (d_cell_conf) {
        const int ncell = grid_rows * grid_cols;
        hipLaunchKernelGGL(det_cells_kernel, dim3(Bc), dim3(64), (size_t)ncell * 12, s, d_det_scores + (size_t)b0 * max_dets,
                           d_det_labels + (size_t)b0 * max_dets, d_det_boxes + (size_t)b0 * max_dets * 4, d_n_det + b0, max_dets,
                           h->d_qweight.p, d_sets, W, H, grid_rows, grid_cols, d_cell_conf + (size_t)b0 * ncell, d_cell_mask + (size_t)b0 * ncell);
        TSTAR_HIP_CHECK(hipGetLastError());
    }
    return TSTAR_OK;
}

extern "C" {

int tstar_yolo_detect(tstar_yolo* h, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                      const int32_t* h_image_query_set, float score_threshold, int max_dets, float* d_det_scores,
                      int32_t* d_det_labels, float* d_det_boxes, int32_t* d_n_det, double* d_cell_conf, uint32_t* d_cell_mask,
                      float* d_dense_scores, float* d_dense_boxes, void* stream) {
    TSTAR_REQUIRE(h && d_images && d_det_scores && d_det_labels && d_det_boxes && d_n_det, "tstar_yolo_detect: null argument");
    hipStream_t s = (hipStream_t)stream;
    int q_uniform = 0;
    YoloGeom g{};
    RC(yolo_prepare(h, "tstar_yolo_detect", B, H, W, grid_rows, grid_cols, h_image_query_set, max_dets, d_cell_conf, d_cell_mask, d_dense_scores, s,
                    &q_uniform, &g));
    const int rw = g.rw, rh = g.rh;
    // chunks of max_batch + one remainder.  Cutting a batch into near-equal chunks instead (156 -> 78 + 78 under a capacity of
    // 96) was measured and is WORSE than 76 + 76 + 4 (bench conv average 98.3 vs 100.5 TFLOP/s): the chunk size is chosen so
    // that the halo layers fill whole rounds of the chip's 768 workgroup slots (20 B workgroups on a 40x40 / 256-channel
    // layer), and two images too many start a third, almost empty round on every such layer.
    for (int b0 = 0; b0 < B; b0 += h->max_batch) {
        const int Bc = (B - b0) < h->max_batch ? (B - b0) : h->max_batch;
        const uint8_t* imgs = d_images + (size_t)b0 * H * W * 3;
        const uint8_t* packed_src = imgs;
        if (rw != W || rh != H) {
            RC(h->tmp_u8.reserve((size_t)Bc * rh * rw * 3, s));
            if (g.ratio < 1.0) {
                const size_t total = (size_t)Bc * rh * rw;
                hipLaunchKernelGGL(area_resize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, imgs, H, W, h->tmp_u8.p, rh, rw, total);
                TSTAR_HIP_CHECK(hipGetLastError());
            } else {
                RC(bilinear_gather_u8(imgs, H, W, h->d_iota.p, Bc, rw, rh, h->tmp_u8.p, 0, s));
            }
            packed_src = h->tmp_u8.p;
        }
        {
            const size_t total = (size_t)Bc * YOLO_IMG * YOLO_IMG;
            hipLaunchKernelGGL(letterbox_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, packed_src, rh, rw, g.top, g.left,
                               h->bufs[h->input_buf], total);
            TSTAR_HIP_CHECK(hipGetLastError());
        }
        const int* d_sets = h_image_query_set ? h->image_set.p + b0 : nullptr;
        RC(run_program(h, Bc, d_sets, s));
        const float* E[8]; const float* R[8];
        for (size_t li = 0; li < h->prog.levels.size(); ++li) { E[li] = h->bufs[h->prog.levels[li].e_buf]; R[li] = h->bufs[h->prog.levels[li].r_buf]; }
        RC(yolo_tail(h, E, R, b0, Bc, H, W, g, d_sets, q_uniform, grid_rows, grid_cols, score_threshold, max_dets, d_det_scores, d_det_labels,
                     d_det_boxes, d_n_det, d_cell_conf, d_cell_mask, d_dense_scores, d_dense_boxes, s));
    }
    return TSTAR_OK;
}

int tstar_yolo_postprocess(tstar_yolo* h, const float* const* d_level_embed, const float* const* d_level_dfl, int n_levels, int B, int H, int W,
                           int grid_rows, int grid_cols, const int32_t* h_image_query_set, float score_threshold, int max_dets,
                           float* d_det_scores, int32_t* d_det_labels, float* d_det_boxes, int32_t* d_n_det, double* d_cell_conf,
                           uint32_t* d_cell_mask, float* d_dense_scores, float* d_dense_boxes, void* stream) {
    TSTAR_REQUIRE(h && d_level_embed && d_level_dfl && d_det_scores && d_det_labels && d_det_boxes && d_n_det, "tstar_yolo_postprocess: null argument");
    TSTAR_REQUIRE(n_levels == (int)h->prog.levels.size(), "tstar_yolo_postprocess: n_levels must equal the number of head levels of the handle");
    for (int l = 0; l < n_levels; ++l) TSTAR_REQUIRE(d_level_embed[l] && d_level_dfl[l], "tstar_yolo_postprocess: null level tensor");
    hipStream_t s = (hipStream_t)stream;
    int q_uniform = 0;
    YoloGeom g{};
    RC(yolo_prepare(h, "tstar_yolo_postprocess", B, H, W, grid_rows, grid_cols, h_image_query_set, max_dets, d_cell_conf, d_cell_mask, d_dense_scores,
                    s, &q_uniform, &g));
    for (int b0 = 0; b0 < B; b0 += h->max_batch) {                   // chunked like detect: d_boxes / cand hold max_batch images
        const int Bc = (B - b0) < h->max_batch ? (B - b0) : h->max_batch;
        const float* E[8]; const float* R[8];
        for (int l = 0; l < n_levels; ++l) {
            const size_t row0 = (size_t)b0 * h->prog.levels[l].size * h->prog.levels[l].size;
            E[l] = d_level_embed[l] + row0 * YOLO_TEXT; R[l] = d_level_dfl[l] + row0 * 4 * YOLO_REG_MAX;
        }
        RC(yolo_tail(h, E, R, b0, Bc, H, W, g, h_image_query_set ? h->image_set.p + b0 : nullptr, q_uniform, grid_rows, grid_cols, score_threshold,
                     max_dets, d_det_scores, d_det_labels, d_det_boxes, d_n_det, d_cell_conf, d_cell_mask, d_dense_scores, d_dense_boxes, s));
    }
    return TSTAR_OK;
}

int tstar_yolo_num_anchors(tstar_yolo* h) { return h ? h->prog.n_anchor : 0; }

int tstar_yolo_buffer_copy(tstar_yolo* h, int buf, float* d_data, int B, int to_buffer, void* stream) {
    TSTAR_REQUIRE(h && d_data, "tstar_yolo_buffer_copy: null argument");
    TSTAR_REQUIRE(buf >= 0 && buf < (int)h->bufs.size(), "tstar_yolo_buffer_copy: no such activation buffer");
    TSTAR_REQUIRE(B >= 1 && B <= h->max_batch, "tstar_yolo_buffer_copy: B must be in 1..max_batch");
    // B <= max_batch images: the zero quad behind the buffer's max_batch images is out of reach
    const YoloBuf& b = h->prog.bufs[buf];
    const size_t bytes = (size_t)B * b.H * b.W * b.C * sizeof(float);
    TSTAR_HIP_CHECK(hipMemcpyAsync(to_buffer ? (void*)h->bufs[buf] : (void*)d_data, to_buffer ? (const void*)d_data : (const void*)h->bufs[buf], bytes,
                                   hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TSTAR_OK;
}

int tstar_yolo_run_ops(tstar_yolo* h, int B, const int32_t* h_image_query_set, int32_t* h_forms, void* stream) {
    TSTAR_REQUIRE(h, "tstar_yolo_run_ops: null argument");
    TSTAR_REQUIRE(B >= 1 && B <= h->max_batch, "tstar_yolo_run_ops: B must be in 1..max_batch");
    hipStream_t s = (hipStream_t)stream;
    if (!h->prog.guides.empty()) {                                            // only the attention ops read the query sets
        int q_uniform = 0;
        RC(check_query_sets("tstar_yolo_run_ops", NO_TEXT_FEATS, h->Q, h_image_query_set, B, h->image_set, s, &q_uniform));
    }
    RC(run_program(h, B, h_image_query_set && !h->prog.guides.empty() ? h->image_set.p : nullptr, s, h_forms));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

}  // extern "C"
