// C ABI of libtstar_hip.so (include/tstar_hip.h): handle management and the
// OWL-ViT (B/32, B/16) forward orchestration over the hand-written gfx950 kernels.
#include "../../include/tstar_hip.h"
#include "common.h"
#include "heads.h"
#include "image_query.h"
#include "ingest.h"
#include "jpeg_entropy_core.h"
#include "jpeg_host.h"
#include "kernels.h"
#include "owl_weights.h"
#include "preprocess_v2.h"
#include <math.h>
#include <map>
#include <mutex>
#include <set>
#include <string.h>
#include <unordered_map>
#include <vector>

namespace tstar {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

int ensure_dyn_lds(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("ensure_dyn_lds: hipGetDevice failed"); return 2; }
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(kernel, dev);
    if (done.count(key)) return 0;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) { set_error(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e)); return 2; }
    done.insert(key);
    return 0;
}

// ---------------------------------------------------------------- small text-tower kernels
// x[q*T + t, :] = tok_emb[ids[q,t], :] + pos_emb[t, :]   (OwlViTTextEmbeddings, modeling_owlvit.py:356-372)
__global__ void embed_tokens_kernel(const int* __restrict__ ids, const float* __restrict__ tok,
                                    const float* __restrict__ pos, float* __restrict__ x, int T, int D) {
    const int r = blockIdx.x;
    const size_t id = (size_t)ids[r];
    const int t = r % T;
    for (int d = threadIdx.x; d < D; d += blockDim.x) x[(size_t)r * D + d] = tok[id * D + d] + pos[(size_t)t * D + d];
}
// y[q, :] = x[q*T + eos[q], :]  (EOS pooling, modeling_owlvit.py:651-658)
__global__ void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ eos, float* __restrict__ y,
                                   int T, int D) {
    const int q = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += blockDim.x) y[(size_t)q * D + d] = x[((size_t)q * T + eos[q]) * D + d];
}
// Wb[i] = bfloat16(W[i]), round to nearest even (exact when W already holds bf16 values);
// optional second term Wlo[i] = bfloat16(W[i] - Wb[i]) (the difference is exact in f32)
__global__ void f32_to_bf16_kernel(const float* __restrict__ W, __bf16* __restrict__ Wb, __bf16* __restrict__ Wlo, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float w = W[i];
        const __bf16 hi = (__bf16)w;
        Wb[i] = hi;
        if (Wlo) Wlo[i] = (__bf16)(w - (float)hi);
    }
}
int convert_f32_to_bf16(const float* W, __bf16* Wb, __bf16* Wlo, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(1024), dim3(256), 0, s, W, Wb, Wlo, n);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}
// out[q,:] = in[q,:] / (||in[q,:]|| + eps); one wave per row, D = 512
__global__ void l2norm_rows_kernel(const float* __restrict__ in, float* __restrict__ out, float eps) {
    const int q = blockIdx.x, lane = threadIdx.x;
    float v[8], s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = in[(size_t)q * 512 + i * 64 + lane]; s += v[i] * v[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float den = sqrtf(s) + eps;
#pragma unroll
    for (int i = 0; i < 8; ++i) out[(size_t)q * 512 + i * 64 + lane] = v[i] / den;
}
}  // namespace tstar

using namespace tstar;

struct tstar_owl {
    float* d_vision = nullptr;
    float* d_text = nullptr;
    VisionW vw{};
    TextW tw{};
    bool has_text = false, has_vision = false;
    OwlGeom geom{};                                                  // patch geometry of the vision tower (B/32 or B/16)
    float* d_lut = nullptr;
    int max_batch = 0;
    int chunk_cap = 0;                                               // images per forward chunk: min(max_batch, owl_chunk_limit(geom))
    size_t mpad = 0;
    // activation workspaces (per chunk of `cap` images).  Lane 0 is the handle's own (max_batch images, allocated at creation; the
    // text tower runs in it).  Lane 1 is a SMALL second one, allocated on first use (tstar_owl_score_lane): a forward that runs in it
    // on another stream shares nothing mutable with a forward in lane 0, so the two may execute concurrently (the searcher's
    // speculative next-grid forward, B = 1, beside the verification batch of the iteration before).
    struct Lane {
        float *x = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr;
        uint8_t* tmp_u8 = nullptr; size_t tmp_u8_bytes = 0;
        int* d_minmax = nullptr; int minmax_cap = 0;                 // OWLv2: per-image clip bounds of the pre-processing (two ints per image)
        int v2_form = -1;                                            // OWLv2: form of the last pre-processing launch (OWLV2_FORM_*)
        int* d_image_set = nullptr; int image_set_cap = 0;
        int cap = 0;                                                 // images per forward chunk
    } lane[TSTAR_OWL_LANES];
    // query sets: TSTAR_OWL_MAX_SETS independent (question) slots, each up to 32 queries; every image of
    // a score call names the slot it is scored against (several (video, question) items batched together)
    int Q[TSTAR_OWL_MAX_SETS] = {0};
    float *q_raw = nullptr, *qn = nullptr;                           // [sets][32][512]
    double* qweight = nullptr;                                       // [sets][32] object2weight per query (float64, as the reference's Python floats)
    uint8_t* qmask = nullptr;                                        // [sets][32]
    int* d_setQ = nullptr;
    int *d_ids = nullptr, *d_eos = nullptr;
    uint8_t* d_kmask = nullptr;
    int seq_cap = TSTAR_OWL_MAX_QUERIES;                             // sequences the three staging buffers above hold
    std::map<std::pair<int, int>, ResampleTable> tabs;   // (in_size, out_size) -> table (out_size: the handle's input width / height)
    std::map<std::pair<int, int>, Owlv2AxisTable> tabs_v2;   // OWLv2: (square side, out_size) -> zoom taps + Gaussian weights of one axis
    std::map<std::pair<int, int>, std::vector<double>> gw_v2;  // OWLv2: Gaussian weights installed by the caller (tstar_owlv2_set_axis_weights)
    // weights_mode 1 / 3 (BASELINE config 5, bf16 weights; two-term / exact three-term activations): bfloat16 copy of every
    // GEMM weight matrix; weights_mode 4 (f32x3): every f32 matrix as three exact bf16 planes in MFMA-fragment order
    int weights_mode = TSTAR_WEIGHTS_F32;
    std::unordered_map<const float*, __bf16*> wb;
    std::unordered_map<const float*, void*> wp;
    std::unordered_map<const float*, void*> wq;          // two-term mode, the N = 768 matrices: the bf16 plane once more in MFMA-fragment order
    const void* w2_of(const float* w) const {
        if (weights_mode != TSTAR_WEIGHTS_BF16) return nullptr;
        auto it = wq.find(w);
        return it == wq.end() ? nullptr : it->second;
    }
    const __bf16* bf16_of(const float* w) const {
        if (weights_mode != TSTAR_WEIGHTS_BF16 && weights_mode != TSTAR_WEIGHTS_BF16_EXACT) return nullptr;
        auto it = wb.find(w);
        return it == wb.end() ? nullptr : it->second;
    }
    const void* packed_of(const float* w) const {
        if (weights_mode != TSTAR_WEIGHTS_F32X3) return nullptr;
        auto it = wp.find(w);
        return it == wp.end() ? nullptr : it->second;
    }
};

static size_t padded(size_t n) { return (n + 63) / 64 * 64; }

template <class MapFn>
static int upload_blob(const float* h_blob, size_t n_expected_check, float** d_out, MapFn&& mapfn) {
    // pass 1: sizes
    size_t packed = 0, pad_total = 0;
    std::vector<std::pair<size_t, size_t>> ents;   // (packed offset, n)
    auto count = [&](size_t n) -> const float* { ents.push_back({packed, n}); packed += n; pad_total += padded(n); return nullptr; };
    mapfn(count);
    if (packed != n_expected_check) {
        set_error("weight blob has " + std::to_string(n_expected_check) + " floats, layout wants " + std::to_string(packed));
        return TSTAR_ERR_ARG;
    }
    float* d = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&d, pad_total * sizeof(float)));
    TSTAR_HIP_CHECK(hipMemset(d, 0, pad_total * sizeof(float)));
    size_t off = 0, i = 0;
    int rc = TSTAR_OK;
    auto place = [&](size_t n) -> const float* {
        const float* p = d + off;
        if (hipMemcpy(d + off, h_blob + ents[i].first, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = TSTAR_ERR_HIP;
        off += padded(n); ++i;
        return p;
    };
    mapfn(place);
    if (rc) { set_error("hipMemcpy of weights failed"); (void)hipFree(d); return rc; }
    *d_out = d;
    return TSTAR_OK;
}

static size_t vision_floats(const OwlGeom& g) {
    size_t n = 0; VisionW w; map_vision(w, g, [&](size_t k) -> const float* { n += k; return nullptr; }); return n;
}

// Images per forward chunk.  A chunk is capped so that it never holds more rows than B/32's largest chunk at 768 x 768 (1024
// images x 577 tokens, the row range every kernel of the forward already runs at): 1024 images at B/32, 256 at B/16 (590080
// rows; hid [Mp, 3072] = 1.81e9 floats), 164 at 3600 patches; 1024 (the max_batch limit) at every input with fewer tokens than
// 577.  Every workspace then stays below 2^31 elements, so the kernels' 32-bit element offsets (the wide GEMM epilogue's
// among them) cannot wrap; checked at creation.
static int owl_chunk_limit(const OwlGeom& g) { const int n = 1024 * V_NTOK / g.ntok; return n < 1024 ? n : 1024; }
// rows of a lane's workspaces: the chunk's tokens, and never fewer than the text tower's largest forward through
// tstar_owl_set_queries (32 sequences of 16 tokens), which runs in lane 0 (a small input at a small max_batch has fewer tokens)
static size_t lane_rows(int cap, const OwlGeom& g) {
    const size_t rows = round_up((size_t)cap * g.ntok, 128), text_rows = (size_t)TSTAR_OWL_MAX_QUERIES * T_LEN;
    return rows > text_rows ? rows : text_rows;
}
static size_t text_floats() {
    size_t n = 0; TextW w; map_text(w, [&](size_t k) -> const float* { n += k; return nullptr; }); return n;
}

static int get_table(tstar_owl* h, int in_size, int out_size, ResampleTable** out, hipStream_t s) {
    const auto key = std::make_pair(in_size, out_size);
    auto it = h->tabs.find(key);
    if (it == h->tabs.end()) {
        ResampleTable t;
        int rc = build_bicubic_table(&t, in_size, out_size, s);
        if (rc) return rc;
        it = h->tabs.emplace(key, t).first;
    }
    *out = &it->second;
    return TSTAR_OK;
}

#define RC(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

static GemmArgs mk_gemm(const tstar_owl* h, const float* A, const float* W, float* C, const float* bias, const float* res,
                        int M, int N, int K, int lda, int ldc, int act) {
    GemmArgs g{};
    g.A = A; g.W = W; g.Wb = h ? h->bf16_of(W) : nullptr; g.Wp = h ? h->packed_of(W) : nullptr; g.Wq = h ? h->w2_of(W) : nullptr; g.C = C; g.bias = bias; g.res = res; g.pos = nullptr;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc; g.act = act; g.patch_np = 0; g.tile_cfg = TILE_AUTO; g.m_split = 0;
    g.a_terms = h && h->weights_mode == TSTAR_WEIGHTS_BF16 ? 2 : 0;      // bf16 weights: two-term activations unless the exact mode is asked for
    return g;
}

// The text tower's GEMMs.  The query embeddings are computed once per query set and enter every score, so the two-term mode runs
// them with the exact three-term activation split on the same bf16 weight plane (what TSTAR_WEIGHTS_BF16_EXACT runs everywhere):
// float32-class embeddings of the rounded checkpoint.  The other modes are unchanged.
static GemmArgs mk_text_gemm(const tstar_owl* h, const float* A, const float* W, float* C, const float* bias, const float* res,
                             int M, int N, int K, int lda, int ldc, int act) {
    GemmArgs g = mk_gemm(h, A, W, C, bias, res, M, N, K, lda, ldc, act);
    if (g.a_terms == 2) { g.a_terms = 0; g.Wq = nullptr; }
    return g;
}

// TSTAR_X3_ATTN_F32=1: the f32x3 mode with the exact-f32 MFMA attention of rounds 1-4 (same-session A/Bs)
static bool x3_attention_f32() {
    static const bool v = getenv("TSTAR_X3_ATTN_F32") != nullptr;
    return v;
}

// CLIP pre-LN encoder stack shared by both towers; x [M,D] updated in place
static int run_encoder(tstar_owl* h, tstar_owl::Lane& L, const LayerW* layers, int nlayers, int B, int T, int D, int FF, int heads,
                       int mode, const uint8_t* key_mask, hipStream_t s) {
    const int M = B * T;
    // mode 1 is the text tower, whose mk_text_gemm keeps every activation bit; mode 0 the vision tower
    const auto mk = mode == 1 ? mk_text_gemm : mk_gemm;
    for (int l = 0; l < nlayers; ++l) {
        const LayerW& w = layers[l];
        RC(layernorm_f32(L.x, L.xn, w.ln1_w, w.ln1_b, M, D, s));
        RC(gemm_f32(mk(h, L.xn, w.qkv_w, L.qkv, w.qkv_b, nullptr, M, 3 * D, D, D, 3 * D, ACT_NONE), s));
        // full attention in the bf16-WEIGHT modes runs on the bf16 matrix pipe too (operands as two bf16 terms); in the f32x3
        // mode with all operand bits (three exact terms, six products: its claim is an error no larger than the f32 path's)
        if (mode == 0 && (h->weights_mode == TSTAR_WEIGHTS_BF16 || h->weights_mode == TSTAR_WEIGHTS_BF16_EXACT)) RC(attention_split(L.qkv, L.att, B, T, heads, s));
        else if (mode == 0 && h->weights_mode == TSTAR_WEIGHTS_F32X3 && !x3_attention_f32()) RC(attention_x3(L.qkv, L.att, B, T, heads, s));
        else RC(attention_f32(L.qkv, L.att, B, T, heads, mode, key_mask, s));
        RC(gemm_f32(mk(h, L.att, w.out_w, L.x, w.out_b, L.x, M, D, D, D, D, ACT_NONE), s));
        RC(layernorm_f32(L.x, L.xn, w.ln2_w, w.ln2_b, M, D, s));
        RC(gemm_f32(mk(h, L.xn, w.fc1_w, L.hid, w.fc1_b, nullptr, M, FF, D, D, FF, ACT_QGELU), s));
        RC(gemm_f32(mk(h, L.hid, w.fc2_w, L.x, w.fc2_b, L.x, M, D, FF, FF, D, ACT_NONE), s));
    }
    return TSTAR_OK;
}

static int get_table_v2(tstar_owl* h, int S, int out_size, Owlv2AxisTable** out) {
    const auto key = std::make_pair(S, out_size);
    auto it = h->tabs_v2.find(key);
    if (it == h->tabs_v2.end()) {
        Owlv2AxisTable t;
        auto gw = h->gw_v2.find(key);
        int rc = build_owlv2_axis_table(&t, S, out_size, gw == h->gw_v2.end() ? nullptr : &gw->second);
        if (rc) return rc;
        it = h->tabs_v2.emplace(key, t).first;
    }
    *out = &it->second;
    return TSTAR_OK;
}

// OWLv2: pad to a square, Gaussian anti-aliasing, linear zoom, clip, normalise, im2col (preprocess_v2.hip); no u8 stage
static int preprocess_chunk_v2(tstar_owl* h, tstar_owl::Lane& L, const uint8_t* d_images, int B, int H, int W, float* out_patches, hipStream_t s) {
    const OwlGeom& G = h->geom;
    const Owlv2Plan p = plan_owlv2_preprocess(H, W, G.in_h, G.in_w);      // refusals before a table is built
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    Owlv2AxisTable *ty, *tx;
    const int S = H > W ? H : W;
    RC(get_table_v2(h, S, G.in_h, &ty));
    RC(get_table_v2(h, S, G.in_w, &tx));
    if (B > L.minmax_cap) {
        TSTAR_HIP_CHECK(hipStreamSynchronize(s));
        if (L.d_minmax) TSTAR_HIP_CHECK(hipFree(L.d_minmax));
        L.d_minmax = nullptr; L.minmax_cap = 0;
        TSTAR_HIP_CHECK(hipMalloc(&L.d_minmax, (size_t)B * 2 * sizeof(int)));
        L.minmax_cap = B;
    }
    return owlv2_preprocess(d_images, out_patches, L.d_minmax, B, H, W, G.in_h, G.in_w, *ty, *tx, h->d_lut, s, &L.v2_form);
}

static int preprocess_chunk(tstar_owl* h, tstar_owl::Lane& L, const uint8_t* d_images, int B, int H, int W, uint8_t* out_u8,
                            float* out_patches, hipStream_t s) {
    if (h->geom.family == TSTAR_OWL_FAMILY_OWLV2) {
        TSTAR_REQUIRE(!out_u8, "tstar_owl_debug_preprocess: an OWLv2 handle has no u8 stage (d_out_u8 must be NULL)");
        return preprocess_chunk_v2(h, L, d_images, B, H, W, out_patches, s);
    }
    ResampleTable *th, *tv;
    const OwlGeom& G = h->geom;
    RC(get_table(h, W, G.in_w, &th, s));
    RC(get_table(h, H, G.in_h, &tv, s));
    const size_t need = (size_t)B * H * G.in_w * 3;
    if (need > L.tmp_u8_bytes) {
        TSTAR_HIP_CHECK(hipStreamSynchronize(s));
        if (L.tmp_u8) TSTAR_HIP_CHECK(hipFree(L.tmp_u8));
        L.tmp_u8 = nullptr; L.tmp_u8_bytes = 0;
        TSTAR_HIP_CHECK(hipMalloc(&L.tmp_u8, need));
        L.tmp_u8_bytes = need;
    }
    RC(resample_h_u8(d_images, L.tmp_u8, B, H, W, *th, s));
    RC(resample_v_normalize_patchify(L.tmp_u8, out_patches, out_u8, B, H, G.in_w, *tv, h->d_lut, G.patch, s));
    return TSTAR_OK;
}

// One activation workspace for forward chunks of up to `cap` images: x, xn, att [Mp, 768], qkv [Mp, 2304], hid [Mp, 3072] with
// Mp = roundup(cap * ntok, 128) (ntok 577 at B/32, 2305 at B/16); zero-filled (rows past M are read by the last GEMM tile of a
// launch).  hid also holds the patch-embed A operand [cap * np, 3 P^2] (3072 or 768 columns: fits either way).
static hipError_t alloc_lane(tstar_owl::Lane& L, int cap, const OwlGeom& g) {
    const size_t mp = lane_rows(cap, g);
    hipError_t e = hipSuccess;
    auto alloc = [&](float** p, size_t n) { if (e == hipSuccess) { e = hipMalloc(p, n * sizeof(float)); if (e == hipSuccess) e = hipMemset(*p, 0, n * sizeof(float)); } };
    alloc(&L.x, mp * V_D); alloc(&L.xn, mp * V_D); alloc(&L.qkv, mp * 3 * V_D); alloc(&L.att, mp * V_D); alloc(&L.hid, mp * V_FF);
    if (e == hipSuccess) L.cap = cap;
    return e;
}
static void free_lane(tstar_owl::Lane& L) {
    void* ptrs[] = {L.x, L.xn, L.qkv, L.att, L.hid, L.tmp_u8, L.d_image_set, L.d_minmax};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    L = tstar_owl::Lane{};
}

#define CHECK_SET(set, fn) TSTAR_REQUIRE((set) >= 0 && (set) < TSTAR_OWL_MAX_SETS, fn ": query_set must be in 0..63")

// every image's query set is installed; *q_uniform = the common Q when every image uses one set size, else 0
static int check_image_sets(const tstar_owl* h, const int32_t* h_image_query_set, int B, int* q_uniform) {
    int qu = -1;
    for (int b = 0; b < B; ++b) {
        const int set = h_image_query_set ? h_image_query_set[b] : 0;
        CHECK_SET(set, "tstar_owl_score");
        if (h->Q[set] == 0) { set_error("tstar_owl_score: no queries installed in the requested query set (call tstar_owl_set_queries first)"); return TSTAR_ERR_STATE; }
        qu = (b == 0 || qu == h->Q[set]) ? h->Q[set] : 0;
    }
    *q_uniform = qu;
    return TSTAR_OK;
}

// the image -> set array of a call, copied into the lane's device staging (grown when a larger batch arrives)
static int stage_image_sets(tstar_owl::Lane& L, const int32_t* h_image_query_set, int B, hipStream_t s) {
    if (B > L.image_set_cap) {
        TSTAR_HIP_CHECK(hipStreamSynchronize(s));
        if (L.d_image_set) TSTAR_HIP_CHECK(hipFree(L.d_image_set));
        L.d_image_set = nullptr; L.image_set_cap = 0;
        TSTAR_HIP_CHECK(hipMalloc(&L.d_image_set, (size_t)B * sizeof(int)));
        L.image_set_cap = B;
    }
    TSTAR_HIP_CHECK(hipMemcpyAsync(L.d_image_set, h_image_query_set, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    return TSTAR_OK;
}

// boxes are relative to the resized image (OWL-ViT) or to the padded square (OWLv2: HF's _scale_boxes multiplies by max(H, W))
static void box_scale(const OwlGeom& G, int H, int W, float* sx, float* sy) {
    const bool v2 = G.family == TSTAR_OWL_FAMILY_OWLV2;
    *sx = (float)(v2 ? (H > W ? H : W) : W);
    *sy = (float)(v2 ? (H > W ? H : W) : H);
}

// the part of DetectRowsArgs that is the handle's own: head weights, installed queries
static DetectRowsArgs detect_args(const tstar_owl* h) {
    DetectRowsArgs a{};
    a.qn = h->qn; a.qmask = h->qmask; a.setQ = h->d_setQ;
    a.shift_w = h->vw.shift_w; a.shift_b = h->vw.shift_b; a.scale_w = h->vw.scale_w; a.scale_b = h->vw.scale_b;
    a.box2_w = h->vw.box2_w; a.box2_b = h->vw.box2_b; a.box_bias = h->vw.box_bias;
    return a;
}

// One forward chunk up to the head tensors, shared by scoring and the image-query embedding: pre-processing of either family,
// patch embedding, the encoder in the handle's weight mode, merge_cls_ln, the class head's dense0 and -- with want_boxes -- the box
// head's two GELU layers (without: bh1 / bh2 are only the free buffers the objectness head may use).  The tensors live in the
// lane's workspaces (L.x is free again on return).
struct OwlHeadTensors {
    float* feats;    // [Bc * np, 768]  L.xn
    float* cls;      // [Bc * np, 512]  L.att
    float* bh1;      // [Bc * np, 768]  L.qkv: the box head's first layer (free once bh2 is written)
    float* bh2;      // [Bc * np, 768]  L.hid
};
static int owl_forward_heads(tstar_owl* h, tstar_owl::Lane& L, const uint8_t* d_images, int Bc, int H, int W, bool want_boxes, OwlHeadTensors* t,
                             hipStream_t s) {
    const OwlGeom& G = h->geom;
    const int NP = G.np, NTOK = G.ntok, PK = G.patch_k;
    const int M = Bc * NTOK, MP = Bc * NP;
    RC(preprocess_chunk(h, L, d_images, Bc, H, W, nullptr, L.hid, s));
    GemmArgs pg = mk_gemm(h, L.hid, h->vw.patch_w, L.x, nullptr, nullptr, MP, V_D, PK, PK, V_D, ACT_NONE);
    pg.pos = h->vw.pos_emb; pg.patch_np = NP;
    RC(gemm_f32(pg, s));
    RC(write_cls_rows(L.x, h->vw.class_emb, h->vw.pos_emb, Bc, NTOK, V_D, s));
    RC(layernorm_f32(L.x, L.x, h->vw.pre_ln_w, h->vw.pre_ln_b, M, V_D, s));
    RC(run_encoder(h, L, h->vw.layers, V_LAYERS, Bc, NTOK, V_D, V_FF, V_HEADS, 0, nullptr, s));
    t->feats = L.xn; t->cls = L.att; t->bh1 = L.qkv; t->bh2 = L.hid;
    RC(merge_cls_ln(L.x, t->feats, h->vw.post_ln_w, h->vw.post_ln_b, h->vw.det_ln_w, h->vw.det_ln_b, Bc, NTOK, V_D, s));
    RC(gemm_f32(mk_gemm(h, t->feats, h->vw.cls_w, t->cls, h->vw.cls_b, nullptr, MP, PROJ, V_D, V_D, PROJ, ACT_NONE), s));
    if (!want_boxes) return TSTAR_OK;
    RC(gemm_f32(mk_gemm(h, t->feats, h->vw.box0_w, t->bh1, h->vw.box0_b, nullptr, MP, V_D, V_D, V_D, V_D, ACT_GELU), s));
    RC(gemm_f32(mk_gemm(h, t->bh1, h->vw.box1_w, t->bh2, h->vw.box1_b, nullptr, MP, V_D, V_D, V_D, V_D, ACT_GELU), s));
    return TSTAR_OK;
}

extern "C" {

const char* tstar_last_error(void) { return g_err.c_str(); }
int tstar_abi_version(void) { return 3; }
size_t tstar_owl_vision_blob_floats(void) { return vision_floats(OwlGeom{}); }
size_t tstar_owl_text_blob_floats(void) { return text_floats(); }
size_t tstar_owl_vision_blob_floats_ex(int image_size, int patch_size) {
    OwlGeom g;
    if (!owl_geom(image_size, patch_size, &g)) { set_error("tstar_owl_vision_blob_floats_ex: unsupported geometry (image 768, patch 32 or 16)"); return 0; }
    return vision_floats(g);
}
size_t tstar_owl_vision_blob_floats_in(int input_h, int input_w, int patch_size) {
    OwlGeom g;
    if (!owl_geom_input(input_h, input_w, patch_size, &g)) {
        set_error("tstar_owl_vision_blob_floats_in: unsupported input size (patch 32 or 16; each side a positive multiple of the patch size; at most 3600 patches)");
        return 0;
    }
    return vision_floats(g);
}
size_t tstar_owl_vision_blob_floats_family(int family, int input_h, int input_w, int patch_size) {
    OwlGeom g;
    if (!owl_geom_family(family, input_h, input_w, patch_size, &g)) {
        set_error("tstar_owl_vision_blob_floats_family: unsupported family / input size (family 0: patch 32 or 16; family 1 (OWLv2): patch 16; each "
                  "side a positive multiple of the patch size; at most 3600 patches)");
        return 0;
    }
    return vision_floats(g);
}
int tstar_owl_num_patches(tstar_owl* h) {
    if (!h) { set_error("tstar_owl_num_patches: null handle"); return -1; }
    return h->geom.np;
}

static int make_bf16_copies(tstar_owl* h, int mode) {
    struct Mat { const float* w; int n, k; };
    std::vector<Mat> mats;
    mats.push_back({h->vw.patch_w, V_D, h->geom.patch_k});
    auto layer = [&](const LayerW& l, int d, int ff) {
        mats.push_back({l.qkv_w, 3 * d, d}); mats.push_back({l.out_w, d, d});
        mats.push_back({l.fc1_w, ff, d}); mats.push_back({l.fc2_w, d, ff});
    };
    for (int i = 0; i < V_LAYERS; ++i) layer(h->vw.layers[i], V_D, V_FF);
    mats.push_back({h->vw.cls_w, PROJ, V_D});
    mats.push_back({h->vw.box0_w, V_D, V_D});
    mats.push_back({h->vw.box1_w, V_D, V_D});
    if (h->vw.obj0_w) { mats.push_back({h->vw.obj0_w, V_D, V_D}); mats.push_back({h->vw.obj1_w, V_D, V_D}); }
    if (h->has_text) {
        for (int i = 0; i < T_LAYERS; ++i) layer(h->tw.layers[i], T_D, T_FF);
        mats.push_back({h->tw.text_proj, PROJ, T_D});
    }
    for (auto& m : mats) {
        const size_t n = (size_t)m.n * m.k;
        int rc;
        if (mode == TSTAR_WEIGHTS_F32X3) {
            void* p = nullptr;
            TSTAR_HIP_CHECK(hipMalloc(&p, n * 6));
            h->wp[m.w] = p;
            rc = pack_weights_x3(m.w, p, m.n, m.k, 0);
        } else {
            __bf16* p = nullptr;
            TSTAR_HIP_CHECK(hipMalloc(&p, n * sizeof(__bf16)));
            h->wb[m.w] = p;
            rc = convert_f32_to_bf16(m.w, p, nullptr, n, 0);
            static const bool w2v_off = getenv("TSTAR_W2V_OFF") != nullptr;           // same-session A/Bs: every layer on the LDS tile
            if (!rc && mode == TSTAR_WEIGHTS_BF16 && m.n == 768 && m.k % 32 == 0 && !w2v_off) {       // per-shape dispatch (gemm_f32.hip plan_gemm)
                void* q = nullptr;
                TSTAR_HIP_CHECK(hipMalloc(&q, n * sizeof(__bf16)));
                h->wq[m.w] = q;
                rc = pack_weights_w2(p, q, m.n, m.k, 0);
            }
        }
        if (rc) return rc;
    }
    TSTAR_HIP_CHECK(hipDeviceSynchronize());
    h->weights_mode = mode;
    return TSTAR_OK;
}

int tstar_owl_create(tstar_owl** out, const float* h_vision_blob, size_t n_vision, const float* h_text_blob,
                     size_t n_text, const float* h_norm_lut, int max_batch, int weights_mode) {
    return tstar_owl_create_ex(out, 768, 32, h_vision_blob, n_vision, h_text_blob, n_text, h_norm_lut, max_batch, weights_mode);
}

int tstar_owl_create_ex(tstar_owl** out, int image_size, int patch_size, const float* h_vision_blob, size_t n_vision,
                        const float* h_text_blob, size_t n_text, const float* h_norm_lut, int max_batch, int weights_mode) {
    OwlGeom geom;
    TSTAR_REQUIRE(owl_geom(image_size, patch_size, &geom),
                  "tstar_owl_create_ex: unsupported geometry; supported: image 768 with patch 32 (B/32) or 16 (B/16)");
    return tstar_owl_create_in(out, geom.in_h, geom.in_w, patch_size, h_vision_blob, n_vision, h_text_blob, n_text, h_norm_lut, max_batch, weights_mode);
}

int tstar_owl_create_in(tstar_owl** out, int input_h, int input_w, int patch_size, const float* h_vision_blob, size_t n_vision,
                        const float* h_text_blob, size_t n_text, const float* h_norm_lut, int max_batch, int weights_mode) {
    return tstar_owl_create_family(out, TSTAR_OWL_FAMILY_OWLVIT, input_h, input_w, patch_size, h_vision_blob, n_vision, h_text_blob, n_text, h_norm_lut,
                                   max_batch, weights_mode);
}

int tstar_owl_create_family(tstar_owl** out, int family, int input_h, int input_w, int patch_size, const float* h_vision_blob, size_t n_vision,
                            const float* h_text_blob, size_t n_text, const float* h_norm_lut, int max_batch, int weights_mode) {
    OwlGeom geom;
    TSTAR_REQUIRE(family == TSTAR_OWL_FAMILY_OWLVIT || family == TSTAR_OWL_FAMILY_OWLV2, "tstar_owl_create_family: family must be 0 (OWL-ViT) or 1 (OWLv2)");
    TSTAR_REQUIRE(family != TSTAR_OWL_FAMILY_OWLV2 || patch_size == 16, "tstar_owl_create_family: OWLv2 is supported at patch 16 (B/16) only");
    TSTAR_REQUIRE(owl_geom_family(family, input_h, input_w, patch_size, &geom),
                  "tstar_owl_create_in: unsupported input size; supported: patch 32 (B/32) or 16 (B/16), each side of the input a positive "
                  "multiple of the patch size, at most 3600 patches");
    TSTAR_REQUIRE(out && (h_vision_blob || h_text_blob), "tstar_owl_create: null argument");
    TSTAR_REQUIRE(!h_vision_blob || h_norm_lut, "tstar_owl_create: the vision tower needs the normalisation LUT");
    TSTAR_REQUIRE(h_vision_blob || weights_mode == TSTAR_WEIGHTS_F32, "tstar_owl_create: a text-only handle runs in float32");
    TSTAR_REQUIRE(max_batch >= 1 && max_batch <= 1024, "tstar_owl_create: max_batch must be in 1..1024");
    TSTAR_REQUIRE(weights_mode == TSTAR_WEIGHTS_F32 || weights_mode == TSTAR_WEIGHTS_BF16 || weights_mode == TSTAR_WEIGHTS_BF16_EXACT ||
                      weights_mode == TSTAR_WEIGHTS_F32X3,
                  "tstar_owl_create: weights_mode must be 0 (f32), 1 (bf16), 3 (bf16, exact three-term activations) or 4 (f32x3); 2 (f32 split) was retired in ABI 3");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("tstar_owl_create: no HIP device visible (this library has no CPU path)");
        return TSTAR_ERR_HIP;
    }
    const int chunk_cap = max_batch < owl_chunk_limit(geom) ? max_batch : owl_chunk_limit(geom);
    TSTAR_REQUIRE(lane_rows(chunk_cap, geom) * V_FF < (size_t(1) << 31),
                  "tstar_owl_create: a forward chunk's workspace would reach 2^31 elements");
    tstar_owl* h = new tstar_owl();
    h->geom = geom;
    int rc = TSTAR_OK;
    if (h_vision_blob) {               // NULL: a text-only handle (CLIP text features for the YOLO-World backend)
        rc = upload_blob(h_vision_blob, n_vision, &h->d_vision, [&](auto&& take) { map_vision(h->vw, h->geom, take); });
        if (rc) { delete h; return rc; }
        h->has_vision = true;
    }
    if (h_text_blob) {
        rc = upload_blob(h_text_blob, n_text, &h->d_text, [&](auto&& take) { map_text(h->tw, take); });
        if (rc) { tstar_owl_destroy(h); return rc; }
        h->has_text = true;
    }
    h->max_batch = max_batch;
    h->chunk_cap = chunk_cap;
    h->mpad = lane_rows(chunk_cap, geom);
    hipError_t e = hipSuccess;
    auto alloc = [&](float** p, size_t n) { if (e == hipSuccess) { e = hipMalloc(p, n * sizeof(float)); if (e == hipSuccess) e = hipMemset(*p, 0, n * sizeof(float)); } };
    e = alloc_lane(h->lane[0], chunk_cap, geom);
    alloc(&h->d_lut, 768);
    constexpr int NSQ = TSTAR_OWL_MAX_SETS * TSTAR_OWL_MAX_QUERIES;
    alloc(&h->q_raw, (size_t)NSQ * PROJ); alloc(&h->qn, (size_t)NSQ * PROJ);
    if (e == hipSuccess) e = hipMalloc(&h->qweight, NSQ * sizeof(double));
    if (e == hipSuccess) e = hipMemset(h->qweight, 0, NSQ * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&h->qmask, NSQ);
    if (e == hipSuccess) e = hipMemset(h->qmask, 0, NSQ);
    if (e == hipSuccess) e = hipMalloc(&h->d_setQ, TSTAR_OWL_MAX_SETS * sizeof(int));
    if (e == hipSuccess) e = hipMemset(h->d_setQ, 0, TSTAR_OWL_MAX_SETS * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&h->d_ids, TSTAR_OWL_MAX_QUERIES * T_LEN * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&h->d_eos, TSTAR_OWL_MAX_QUERIES * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&h->d_kmask, TSTAR_OWL_MAX_QUERIES * T_LEN);
    if (e == hipSuccess && h_norm_lut && family == TSTAR_OWL_FAMILY_OWLVIT) e = hipMemcpy(h->d_lut, h_norm_lut, 768 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && h_norm_lut && family == TSTAR_OWL_FAMILY_OWLV2) {
        // OWLv2: h_norm_lut is mean[3], std[3]; the device holds the rescale table float32(float64(u8) * (1 / 255)) | mean | std
        float norm[262];
        for (int u = 0; u < 256; ++u) norm[u] = (float)((double)u * (1.0 / 255.0));
        for (int i = 0; i < 6; ++i) norm[256 + i] = h_norm_lut[i];
        e = hipMemcpy(h->d_lut, norm, sizeof(norm), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        set_error(std::string("tstar_owl_create: workspace allocation failed: ") + hipGetErrorString(e));
        tstar_owl_destroy(h);
        return TSTAR_ERR_HIP;
    }
    if (weights_mode != TSTAR_WEIGHTS_F32) {
        rc = make_bf16_copies(h, weights_mode);
        if (rc) { tstar_owl_destroy(h); return rc; }
    }
    *out = h;
    return TSTAR_OK;
}

int tstar_owl_destroy(tstar_owl* h) {
    if (!h) return TSTAR_OK;
    void* ptrs[] = {h->d_vision, h->d_text, h->d_lut, h->q_raw, h->qn, h->qweight, h->qmask, h->d_ids, h->d_eos, h->d_kmask, h->d_setQ};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (auto& L : h->lane) free_lane(L);
    for (auto& kv : h->tabs) free_table(&kv.second);
    for (auto& kv : h->tabs_v2) free_owlv2_axis_table(&kv.second);
    for (auto& kv : h->wb) if (kv.second) (void)hipFree(kv.second);
    for (auto& kv : h->wp) if (kv.second) (void)hipFree(kv.second);
    for (auto& kv : h->wq) if (kv.second) (void)hipFree(kv.second);
    delete h;
    return TSTAR_OK;
}

static int finish_queries(tstar_owl* h, int set, const uint8_t* h_mask, const double* h_w, int Q, hipStream_t s) {
    const size_t qo = (size_t)set * TSTAR_OWL_MAX_QUERIES;
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3(Q), dim3(64), 0, s, h->q_raw + qo * PROJ, h->qn + qo * PROJ, 1e-6f);
    TSTAR_HIP_CHECK(hipGetLastError());
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->qmask + qo, h_mask, Q, hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->qweight + qo, h_w, Q * sizeof(double), hipMemcpyHostToDevice, s));
    h->Q[set] = Q;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_setQ, h->Q, sizeof(h->Q), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

// Host staging of one text forward; lives until the stream has been synchronised (the copies below are asynchronous)
struct TextStage {
    std::vector<int> eos;
    std::vector<uint8_t> km, qm;
};

// The text tower on one query set in lane 0 (the handle's own workspace): token + position embedding -> L.x [Q*16, 512]; with
// pooled != 0 also the 12 layers, the final LayerNorm and the row of every sequence's first maximum id -> L.att [Q, 512].
static int text_forward(tstar_owl* h, const char* fn, const int32_t* h_ids, const int32_t* h_am, int Q, int pooled, TextStage& st, hipStream_t s) {
    auto& L = h->lane[0];
    st.eos.resize(Q); st.km.resize(Q * T_LEN); st.qm.resize(Q);
    for (int q = 0; q < Q; ++q) {
        int best = 0;
        for (int t = 0; t < T_LEN; ++t) {
            const int id = h_ids[q * T_LEN + t];
            TSTAR_REQUIRE(id >= 0 && id < T_VOCAB, std::string(fn) + ": token id out of range");
            if (id > h_ids[q * T_LEN + best]) best = t;        // argmax, first occurrence
            st.km[q * T_LEN + t] = h_am[q * T_LEN + t] != 0;
        }
        st.eos[q] = best;
        st.qm[q] = h_ids[q * T_LEN] > 0;                       // modeling_owlvit.py:1447
    }
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_ids, h_ids, Q * T_LEN * sizeof(int), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_eos, st.eos.data(), Q * sizeof(int), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_kmask, st.km.data(), Q * T_LEN, hipMemcpyHostToDevice, s));
    const int M = Q * T_LEN;
    hipLaunchKernelGGL(embed_tokens_kernel, dim3(M), dim3(128), 0, s, h->d_ids, h->tw.tok_emb, h->tw.tpos_emb, L.x,
                       T_LEN, T_D);
    TSTAR_HIP_CHECK(hipGetLastError());
    if (!pooled) return TSTAR_OK;
    RC(run_encoder(h, L, h->tw.layers, T_LAYERS, Q, T_LEN, T_D, T_FF, T_HEADS, 1, h->d_kmask, s));
    RC(layernorm_f32(L.x, L.xn, h->tw.final_ln_w, h->tw.final_ln_b, M, T_D, s));
    hipLaunchKernelGGL(gather_rows_kernel, dim3(Q), dim3(128), 0, s, L.xn, h->d_eos, L.att, T_LEN, T_D);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

int tstar_owl_set_queries(tstar_owl* h, int query_set, const int32_t* h_ids, const int32_t* h_am, const double* h_w, int Q,
                          void* stream) {
    TSTAR_REQUIRE(h && h_ids && h_am && h_w, "tstar_owl_set_queries: null argument");
    CHECK_SET(query_set, "tstar_owl_set_queries");
    TSTAR_REQUIRE(Q >= 1 && Q <= TSTAR_OWL_MAX_QUERIES, "tstar_owl_set_queries: Q must be in 1..32");
    if (!h->has_text) { set_error("tstar_owl_set_queries: handle was created without text weights"); return TSTAR_ERR_STATE; }
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[0];                                      // the text tower runs in the handle's own workspace
    TextStage st;
    RC(text_forward(h, "tstar_owl_set_queries", h_ids, h_am, Q, 1, st, s));
    RC(gemm_f32(mk_text_gemm(h, L.att, h->tw.text_proj, L.hid, nullptr, nullptr, Q, PROJ, T_D, T_D, PROJ, ACT_NONE), s));
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3(Q), dim3(64), 0, s, L.hid,
                       h->q_raw + (size_t)query_set * TSTAR_OWL_MAX_QUERIES * PROJ, 0.0f);
    TSTAR_HIP_CHECK(hipGetLastError());
    return finish_queries(h, query_set, st.qm.data(), h_w, Q, s);
}

int tstar_owl_debug_text(tstar_owl* h, const int32_t* h_ids, const int32_t* h_am, int Q, int stage, float* h_out, void* stream) {
    TSTAR_REQUIRE(h && h_ids && h_am && h_out, "tstar_owl_debug_text: null argument");
    TSTAR_REQUIRE(Q >= 1 && Q <= TSTAR_OWL_MAX_QUERIES, "tstar_owl_debug_text: Q must be in 1..32");
    TSTAR_REQUIRE(stage == 0 || stage == 1, "tstar_owl_debug_text: stage must be 0 (embedding rows) or 1 (pooled rows)");
    if (!h->has_text) { set_error("tstar_owl_debug_text: handle was created without text weights"); return TSTAR_ERR_STATE; }
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[0];
    TextStage st;
    RC(text_forward(h, "tstar_owl_debug_text", h_ids, h_am, Q, stage, st, s));
    const size_t n = (size_t)Q * (stage == 0 ? T_LEN : 1) * T_D;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h_out, stage == 0 ? L.x : L.att, n * sizeof(float), hipMemcpyDeviceToHost, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

int tstar_owl_set_queries_many(tstar_owl* h, int n_sets, const int32_t* h_sets, const int32_t* h_Q, const int32_t* h_ids, const int32_t* h_am,
                               const double* h_w, void* stream) {
    TSTAR_REQUIRE(h && h_sets && h_Q && h_ids && h_am && h_w, "tstar_owl_set_queries_many: null argument");
    TSTAR_REQUIRE(n_sets >= 1 && n_sets <= TSTAR_OWL_MAX_SETS, "tstar_owl_set_queries_many: n_sets must be in 1..64");
    if (!h->has_text) { set_error("tstar_owl_set_queries_many: handle was created without text weights"); return TSTAR_ERR_STATE; }
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[0];
    int total = 0;
    for (int i = 0; i < n_sets; ++i) {
        CHECK_SET(h_sets[i], "tstar_owl_set_queries_many");
        TSTAR_REQUIRE(h_Q[i] >= 1 && h_Q[i] <= TSTAR_OWL_MAX_QUERIES, "tstar_owl_set_queries_many: every Q must be in 1..32");
        total += h_Q[i];
    }
    for (int q = 0; q < total * T_LEN; ++q) TSTAR_REQUIRE(h_ids[q] >= 0 && h_ids[q] < T_VOCAB, "tstar_owl_set_queries_many: token id out of range");
    // sequences per text forward: what the activation workspace holds (mpad rows of >= T_D floats; T_LEN rows per sequence)
    const int cap = (int)(h->mpad / T_LEN);
    TSTAR_REQUIRE(cap >= TSTAR_OWL_MAX_QUERIES, "tstar_owl_set_queries_many: workspace too small");
    if (h->seq_cap < cap) {                                   // staging for ids / EOS positions / key masks of one forward
        TSTAR_HIP_CHECK(hipStreamSynchronize(s));
        if (h->d_ids) (void)hipFree(h->d_ids);
        if (h->d_eos) (void)hipFree(h->d_eos);
        if (h->d_kmask) (void)hipFree(h->d_kmask);
        h->d_ids = nullptr; h->d_eos = nullptr; h->d_kmask = nullptr; h->seq_cap = 0;
        TSTAR_HIP_CHECK(hipMalloc(&h->d_ids, (size_t)cap * T_LEN * sizeof(int)));
        TSTAR_HIP_CHECK(hipMalloc(&h->d_eos, (size_t)cap * sizeof(int)));
        TSTAR_HIP_CHECK(hipMalloc(&h->d_kmask, (size_t)cap * T_LEN));
        h->seq_cap = cap;
    }
    std::vector<int> eos(total);
    std::vector<uint8_t> km((size_t)total * T_LEN), qm(total);
    for (int q = 0; q < total; ++q) {
        int best = 0;
        for (int t = 0; t < T_LEN; ++t) {
            if (h_ids[q * T_LEN + t] > h_ids[q * T_LEN + best]) best = t;   // argmax, first occurrence
            km[(size_t)q * T_LEN + t] = h_am[q * T_LEN + t] != 0;
        }
        eos[q] = best;
        qm[q] = h_ids[q * T_LEN] > 0;
    }
    // ONE text forward per group of sets that fits the workspace: the same kernels as tstar_owl_set_queries on more rows (every
    // GEMM tile shape and the per-sequence causal attention give the same bits whatever the batch: results equal one-by-one calls)
    int i0 = 0, q0 = 0;
    while (i0 < n_sets) {
        int i1 = i0, nseq = 0;
        while (i1 < n_sets && nseq + h_Q[i1] <= cap) nseq += h_Q[i1++];
        const int M = nseq * T_LEN;
        TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_ids, h_ids + (size_t)q0 * T_LEN, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
        TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_eos, eos.data() + q0, nseq * sizeof(int), hipMemcpyHostToDevice, s));
        TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_kmask, km.data() + (size_t)q0 * T_LEN, M, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(embed_tokens_kernel, dim3(M), dim3(128), 0, s, h->d_ids, h->tw.tok_emb, h->tw.tpos_emb, L.x, T_LEN, T_D);
        TSTAR_HIP_CHECK(hipGetLastError());
        RC(run_encoder(h, L, h->tw.layers, T_LAYERS, nseq, T_LEN, T_D, T_FF, T_HEADS, 1, h->d_kmask, s));
        RC(layernorm_f32(L.x, L.xn, h->tw.final_ln_w, h->tw.final_ln_b, M, T_D, s));
        hipLaunchKernelGGL(gather_rows_kernel, dim3(nseq), dim3(128), 0, s, L.xn, h->d_eos, L.att, T_LEN, T_D);
        TSTAR_HIP_CHECK(hipGetLastError());
        RC(gemm_f32(mk_text_gemm(h, L.att, h->tw.text_proj, L.hid, nullptr, nullptr, nseq, PROJ, T_D, T_D, PROJ, ACT_NONE), s));
        int off = 0;
        for (int i = i0; i < i1; ++i) {
            const int set = h_sets[i], Q = h_Q[i];
            const size_t qo = (size_t)set * TSTAR_OWL_MAX_QUERIES;
            hipLaunchKernelGGL(l2norm_rows_kernel, dim3(Q), dim3(64), 0, s, L.hid + (size_t)off * PROJ, h->q_raw + qo * PROJ, 0.0f);
            hipLaunchKernelGGL(l2norm_rows_kernel, dim3(Q), dim3(64), 0, s, h->q_raw + qo * PROJ, h->qn + qo * PROJ, 1e-6f);
            TSTAR_HIP_CHECK(hipGetLastError());
            TSTAR_HIP_CHECK(hipMemcpyAsync(h->qmask + qo, qm.data() + q0 + off, Q, hipMemcpyHostToDevice, s));
            TSTAR_HIP_CHECK(hipMemcpyAsync(h->qweight + qo, h_w + q0 + off, Q * sizeof(double), hipMemcpyHostToDevice, s));
            h->Q[set] = Q;
            off += Q;
        }
        // the staging buffers are reused by the next group: wait for this one
        TSTAR_HIP_CHECK(hipStreamSynchronize(s));
        q0 += nseq;
        i0 = i1;
    }
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_setQ, h->Q, sizeof(h->Q), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

int tstar_owl_set_query_embeds(tstar_owl* h, int query_set, const float* h_qe, const uint8_t* h_mask, const double* h_w,
                               int Q, void* stream) {
    TSTAR_REQUIRE(h && h_qe && h_mask && h_w, "tstar_owl_set_query_embeds: null argument");
    CHECK_SET(query_set, "tstar_owl_set_query_embeds");
    TSTAR_REQUIRE(Q >= 1 && Q <= TSTAR_OWL_MAX_QUERIES, "tstar_owl_set_query_embeds: Q must be in 1..32");
    hipStream_t s = (hipStream_t)stream;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->q_raw + (size_t)query_set * TSTAR_OWL_MAX_QUERIES * PROJ, h_qe,
                                   (size_t)Q * PROJ * sizeof(float), hipMemcpyHostToDevice, s));
    return finish_queries(h, query_set, h_mask, h_w, Q, s);
}

int tstar_owl_set_class_weights(tstar_owl* h, int query_set, const double* h_w, int Q, void* stream) {
    TSTAR_REQUIRE(h && h_w, "tstar_owl_set_class_weights: null argument");
    CHECK_SET(query_set, "tstar_owl_set_class_weights");
    TSTAR_REQUIRE(Q == h->Q[query_set] && Q >= 1, "tstar_owl_set_class_weights: Q does not match the installed queries");
    hipStream_t s = (hipStream_t)stream;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->qweight + (size_t)query_set * TSTAR_OWL_MAX_QUERIES, h_w, Q * sizeof(double),
                                   hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

int tstar_owl_get_query_embeds(tstar_owl* h, int query_set, float* h_out, int Q, void* stream) {
    TSTAR_REQUIRE(h && h_out, "tstar_owl_get_query_embeds: null argument");
    CHECK_SET(query_set, "tstar_owl_get_query_embeds");
    TSTAR_REQUIRE(Q == h->Q[query_set], "tstar_owl_get_query_embeds: Q does not match the installed queries");
    hipStream_t s = (hipStream_t)stream;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h_out, h->q_raw + (size_t)query_set * TSTAR_OWL_MAX_QUERIES * PROJ,
                                   (size_t)Q * PROJ * sizeof(float), hipMemcpyDeviceToHost, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

// the body of the score entries; d_boxes_xyxy == nullptr (tstar_owl_score_cells, 1 x 1 grid): no box head, no box outputs
static int owl_score(tstar_owl* h, int lane, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                     const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy, double* d_cell_conf,
                     uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits, float* d_boxes_cxcywh, float* d_objectness, void* stream) {
    const bool want_boxes = d_boxes_xyxy != nullptr;
    TSTAR_REQUIRE(lane >= 0 && lane < TSTAR_OWL_LANES, "tstar_owl_score_lane: lane must be 0 or 1");
    TSTAR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "tstar_owl_score: empty batch or image");
    TSTAR_REQUIRE(grid_rows >= 1 && grid_cols >= 1, "tstar_owl_score: grid must be at least 1x1");
    if (!h->has_vision) { set_error("tstar_owl_score: handle was created without vision weights (text-only)"); return TSTAR_ERR_STATE; }
    TSTAR_REQUIRE(!d_objectness || h->geom.family == TSTAR_OWL_FAMILY_OWLV2, "tstar_owl_score_lane_obj: objectness needs an OWLv2 handle (OWL-ViT has no objectness head)");
    if (h->geom.family == TSTAR_OWL_FAMILY_OWLV2) {          // refusals before anything is launched
        const Owlv2Plan vp = plan_owlv2_preprocess(H, W, h->geom.in_h, h->geom.in_w);
        if (vp.error) { set_error(vp.error); return TSTAR_ERR_ARG; }
    }
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[lane];
    if (lane != 0) {
        // lane 1: allocated on first use (a one-off, like the resample tables) for forward chunks of min(max_batch, max(TSTAR_OWL_AUX_BATCH, B))
        // images, and grown when a larger batch arrives (the device is drained first)
        int need = B > TSTAR_OWL_AUX_BATCH ? B : TSTAR_OWL_AUX_BATCH;
        if (need > h->chunk_cap) need = h->chunk_cap;
        if (!L.x || L.cap < need) {
            if (L.x) { TSTAR_HIP_CHECK(hipDeviceSynchronize()); free_lane(L); }      // (rare: whichever stream used the smaller workspace last)
            const hipError_t e = alloc_lane(L, need, h->geom);
            if (e != hipSuccess) {
                free_lane(L);
                set_error(std::string("tstar_owl_score_lane: workspace allocation failed: ") + hipGetErrorString(e));
                return TSTAR_ERR_HIP;
            }
            TSTAR_HIP_CHECK(hipDeviceSynchronize());      // the zero fill ran on the null stream
        }
    }
    int q_uniform = -1;                                   // the common Q when every image uses one set size
    RC(check_image_sets(h, h_image_query_set, B, &q_uniform));
    TSTAR_REQUIRE(!d_logits || q_uniform > 0, "tstar_owl_score: raw logits need the same query count for every image");
    if (h_image_query_set) RC(stage_image_sets(L, h_image_query_set, B, s));
    const int ncell = grid_rows * grid_cols;
    const OwlGeom& G = h->geom;
    const int NP = G.np;
    for (int b0 = 0; b0 < B; b0 += L.cap) {
        const int Bc = (B - b0) < L.cap ? (B - b0) : L.cap;
        const int MP = Bc * NP;
        OwlHeadTensors t;
        RC(owl_forward_heads(h, L, d_images + (size_t)b0 * H * W * 3, Bc, H, W, want_boxes, &t, s));
        float *feats = t.feats, *cls = t.cls, *bh1 = t.bh1, *bh2 = t.bh2;
        DetectRowsArgs a = detect_args(h);
        a.feats = feats; a.cls = cls; a.boxh = want_boxes ? bh2 : nullptr;
        a.scores = d_scores + (size_t)b0 * NP;
        a.labels = d_labels + (size_t)b0 * NP;
        a.xyxy = want_boxes ? d_boxes_xyxy + (size_t)b0 * NP * 4 : nullptr;
        a.logits = d_logits ? d_logits + (size_t)b0 * NP * q_uniform : nullptr;
        a.image_set = h_image_query_set ? L.d_image_set + b0 : nullptr;
        a.cxcywh = d_boxes_cxcywh ? d_boxes_cxcywh + (size_t)b0 * NP * 4 : nullptr;
        a.rows = MP; a.np = NP; a.Q = q_uniform;
        box_scale(G, H, W, &a.box_sx, &a.box_sy);
        RC(detect_rows(a, s));
        if (d_objectness) {                                   // after detect_rows: feats is still whole, the heads' buffers are free
            RC(gemm_f32(mk_gemm(h, feats, h->vw.obj0_w, bh1, h->vw.obj0_b, nullptr, MP, V_D, V_D, V_D, V_D, ACT_GELU), s));
            RC(gemm_f32(mk_gemm(h, bh1, h->vw.obj1_w, bh2, h->vw.obj1_b, nullptr, MP, V_D, V_D, V_D, V_D, ACT_GELU), s));
            RC(row_dot768(bh2, h->vw.obj2_w, h->vw.obj2_b, d_objectness + (size_t)b0 * NP, MP, s));
        }
        RC(cell_reduce(a.scores, a.labels, a.xyxy, h->qweight, a.image_set, Bc, NP, W, H, grid_rows, grid_cols, 0.005f,
                       d_cell_conf + (size_t)b0 * ncell, d_cell_mask + (size_t)b0 * ncell,
                       d_n_kept ? d_n_kept + b0 : nullptr, s));
    }
    return TSTAR_OK;
}

int tstar_owl_score(tstar_owl* h, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                    const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy, double* d_cell_conf,
                    uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits, float* d_boxes_cxcywh, void* stream) {
    return tstar_owl_score_lane(h, 0, d_images, B, H, W, grid_rows, grid_cols, h_image_query_set, d_scores, d_labels, d_boxes_xyxy, d_cell_conf,
                                d_cell_mask, d_n_kept, d_logits, d_boxes_cxcywh, stream);
}

int tstar_owl_score_lane(tstar_owl* h, int lane, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                         const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy, double* d_cell_conf,
                         uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits, float* d_boxes_cxcywh, void* stream) {
    return tstar_owl_score_lane_obj(h, lane, d_images, B, H, W, grid_rows, grid_cols, h_image_query_set, d_scores, d_labels, d_boxes_xyxy, d_cell_conf,
                                    d_cell_mask, d_n_kept, d_logits, d_boxes_cxcywh, nullptr, stream);
}

int tstar_owl_score_lane_obj(tstar_owl* h, int lane, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                             const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy, double* d_cell_conf,
                             uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits, float* d_boxes_cxcywh, float* d_objectness, void* stream) {
    TSTAR_REQUIRE(h && d_images && d_scores && d_labels && d_boxes_xyxy && d_cell_conf && d_cell_mask,
                  "tstar_owl_score: null argument");
    return owl_score(h, lane, d_images, B, H, W, grid_rows, grid_cols, h_image_query_set, d_scores, d_labels, d_boxes_xyxy, d_cell_conf, d_cell_mask,
                     d_n_kept, d_logits, d_boxes_cxcywh, d_objectness, stream);
}

int tstar_owl_score_cells(tstar_owl* h, int lane, const uint8_t* d_images, int B, int H, int W, int grid_rows, int grid_cols,
                          const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, double* d_cell_conf, uint32_t* d_cell_mask,
                          int32_t* d_n_kept, float* d_logits, float* d_objectness, void* stream) {
    TSTAR_REQUIRE(h && d_images && d_scores && d_labels && d_cell_conf && d_cell_mask, "tstar_owl_score_cells: null argument");
    TSTAR_REQUIRE(grid_rows >= 1 && grid_cols >= 1, "tstar_owl_score: grid must be at least 1x1");
    TSTAR_REQUIRE(grid_rows * grid_cols == 1, "tstar_owl_score_cells: only a 1x1 grid can be scored without boxes (the cell of a detection is its box centre's)");
    return owl_score(h, lane, d_images, B, H, W, grid_rows, grid_cols, h_image_query_set, d_scores, d_labels, nullptr, d_cell_conf, d_cell_mask,
                     d_n_kept, d_logits, nullptr, d_objectness, stream);
}

int tstar_owl_debug_preprocess(tstar_owl* h, const uint8_t* d_images, int B, int H, int W, uint8_t* d_out_u8,
                               float* d_out_patches, void* stream) {
    TSTAR_REQUIRE(h && d_images && d_out_patches, "tstar_owl_debug_preprocess: null argument");
    TSTAR_REQUIRE(B >= 1 && B <= h->max_batch, "tstar_owl_debug_preprocess: B must be in 1..max_batch");
    if (!h->has_vision) { set_error("tstar_owl_debug_preprocess: handle was created without vision weights (text-only)"); return TSTAR_ERR_STATE; }
    return preprocess_chunk(h, h->lane[0], d_images, B, H, W, d_out_u8, d_out_patches, (hipStream_t)stream);
}

int tstar_owl_debug_heads(tstar_owl* h, const float* d_feats, const float* d_cls, const float* d_boxh, int B, int H, int W,
                          const int32_t* h_image_query_set, float* d_scores, int32_t* d_labels, float* d_boxes_xyxy, float* d_logits,
                          float* d_boxes_cxcywh, const float* d_obj_hidden, float* d_objectness, void* stream) {
    TSTAR_REQUIRE(h && d_feats && d_cls && d_boxh && d_scores && d_labels && d_boxes_xyxy, "tstar_owl_debug_heads: null argument");
    TSTAR_REQUIRE(B >= 1 && B <= h->max_batch, "tstar_owl_debug_heads: B must be in 1..max_batch");
    TSTAR_REQUIRE(H >= 1 && W >= 1, "tstar_owl_debug_heads: empty image");
    if (!h->has_vision) { set_error("tstar_owl_debug_heads: handle was created without vision weights (text-only)"); return TSTAR_ERR_STATE; }
    TSTAR_REQUIRE(!d_obj_hidden == !d_objectness, "tstar_owl_debug_heads: d_obj_hidden and d_objectness go together");
    TSTAR_REQUIRE(!d_objectness || h->geom.family == TSTAR_OWL_FAMILY_OWLV2, "tstar_owl_debug_heads: objectness needs an OWLv2 handle (OWL-ViT has no objectness head)");
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[0];
    int q_uniform = -1;
    RC(check_image_sets(h, h_image_query_set, B, &q_uniform));
    TSTAR_REQUIRE(!d_logits || q_uniform > 0, "tstar_owl_debug_heads: raw logits need the same query count for every image");
    if (h_image_query_set) RC(stage_image_sets(L, h_image_query_set, B, s));
    const int NP = h->geom.np;
    DetectRowsArgs a = detect_args(h);
    a.feats = d_feats; a.cls = d_cls; a.boxh = d_boxh;
    a.scores = d_scores; a.labels = d_labels; a.xyxy = d_boxes_xyxy; a.logits = d_logits; a.cxcywh = d_boxes_cxcywh;
    a.image_set = h_image_query_set ? L.d_image_set : nullptr;
    a.rows = B * NP; a.np = NP; a.Q = q_uniform;
    box_scale(h->geom, H, W, &a.box_sx, &a.box_sy);
    RC(detect_rows(a, s));
    if (d_objectness) RC(row_dot768(d_obj_hidden, h->vw.obj2_w, h->vw.obj2_b, d_objectness, B * NP, s));
    return TSTAR_OK;
}

int tstar_owl_debug_merge(tstar_owl* h, float* d_x, int B, int write_cls, float* d_feats, void* stream) {
    TSTAR_REQUIRE(h && d_x && d_feats, "tstar_owl_debug_merge: null argument");
    TSTAR_REQUIRE(B >= 1 && B <= h->max_batch, "tstar_owl_debug_merge: B must be in 1..max_batch");
    if (!h->has_vision) { set_error("tstar_owl_debug_merge: handle was created without vision weights (text-only)"); return TSTAR_ERR_STATE; }
    hipStream_t s = (hipStream_t)stream;
    if (write_cls) RC(write_cls_rows(d_x, h->vw.class_emb, h->vw.pos_emb, B, h->geom.ntok, V_D, s));
    return merge_cls_ln(d_x, d_feats, h->vw.post_ln_w, h->vw.post_ln_b, h->vw.det_ln_w, h->vw.det_ln_b, B, h->geom.ntok, V_D, s);
}

int tstar_owl_debug_embed(tstar_owl* h, const float* d_patches, int B, int stage, float* d_x, void* stream) {
    TSTAR_REQUIRE(h && d_patches && d_x, "tstar_owl_debug_embed: null argument");
    TSTAR_REQUIRE(stage == 0 || stage == 1, "tstar_owl_debug_embed: stage must be 0 (patch GEMM + class rows) or 1 (+ pre-LayerNorm)");
    if (!h->has_vision) { set_error("tstar_owl_debug_embed: handle was created without vision weights (text-only)"); return TSTAR_ERR_STATE; }
    auto& L = h->lane[0];
    TSTAR_REQUIRE(B >= 1 && B <= L.cap, "tstar_owl_debug_embed: B must be in 1..the images of one forward chunk (min(max_batch, chunk limit))");
    hipStream_t s = (hipStream_t)stream;
    const OwlGeom& G = h->geom;
    const int M = B * G.ntok;
    GemmArgs pg = mk_gemm(h, d_patches, h->vw.patch_w, L.x, nullptr, nullptr, B * G.np, V_D, G.patch_k, G.patch_k, V_D, ACT_NONE);
    pg.pos = h->vw.pos_emb; pg.patch_np = G.np;
    RC(gemm_f32(pg, s));
    RC(write_cls_rows(L.x, h->vw.class_emb, h->vw.pos_emb, B, G.ntok, V_D, s));
    if (stage == 1) RC(layernorm_f32(L.x, L.x, h->vw.pre_ln_w, h->vw.pre_ln_b, M, V_D, s));
    TSTAR_HIP_CHECK(hipMemcpyAsync(d_x, L.x, (size_t)M * V_D * sizeof(float), hipMemcpyDeviceToDevice, s));
    return TSTAR_OK;
}

int tstar_cell_reduce(const float* d_scores, const int32_t* d_labels, const float* d_boxes_xyxy, const double* h_weights, int n_sets,
                      const int32_t* h_image_set, int B, int np, int W, int H, int grid_rows, int grid_cols, float thr,
                      double* d_cell_conf, uint32_t* d_cell_mask, int32_t* d_n_kept, void* stream) {
    TSTAR_REQUIRE(d_scores && d_labels && d_boxes_xyxy && h_weights && d_cell_conf && d_cell_mask && d_n_kept, "tstar_cell_reduce: null argument");
    TSTAR_REQUIRE(B >= 1 && np >= 1 && W >= 1 && H >= 1, "tstar_cell_reduce: empty batch or image");
    TSTAR_REQUIRE(n_sets >= 1 && n_sets <= TSTAR_OWL_MAX_SETS, "tstar_cell_reduce: n_sets must be in 1..64");
    TSTAR_REQUIRE(grid_rows > 0 && grid_cols > 0 && grid_rows * grid_cols <= 4096, "tstar_cell_reduce: grid must have 1..4096 cells");
    for (int b = 0; h_image_set && b < B; ++b)
        TSTAR_REQUIRE(h_image_set[b] >= 0 && h_image_set[b] < n_sets, "tstar_cell_reduce: image set out of range");
    hipStream_t s = (hipStream_t)stream;
    double* d_w = nullptr;
    int* d_set = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&d_w, (size_t)n_sets * TSTAR_OWL_MAX_QUERIES * sizeof(double)));
    hipError_t e = hipMemcpyAsync(d_w, h_weights, (size_t)n_sets * TSTAR_OWL_MAX_QUERIES * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && h_image_set) {
        e = hipMalloc(&d_set, (size_t)B * sizeof(int));
        if (e == hipSuccess) e = hipMemcpyAsync(d_set, h_image_set, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s);
    }
    int rc = TSTAR_OK;
    if (e == hipSuccess)
        rc = cell_reduce(d_scores, d_labels, d_boxes_xyxy, d_w, d_set, B, np, W, H, grid_rows, grid_cols, thr, d_cell_conf, d_cell_mask, d_n_kept, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);           // the staging copies are freed below
    (void)hipFree(d_w);
    if (d_set) (void)hipFree(d_set);
    if (!rc && e != hipSuccess) { set_error(std::string("tstar_cell_reduce: ") + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    return rc;
}

// device results of the selection -> the caller's host arrays; the staging buffer is freed here
static int image_query_finish(const char* fn, int rc, void* d_buf, const ImageQueryOut& o, int n, float* h_embeds, int32_t* h_best, float* h_boxes,
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

int tstar_image_query_select(const float* d_cls, const float* d_boxes_cxcywh, int n, int np, float* h_embeds, int32_t* h_best, float* h_boxes_cxcywh,
                             int32_t* h_n_selected, int32_t* h_status, void* stream) {
    TSTAR_REQUIRE(d_cls && d_boxes_cxcywh && h_embeds && h_best && h_boxes_cxcywh && h_n_selected && h_status, "tstar_image_query_select: null argument");
    TSTAR_REQUIRE(n >= 1 && n <= 65535, "tstar_image_query_select: n must be in 1..65535");
    TSTAR_REQUIRE(np >= 1 && np <= IMAGE_QUERY_MAX_NP, "tstar_image_query_select: np must be in 1..3600");
    TSTAR_REQUIRE(((uintptr_t)d_cls & 15) == 0, "tstar_image_query_select: d_cls must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    void* d_buf = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&d_buf, image_query_out_bytes(n)));
    const ImageQueryOut o = image_query_out_at(d_buf, n);
    const int rc = image_query_select(d_cls, d_boxes_cxcywh, n, np, o, s);
    return image_query_finish("tstar_image_query_select", rc, d_buf, o, n, h_embeds, h_best, h_boxes_cxcywh, h_n_selected, h_status, s);
}

int tstar_owl_embed_image_queries(tstar_owl* h, const uint8_t* d_images, int n, int H, int W, float* h_embeds, int32_t* h_best, float* h_boxes_cxcywh,
                                  int32_t* h_n_selected, int32_t* h_status, void* stream) {
    TSTAR_REQUIRE(h && d_images && h_embeds && h_best && h_boxes_cxcywh && h_n_selected && h_status, "tstar_owl_embed_image_queries: null argument");
    TSTAR_REQUIRE(n >= 1 && n <= 65535 && H >= 1 && W >= 1, "tstar_owl_embed_image_queries: empty batch or image (n in 1..65535)");
    if (!h->has_vision) { set_error("tstar_owl_embed_image_queries: handle was created without vision weights (text-only)"); return TSTAR_ERR_STATE; }
    if (h->geom.family == TSTAR_OWL_FAMILY_OWLV2) {          // refusals before anything is launched
        const Owlv2Plan vp = plan_owlv2_preprocess(H, W, h->geom.in_h, h->geom.in_w);
        if (vp.error) { set_error(vp.error); return TSTAR_ERR_ARG; }
    }
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[0];                                     // the handle's own workspace, as the text tower
    const int NP = h->geom.np;
    void* d_buf = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&d_buf, image_query_out_bytes(n)));
    const ImageQueryOut o = image_query_out_at(d_buf, n);
    int rc = TSTAR_OK;
    for (int b0 = 0; b0 < n && !rc; b0 += L.cap) {
        const int Bc = (n - b0) < L.cap ? (n - b0) : L.cap;
        const int MP = Bc * NP;
        OwlHeadTensors t;
        rc = owl_forward_heads(h, L, d_images + (size_t)b0 * H * W * 3, Bc, H, W, true, &t, s);
        if (rc) break;
        // the box head's tail is detect_rows, as in tstar_owl_score (the boxes are its d_boxes_cxcywh bits); what it writes besides
        // goes to L.x, which is free after merge_cls_ln: scores | labels | xyxy | cxcywh, each at a multiple of four floats
        const size_t R = round_up((size_t)MP, 4);
        DetectRowsArgs a = detect_args(h);
        a.feats = t.feats; a.cls = t.cls; a.boxh = t.bh2;
        a.scores = L.x; a.labels = reinterpret_cast<int*>(L.x + R); a.xyxy = L.x + 2 * R; a.cxcywh = L.x + 6 * R;
        a.logits = nullptr; a.image_set = nullptr;
        a.rows = MP; a.np = NP; a.Q = h->Q[0];
        box_scale(h->geom, H, W, &a.box_sx, &a.box_sy);
        rc = detect_rows(a, s);
        if (!rc) rc = image_query_select(t.cls, a.cxcywh, Bc, NP, image_query_out_offset(o, b0), s);
    }
    return image_query_finish("tstar_owl_embed_image_queries", rc, d_buf, o, n, h_embeds, h_best, h_boxes_cxcywh, h_n_selected, h_status, s);
}

int tstar_owlv2_last_preprocess_form(tstar_owl* h, int lane) {
    if (!h || lane < 0 || lane >= TSTAR_OWL_LANES) { set_error("tstar_owlv2_last_preprocess_form: null handle or bad lane"); return -1; }
    return h->lane[lane].v2_form;
}

int tstar_owlv2_set_axis_weights(tstar_owl* h, int S, int out, const double* gw, int n) {
    TSTAR_REQUIRE(h && gw && S >= 2 && out >= 1, "tstar_owlv2_set_axis_weights: bad argument");
    const Owlv2Axis a = owlv2_axis(S, out);
    TSTAR_REQUIRE(n == (a.radius > 0 ? a.radius : 0) + 1, "tstar_owlv2_set_axis_weights: n must be the axis' radius + 1");
    const auto key = std::make_pair(S, out);
    auto it = h->tabs_v2.find(key);
    if (it != h->tabs_v2.end()) {                            // a table built from other weights: drop it once the device is done with it
        TSTAR_HIP_CHECK(hipDeviceSynchronize());
        free_owlv2_axis_table(&it->second);
        h->tabs_v2.erase(it);
    }
    h->gw_v2[key] = std::vector<double>(gw, gw + n);
    return TSTAR_OK;
}

int tstar_owlv2_preprocess_plan(int H, int W, int out_h, int out_w, int* plan10) {
    TSTAR_REQUIRE(plan10, "tstar_owlv2_preprocess_plan: null argument");
    const Owlv2Plan p = plan_owlv2_preprocess(H, W, out_h, out_w);
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    const int v[10] = {p.form, p.tile_h, p.tile_w, p.win_h, p.win_w, p.lds_bytes, p.grid_x, p.grid_y, p.radius_y, p.radius_x};
    for (int i = 0; i < 10; ++i) plan10[i] = v[i];
    return TSTAR_OK;
}

int tstar_owlv2_axis_window(int S, int out, int tile, int k, int radius, int* lo_n2) {
    TSTAR_REQUIRE(lo_n2 && S >= 2 && out >= 1 && tile >= 1 && k >= 0 && k * tile < out, "tstar_owlv2_axis_window: bad argument");
    owlv2_axis_window(S, out, tile, k, radius, &lo_n2[0], &lo_n2[1]);
    return TSTAR_OK;
}

int tstar_owlv2_axis_tables(int S, int out, int32_t* i0, int32_t* i1, double* t, double* gw, int gw_cap) {
    TSTAR_REQUIRE(i0 && i1 && t && gw && S >= 2 && out >= 1, "tstar_owlv2_axis_tables: bad argument");
    std::vector<int> a, b;
    std::vector<double> tt, g;
    owlv2_axis_host(S, out, a, b, tt, g);
    TSTAR_REQUIRE((int)g.size() <= gw_cap, "tstar_owlv2_axis_tables: gw_cap is smaller than radius + 1");
    for (int j = 0; j < out; ++j) { i0[j] = a[j]; i1[j] = b[j]; t[j] = tt[j]; }
    for (size_t k = 0; k < g.size(); ++k) gw[k] = g[k];
    return TSTAR_OK;
}

int tstar_frames_to_grid(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx, int grid_rows,
                         int grid_cols, uint8_t* d_grid, int nv12, void* stream) {
    TSTAR_REQUIRE(d_video && d_frame_idx && d_grid, "tstar_frames_to_grid: null argument");
    TSTAR_REQUIRE(N >= 1 && H >= 2 && W >= 2, "tstar_frames_to_grid: bad video shape");
    TSTAR_REQUIRE(!nv12 || (H % 2 == 0 && W % 2 == 0), "tstar_frames_to_grid: NV12 needs even dimensions");
    return frames_to_grid_u8(d_video, H, W, d_frame_idx, grid_rows, grid_cols, 200, 95, d_grid, nv12, (hipStream_t)stream);
}

int tstar_frames_resize(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx, int n, int out_w,
                        int out_h, uint8_t* d_out, int nv12, void* stream) {
    TSTAR_REQUIRE(d_video && d_frame_idx && d_out, "tstar_frames_resize: null argument");
    TSTAR_REQUIRE(N >= 1 && H >= 2 && W >= 2, "tstar_frames_resize: bad video shape");
    TSTAR_REQUIRE(!nv12 || (H % 2 == 0 && W % 2 == 0), "tstar_frames_resize: NV12 needs even dimensions");
    return bilinear_gather_u8(d_video, H, W, d_frame_idx, n, out_w, out_h, d_out, nv12, (hipStream_t)stream);
}

int tstar_nv12_to_rgb(const uint8_t* d_video, int N, int H, int W, const int32_t* d_frame_idx, int n, uint8_t* d_out,
                      void* stream) {
    TSTAR_REQUIRE(d_video && d_frame_idx && d_out, "tstar_nv12_to_rgb: null argument");
    TSTAR_REQUIRE(N >= 1 && H >= 2 && W >= 2, "tstar_nv12_to_rgb: bad video shape");
    return nv12_to_rgb_u8(d_video, H, W, d_frame_idx, n, d_out, (hipStream_t)stream);
}

int tstar_i420_to_nv12(const uint8_t* d_i420, int n, int H, int W, uint8_t* d_nv12, void* stream) {
    TSTAR_REQUIRE(d_i420 && d_nv12 && d_i420 != d_nv12, "tstar_i420_to_nv12: null or aliased argument");
    return i420_to_nv12_u8(d_i420, n, H, W, d_nv12, (hipStream_t)stream);
}

int tstar_jpeg_entropy_device(const uint8_t* d_bytes, size_t total_bytes, const void* d_segments, const void* d_table_sets,
                              int n_sets, const void* d_frames, int n_frames, int n_segments, int W, int H, int ncomp, int hs,
                              int vs, int16_t* d_coef, int32_t* d_seg_status, void* stream) {
    jpegcore::SegmentBatch b;
    const char* bad = jpegcore::segment_batch(d_bytes, total_bytes, d_segments, d_table_sets, n_sets, d_frames, n_frames, n_segments,
                                              JpegGeom{W, H, ncomp, hs, vs}, d_coef, d_seg_status, &b);
    TSTAR_REQUIRE(!bad, std::string("tstar_jpeg_entropy_device: ") + bad);
    return jpeg_entropy_segments(b, (hipStream_t)stream);
}

int tstar_jpeg_entropy_split_device(const uint8_t* d_bytes, size_t total_bytes, const void* d_segments, const void* d_table_sets,
                                    int n_sets, const void* d_frames, int n_frames, int n_segments, int W, int H, int ncomp, int hs,
                                    int vs, int sub_bytes, int min_split_bytes, int max_rounds, void* d_workspace,
                                    size_t workspace_bytes, int16_t* d_coef, int32_t* d_seg_status, int32_t* d_seg_info, void* stream) {
    TSTAR_REQUIRE(d_seg_info && d_workspace, "tstar_jpeg_entropy_split_device: null argument");
    jpegcore::SegmentBatch b;
    const char* bad = jpegcore::segment_batch(d_bytes, total_bytes, d_segments, d_table_sets, n_sets, d_frames, n_frames, n_segments,
                                              JpegGeom{W, H, ncomp, hs, vs}, d_coef, d_seg_status, &b);
    TSTAR_REQUIRE(!bad, std::string("tstar_jpeg_entropy_split_device: ") + bad);
    return jpeg_entropy_split(b, sub_bytes, min_split_bytes, max_rounds, d_workspace, workspace_bytes, d_seg_info, (hipStream_t)stream);
}

int tstar_jpeg_reconstruct(const int16_t* d_coef, const uint16_t* d_quant, int n, int W, int H, int ncomp, int hs, int vs,
                           uint8_t* d_planes, uint8_t* d_rgb, void* stream) {
    TSTAR_REQUIRE(d_coef && d_quant && d_planes && d_rgb, "tstar_jpeg_reconstruct: null argument");
    const JpegGeom g{W, H, ncomp, hs, vs};
    return jpeg_reconstruct_u8(d_coef, d_quant, n, g, d_planes, d_rgb, (hipStream_t)stream);
}

int tstar_gemm_f32(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual, int M,
                   int N, int K, int act, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_f32: null argument");
    return gemm_f32(mk_gemm(nullptr, d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act), (hipStream_t)stream);
}

int tstar_gemm_f32_cfg(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual,
                       int M, int N, int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_f32_cfg: null argument");
    GemmArgs g = mk_gemm(nullptr, d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act);
    g.tile_cfg = tile_cfg;
    return gemm_f32(g, (hipStream_t)stream);
}

static int gemm_converted(const char* fn, int a_terms, const float* d_A, const float* d_W, float* d_C, const float* d_bias,
                          const float* d_residual, int M, int N, int K, int act, int tile_cfg, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    __bf16* wb = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&wb, (size_t)N * K * sizeof(__bf16)));
    int rc = convert_f32_to_bf16(d_W, wb, nullptr, (size_t)N * K, s);
    void* wq = nullptr;
    if (!rc && a_terms == 2 && N % 256 == 0 && K % 32 == 0) {       // the fragment-packed plane of the two-term mode's VGPR-weight tile (tile_cfg 6, or N = 768)
        TSTAR_HIP_CHECK(hipMalloc(&wq, (size_t)N * K * sizeof(__bf16)));
        rc = pack_weights_w2(wb, wq, N, K, s);
    }
    if (!rc) {
        GemmArgs g = mk_gemm(nullptr, d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act);
        g.Wb = wb;
        g.Wq = wq;
        g.a_terms = a_terms;
        g.tile_cfg = tile_cfg;
        rc = gemm_f32(g, s);
    }
    hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(wb);
    if (wq) (void)hipFree(wq);
    if (!rc && e != hipSuccess) { set_error(std::string(fn) + ": " + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    return rc;
}

int tstar_gemm_bf16w(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual, int M,
                     int N, int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_bf16w: null argument");
    return gemm_converted("tstar_gemm_bf16w", 0, d_A, d_W, d_C, d_bias, d_residual, M, N, K, act, tile_cfg, stream);
}

int tstar_gemm_bf16w_pre(const float* d_A, const void* d_Wb, float* d_C, const float* d_bias, const float* d_residual, int M, int N,
                         int K, int act, int a_terms, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_Wb && d_C, "tstar_gemm_bf16w_pre: null argument");
    TSTAR_REQUIRE(a_terms == 2 || a_terms == 3, "tstar_gemm_bf16w_pre: a_terms must be 2 or 3");
    GemmArgs g = mk_gemm(nullptr, d_A, reinterpret_cast<const float*>(d_Wb), d_C, d_bias, d_residual, M, N, K, K, N, act);
    g.Wb = static_cast<const __bf16*>(d_Wb);
    g.a_terms = a_terms;
    g.tile_cfg = tile_cfg;
    return gemm_f32(g, (hipStream_t)stream);
}

int tstar_gemm_bf16w2(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual, int M,
                      int N, int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_bf16w2: null argument");
    return gemm_converted("tstar_gemm_bf16w2", 2, d_A, d_W, d_C, d_bias, d_residual, M, N, K, act, tile_cfg, stream);
}

int tstar_gemm_f32x3(const float* d_A, const float* d_W, float* d_C, const float* d_bias, const float* d_residual, int M,
                     int N, int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_C, "tstar_gemm_f32x3: null argument");
    TSTAR_REQUIRE(M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 32 == 0, "tstar_gemm_f32x3: N must be a multiple of 128, K of 32 (include/tstar_hip.h)");
    hipStream_t s = (hipStream_t)stream;
    void* wp = nullptr;
    TSTAR_HIP_CHECK(hipMalloc(&wp, (size_t)N * K * 6));
    int rc = pack_weights_x3(d_W, wp, N, K, s);
    if (!rc) {
        GemmArgs g = mk_gemm(nullptr, d_A, d_W, d_C, d_bias, d_residual, M, N, K, K, N, act);
        g.Wp = wp;
        g.tile_cfg = tile_cfg;
        rc = gemm_f32(g, s);
    }
    hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(wp);
    if (!rc && e != hipSuccess) { set_error(std::string("tstar_gemm_f32x3: ") + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    return rc;
}

int tstar_pack_f32x3(const float* d_W, void* d_Wp, int N, int K, void* stream) {
    TSTAR_REQUIRE(d_W && d_Wp, "tstar_pack_f32x3: null argument");
    TSTAR_REQUIRE(N > 0 && K > 0, "tstar_pack_f32x3: empty matrix");
    return pack_weights_x3(d_W, d_Wp, N, K, (hipStream_t)stream);
}

int tstar_gemm_f32x3_pre(const float* d_A, const void* d_Wp, float* d_C, const float* d_bias, const float* d_residual, int M, int N,
                         int K, int act, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_Wp && d_C, "tstar_gemm_f32x3_pre: null argument");
    TSTAR_REQUIRE(M > 0 && N > 0 && K > 0 && N % 128 == 0 && K % 32 == 0, "tstar_gemm_f32x3_pre: N must be a multiple of 128, K of 32 (include/tstar_hip.h)");
    GemmArgs g = mk_gemm(nullptr, d_A, reinterpret_cast<const float*>(d_Wp), d_C, d_bias, d_residual, M, N, K, K, N, act);
    g.Wp = d_Wp;
    g.tile_cfg = tile_cfg;
    return gemm_f32(g, (hipStream_t)stream);
}

static int gemm_wmode_of(int weights_mode) {
    return weights_mode == TSTAR_WEIGHTS_F32 ? GEMM_W_F32 : weights_mode == TSTAR_WEIGHTS_BF16 ? GEMM_W_BF16_2T :
           weights_mode == TSTAR_WEIGHTS_BF16_EXACT ? GEMM_W_BF16_EXACT : weights_mode == TSTAR_WEIGHTS_F32X3 ? GEMM_W_F32X3 : -1;
}

int tstar_gemm_plan(int weights_mode, int M, int N, int ldc, int patch_np, int tile_cfg, int has_packed_w2, int* plan4) {
    TSTAR_REQUIRE(plan4, "tstar_gemm_plan: null argument");
    const GemmPlan p = plan_gemm(gemm_wmode_of(weights_mode), M, N, ldc, patch_np, tile_cfg, has_packed_w2 != 0);
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    plan4[0] = p.kind; plan4[1] = p.m_split; plan4[2] = p.blocks; plan4[3] = p.lds_bytes;
    return TSTAR_OK;
}

// The patch-embedding launch of owl_forward_heads (pos != nullptr, patch_np = np: the PATCH epilogue) on caller-supplied operands, with
// the weight planes of `weights_mode` made as the tstar_gemm_* diagnostics make them.  Every refusal comes before the first allocation.
int tstar_gemm_patch_embed(const float* d_A, const float* d_W, float* d_X, const float* d_pos, int B, int np, int N, int K,
                           int weights_mode, int tile_cfg, void* stream) {
    TSTAR_REQUIRE(d_A && d_W && d_X && d_pos, "tstar_gemm_patch_embed: null argument");
    TSTAR_REQUIRE(B >= 1 && np >= 1, "tstar_gemm_patch_embed: B and np must be at least 1");
    TSTAR_REQUIRE((long long)B * (np + 1ll) < (1ll << 31), "tstar_gemm_patch_embed: B * (np + 1) token rows do not fit an int");
    const int wmode = gemm_wmode_of(weights_mode);
    TSTAR_REQUIRE(wmode >= 0, "tstar_gemm_patch_embed: unknown weights_mode (a TSTAR_WEIGHTS_* value)");
    TSTAR_REQUIRE(N > 0 && K > 0 && K % 32 == 0, "tstar_gemm_patch_embed: K must be a positive multiple of 32 (gemm_f32)");
    const int M = B * np;
    const bool two_term = weights_mode == TSTAR_WEIGHTS_BF16;
    const bool has_wq = two_term && N % 256 == 0;             // the fragment-packed plane, where gemm_converted makes one
    const GemmPlan p = plan_gemm(wmode, M, N, N, np, tile_cfg, has_wq);
    if (p.error) { set_error(std::string("tstar_gemm_patch_embed: ") + p.error); return TSTAR_ERR_ARG; }
    hipStream_t s = (hipStream_t)stream;
    __bf16* wb = nullptr;
    void *wq = nullptr, *wp = nullptr;
    int rc = TSTAR_OK;
    if (two_term || weights_mode == TSTAR_WEIGHTS_BF16_EXACT) {
        TSTAR_HIP_CHECK(hipMalloc(&wb, (size_t)N * K * sizeof(__bf16)));
        rc = convert_f32_to_bf16(d_W, wb, nullptr, (size_t)N * K, s);
        if (!rc && has_wq) {
            TSTAR_HIP_CHECK(hipMalloc(&wq, (size_t)N * K * sizeof(__bf16)));
            rc = pack_weights_w2(wb, wq, N, K, s);
        }
    } else if (weights_mode == TSTAR_WEIGHTS_F32X3) {
        TSTAR_HIP_CHECK(hipMalloc(&wp, (size_t)N * K * 6));
        rc = pack_weights_x3(d_W, wp, N, K, s);
    }
    if (!rc) {
        GemmArgs g = mk_gemm(nullptr, d_A, d_W, d_X, nullptr, nullptr, M, N, K, K, N, ACT_NONE);
        g.Wb = wb; g.Wq = wq; g.Wp = wp;
        g.a_terms = two_term ? 2 : wb ? 3 : 0;
        g.pos = d_pos; g.patch_np = np;
        g.tile_cfg = tile_cfg;
        rc = gemm_f32(g, s);
    }
    hipError_t e = hipStreamSynchronize(s);
    if (wb) (void)hipFree(wb);
    if (wq) (void)hipFree(wq);
    if (wp) (void)hipFree(wp);
    if (!rc && e != hipSuccess) { set_error(std::string("tstar_gemm_patch_embed: ") + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    return rc;
}

int tstar_ingest_plan(int op, int nv12, int H, int W, int n, int ow, int oh, int out_aligned4, int video_aligned4, int generic, int nv12_lds,
                      int grid_px, int* plan6) {
    TSTAR_REQUIRE(plan6, "tstar_ingest_plan: null argument");
    const IngestPlan p = plan_ingest(op, nv12 != 0, H, W, n, ow, oh, out_aligned4 != 0, video_aligned4 != 0, IngestOverrides{generic != 0, nv12_lds != 0, grid_px});
    if (p.error) { set_error(p.error); return TSTAR_ERR_ARG; }
    plan6[0] = p.kind; plan6[1] = p.px; plan6[2] = (int)p.grid_x; plan6[3] = (int)p.grid_y; plan6[4] = p.lds_bytes; plan6[5] = p.lds_pitch;
    return TSTAR_OK;
}

int tstar_layernorm_f32(const float* d_x, float* d_y, const float* d_w, const float* d_b, int rows, int D, void* stream) {
    TSTAR_REQUIRE(d_x && d_y && d_w && d_b, "tstar_layernorm_f32: null argument");
    return layernorm_f32(d_x, d_y, d_w, d_b, rows, D, (hipStream_t)stream);
}

int tstar_attention_f32(const float* d_qkv, float* d_out, int B, int T, int heads, int mode, const uint8_t* d_key_mask,
                        void* stream) {
    TSTAR_REQUIRE(d_qkv && d_out, "tstar_attention_f32: null argument");
    return attention_f32(d_qkv, d_out, B, T, heads, mode, d_key_mask, (hipStream_t)stream);
}

int tstar_draw_boxes(uint8_t* d_images, int B, int H, int W, const float* d_boxes_xyxy, const float* d_scores, void* stream) {
    TSTAR_REQUIRE(d_images && d_boxes_xyxy && d_scores, "tstar_draw_boxes: null argument");
    return draw_boxes(d_images, B, H, W, d_boxes_xyxy, d_scores, V_NP, 0.005f, (hipStream_t)stream);
}

int tstar_draw_boxes_np(uint8_t* d_images, int B, int H, int W, const float* d_boxes_xyxy, const float* d_scores, int np, void* stream) {
    TSTAR_REQUIRE(d_images && d_boxes_xyxy && d_scores, "tstar_draw_boxes_np: null argument");
    TSTAR_REQUIRE(np >= 1, "tstar_draw_boxes_np: np must be positive");
    return draw_boxes(d_images, B, H, W, d_boxes_xyxy, d_scores, np, 0.005f, (hipStream_t)stream);
}

int tstar_attention_x3(const float* d_qkv, float* d_out, int B, int T, int heads, void* stream) {
    TSTAR_REQUIRE(d_qkv && d_out, "tstar_attention_x3: null argument");
    return attention_x3(d_qkv, d_out, B, T, heads, (hipStream_t)stream);
}

int tstar_attention_x3_order(const float* d_qkv, float* d_out, int B, int T, int heads, int order, void* stream) {
    TSTAR_REQUIRE(d_qkv && d_out, "tstar_attention_x3_order: null argument");
    TSTAR_REQUIRE(order == 0 || order == 1, "tstar_attention_x3_order: order must be 0 (linear) or 1 (XCD groups)");
    return attention_x3(d_qkv, d_out, B, T, heads, (hipStream_t)stream, order);
}

int tstar_xcd_group_block(int bid, int ngroups, int gsize) {
    if (bid < 0 || ngroups < 1 || gsize < 1 || bid >= xcd_groups_grid(ngroups, gsize)) return -2;
    return xcd_remap_groups(bid, ngroups, gsize);
}
int tstar_xcd_groups_grid(int ngroups, int gsize) { return ngroups < 1 || gsize < 1 ? -1 : xcd_groups_grid(ngroups, gsize); }

int tstar_attention_split(const float* d_qkv, float* d_out, int B, int T, int heads, void* stream) {
    TSTAR_REQUIRE(d_qkv && d_out, "tstar_attention_split: null argument");
    return attention_split(d_qkv, d_out, B, T, heads, (hipStream_t)stream);
}

}  // extern "C"
