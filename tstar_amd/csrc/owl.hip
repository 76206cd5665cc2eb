// The OWL-ViT / OWLv2 detector handle (include/tstar_hip.h: tstar_owl_*, tstar_owlv2_*): weights, workspace lanes, text tower, query
// sets and the forward orchestration over the hand-written gfx950 kernels.
#include "../../include/tstar_hip.h"
#include "common.h"
#include "heads.h"
#include "image_query.h"
#include "kernels.h"
#include "owl_weights.h"
#include "preprocess_v2.h"
#include "records.h"
#include <math.h>
#include <map>
#include <string.h>
#include <unordered_map>
#include <vector>

namespace tstar {
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
        DeviceBuf<uint8_t> tmp_u8;                                   // OWL-ViT: the chunk's images after the horizontal resampling pass
        DeviceBuf<int> minmax;                                       // OWLv2: per-image clip bounds of the pre-processing (two ints per image)
        int v2_form = -1;                                            // OWLv2: form of the last pre-processing launch (OWLV2_FORM_*)
        DeviceBuf<int> image_set;                                    // the image -> query set array of a call
        int cap = 0;                                                 // images per forward chunk
    } lane[TSTAR_OWL_LANES];
    // query sets: TSTAR_OWL_MAX_SETS independent (question) slots, each up to 32 queries; every image of
    // a score call names the slot it is scored against (several (video, question) items batched together)
    int Q[TSTAR_OWL_MAX_SETS] = {0};
    float *q_raw = nullptr, *qn = nullptr;                           // [sets][32][512]
    double* qweight = nullptr;                                       // [sets][32] object2weight per query (float64, as the reference's Python floats)
    uint8_t* qmask = nullptr;                                        // [sets][32]
    int* d_setQ = nullptr;
    // frame records (records.h): at most one pool per handle, allocated by tstar_owl_records_reserve and freed with the handle
    float* rec_pool = nullptr;
    int rec_slots = 0;
    DeviceBuf<int> rec_idx;                                          // staging of one record call: miss slots [n_miss] | slots [B]
    DeviceBuf<int> rec_sets;                                         // ... and its image -> query set array
    DeviceBuf<int> ids, eos;                             // staging of one text forward: token ids [n][16], first-maximum positions [n]
    DeviceBuf<uint8_t> kmask;                            // ... key masks [n][16]; n = 32 from creation, what lane 0 holds after set_queries_many
    int reserve_text_staging(int nseq, hipStream_t s) {
        RC(ids.reserve((size_t)nseq * T_LEN, s));
        RC(eos.reserve((size_t)nseq, s));
        return kmask.reserve((size_t)nseq * T_LEN, s);
    }
    std::map<std::pair<int, int>, ResampleTable> tabs;   // (in_size, out_size) -> table (out_size: the handle's input width / height)
    std::map<std::pair<int, int>, Owlv2AxisTable> tabs_v2;   // OWLv2: (square side, out_size) -> zoom taps + Gaussian weights of one axis
    std::map<std::pair<int, int>, std::vector<double>> gw_v2;  // OWLv2: Gaussian weights installed by the caller (tstar_owlv2_set_axis_weights)
    // weights_mode 1 / 3 (BASELINE config 5, bf16 weights; two-term / exact three-term activations): bfloat16 copy of every
    // GEMM weight matrix (two-term mode, the N = 768 matrices: once more in MFMA-fragment order); weights_mode 4 (f32x3): every f32
    // matrix as three exact bf16 planes in MFMA-fragment order.  Empty in the f32 mode; freed with the handle.
    int weights_mode = TSTAR_WEIGHTS_F32;
    std::unordered_map<const float*, WeightPlanes> planes;           // f32 matrix -> its planes in gemm_wmode_of(weights_mode)
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

// a launch with the weight planes of the handle's weights_mode
static GemmArgs mk_gemm(const tstar_owl* h, const float* A, const float* W, float* C, const float* bias, const float* res,
                        int M, int N, int K, int lda, int ldc, int act) {
    GemmArgs g = gemm_args(A, W, C, bias, res, M, N, K, lda, ldc, act);
    const auto it = h->planes.find(W);
    return it == h->planes.end() ? g : with_planes(g, it->second);
}

// The text tower's GEMMs.  The query embeddings are computed once per query set and enter every score, so the two-term mode runs
// them with the exact three-term activation split on the same bf16 weight plane (what TSTAR_WEIGHTS_BF16_EXACT runs everywhere):
// float32-class embeddings of the rounded checkpoint.  The other modes are unchanged.
static GemmArgs mk_text_gemm(const tstar_owl* h, const float* A, const float* W, float* C, const float* bias, const float* res,
                             int M, int N, int K, int lda, int ldc, int act) {
    GemmArgs g = mk_gemm(h, A, W, C, bias, res, M, N, K, lda, ldc, act);
    if (g.wmode == GEMM_W_BF16_2T) { g.wmode = GEMM_W_BF16_EXACT; g.Wq = nullptr; }
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
    RC(L.minmax.reserve((size_t)B * 2, s));
    return owlv2_preprocess(d_images, out_patches, L.minmax.p, B, H, W, G.in_h, G.in_w, *ty, *tx, h->d_lut, s, &L.v2_form);
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
    RC(L.tmp_u8.reserve((size_t)B * H * G.in_w * 3, s));
    RC(resample_h_u8(d_images, L.tmp_u8.p, B, H, W, *th, s));
    RC(resample_v_normalize_patchify(L.tmp_u8.p, out_patches, out_u8, B, H, G.in_w, *tv, h->d_lut, G.patch, s));
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
    void* ptrs[] = {L.x, L.xn, L.qkv, L.att, L.hid};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    L.tmp_u8.release(); L.image_set.release(); L.minmax.release();
    L = tstar_owl::Lane{};
}

static const char* const NO_QUERIES = "no queries installed in the requested query set (call tstar_owl_set_queries first)";

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

static int build_all_weight_planes(tstar_owl* h, int mode) {
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
    static const bool w2v_off = getenv("TSTAR_W2V_OFF") != nullptr;   // same-session A/Bs: every layer on the LDS tile
    // the handle's policy: a fragment-packed two-term plane for the N = 768 matrices only (per-shape dispatch, gemm_f32.hip plan_gemm)
    for (auto& m : mats) RC(build_weight_planes(m.w, m.n, m.k, gemm_wmode_of(mode), m.n == 768 && !w2v_off, 0, &h->planes[m.w]));
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
    rc = h->reserve_text_staging(TSTAR_OWL_MAX_QUERIES, nullptr);
    if (rc) { tstar_owl_destroy(h); return rc; }
    if (weights_mode != TSTAR_WEIGHTS_F32) {
        rc = build_all_weight_planes(h, weights_mode);
        if (rc) { tstar_owl_destroy(h); return rc; }
    }
    *out = h;
    return TSTAR_OK;
}

int tstar_owl_destroy(tstar_owl* h) {
    if (!h) return TSTAR_OK;
    void* ptrs[] = {h->d_vision, h->d_text, h->d_lut, h->q_raw, h->qn, h->qweight, h->qmask, h->d_setQ, h->rec_pool};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    h->rec_idx.release(); h->rec_sets.release();
    h->ids.release(); h->eos.release(); h->kmask.release();
    for (auto& L : h->lane) free_lane(L);
    for (auto& kv : h->tabs) free_table(&kv.second);
    for (auto& kv : h->tabs_v2) free_owlv2_axis_table(&kv.second);
    delete h;                                                // the weight planes go with the map that owns them
    return TSTAR_OK;
}

// Installing a query set, the part that waits for nothing: q_raw[set] -> qn[set], the masks and weights, the slot's size on the host
static int enqueue_queries(tstar_owl* h, int set, const uint8_t* h_mask, const double* h_w, int Q, hipStream_t s) {
    const size_t qo = (size_t)set * TSTAR_OWL_MAX_QUERIES;
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3(Q), dim3(64), 0, s, h->q_raw + qo * PROJ, h->qn + qo * PROJ, 1e-6f);
    TSTAR_HIP_CHECK(hipGetLastError());
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->qmask + qo, h_mask, Q, hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->qweight + qo, h_w, Q * sizeof(double), hipMemcpyHostToDevice, s));
    h->Q[set] = Q;
    return TSTAR_OK;
}
// ... and the end of the call: the slot sizes go to the device, the stream is drained (the arrays enqueued above are the caller's)
static int commit_queries(tstar_owl* h, hipStream_t s) {
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->d_setQ, h->Q, sizeof(h->Q), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

// Host staging of the text forwards of one call; lives until the stream has been synchronised (the copies below are asynchronous)
struct TextStage {
    std::vector<int> eos;
    std::vector<uint8_t> km, qm;
    // n sequences of entry `fn`: every token id in range, the first-maximum position, the key mask and the query mask of each
    int fill(const char* fn, const int32_t* h_ids, const int32_t* h_am, int n) {
        eos.resize(n); km.resize((size_t)n * T_LEN); qm.resize(n);
        for (int q = 0; q < n; ++q) {
            const int32_t *ids = h_ids + (size_t)q * T_LEN, *am = h_am + (size_t)q * T_LEN;
            int best = 0;
            for (int t = 0; t < T_LEN; ++t) {
                TSTAR_REQUIRE(ids[t] >= 0 && ids[t] < T_VOCAB, std::string(fn) + ": token id out of range");
                if (ids[t] > ids[best]) best = t;                  // argmax, first occurrence
                km[(size_t)q * T_LEN + t] = am[t] != 0;
            }
            eos[q] = best;
            qm[q] = ids[0] > 0;                                    // modeling_owlvit.py:1447
        }
        return TSTAR_OK;
    }
};

// The text tower on sequences [q0, q0 + nseq) of a filled stage, in lane 0 (the handle's own workspace): token + position embedding
// -> L.x [nseq*16, 512]; with pooled != 0 also the 12 layers, the final LayerNorm and the row of every sequence's first maximum id
// -> L.att [nseq, 512].  Every GEMM tile shape and the per-sequence causal attention give a sequence the same bits in any batch.
static int text_forward(tstar_owl* h, const int32_t* h_ids, const TextStage& st, int q0, int nseq, int pooled, hipStream_t s) {
    auto& L = h->lane[0];
    const int M = nseq * T_LEN;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->ids.p, h_ids + (size_t)q0 * T_LEN, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->eos.p, st.eos.data() + q0, nseq * sizeof(int), hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->kmask.p, st.km.data() + (size_t)q0 * T_LEN, M, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(embed_tokens_kernel, dim3(M), dim3(128), 0, s, h->ids.p, h->tw.tok_emb, h->tw.tpos_emb, L.x, T_LEN, T_D);
    TSTAR_HIP_CHECK(hipGetLastError());
    if (!pooled) return TSTAR_OK;
    RC(run_encoder(h, L, h->tw.layers, T_LAYERS, nseq, T_LEN, T_D, T_FF, T_HEADS, 1, h->kmask.p, s));
    RC(layernorm_f32(L.x, L.xn, h->tw.final_ln_w, h->tw.final_ln_b, M, T_D, s));
    hipLaunchKernelGGL(gather_rows_kernel, dim3(nseq), dim3(128), 0, s, L.xn, h->eos.p, L.att, T_LEN, T_D);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

// the pooled rows L.att [nseq, 512] through text_projection -> L.hid [nseq, 512]
static int text_project(tstar_owl* h, int nseq, hipStream_t s) {
    auto& L = h->lane[0];
    return gemm_f32(mk_text_gemm(h, L.att, h->tw.text_proj, L.hid, nullptr, nullptr, nseq, PROJ, T_D, T_D, PROJ, ACT_NONE), s);
}

// rows [off, off + Q) of L.hid, each over its norm -> q_raw[set] (what tstar_owl_get_query_embeds returns)
static int normalise_into_set(tstar_owl* h, int off, int set, int Q, hipStream_t s) {
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3(Q), dim3(64), 0, s, h->lane[0].hid + (size_t)off * PROJ,
                       h->q_raw + (size_t)set * TSTAR_OWL_MAX_QUERIES * PROJ, 0.0f);
    TSTAR_HIP_CHECK(hipGetLastError());
    return TSTAR_OK;
}

int tstar_owl_set_queries(tstar_owl* h, int query_set, const int32_t* h_ids, const int32_t* h_am, const double* h_w, int Q,
                          void* stream) {
    TSTAR_REQUIRE(h && h_ids && h_am && h_w, "tstar_owl_set_queries: null argument");
    TSTAR_CHECK_SET(query_set, "tstar_owl_set_queries");
    TSTAR_REQUIRE(Q >= 1 && Q <= TSTAR_OWL_MAX_QUERIES, "tstar_owl_set_queries: Q must be in 1..32");
    if (!h->has_text) { set_error("tstar_owl_set_queries: handle was created without text weights"); return TSTAR_ERR_STATE; }
    hipStream_t s = (hipStream_t)stream;
    TextStage st;
    RC(st.fill("tstar_owl_set_queries", h_ids, h_am, Q));
    RC(text_forward(h, h_ids, st, 0, Q, 1, s));
    RC(text_project(h, Q, s));
    RC(normalise_into_set(h, 0, query_set, Q, s));
    RC(enqueue_queries(h, query_set, st.qm.data(), h_w, Q, s));
    return commit_queries(h, s);
}

int tstar_owl_debug_text(tstar_owl* h, const int32_t* h_ids, const int32_t* h_am, int Q, int stage, float* h_out, void* stream) {
    TSTAR_REQUIRE(h && h_ids && h_am && h_out, "tstar_owl_debug_text: null argument");
    TSTAR_REQUIRE(Q >= 1 && Q <= TSTAR_OWL_MAX_QUERIES, "tstar_owl_debug_text: Q must be in 1..32");
    TSTAR_REQUIRE(stage == 0 || stage == 1, "tstar_owl_debug_text: stage must be 0 (embedding rows) or 1 (pooled rows)");
    if (!h->has_text) { set_error("tstar_owl_debug_text: handle was created without text weights"); return TSTAR_ERR_STATE; }
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[0];
    TextStage st;
    RC(st.fill("tstar_owl_debug_text", h_ids, h_am, Q));
    RC(text_forward(h, h_ids, st, 0, Q, stage, s));
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
    int total = 0;
    for (int i = 0; i < n_sets; ++i) {
        TSTAR_CHECK_SET(h_sets[i], "tstar_owl_set_queries_many");
        TSTAR_REQUIRE(h_Q[i] >= 1 && h_Q[i] <= TSTAR_OWL_MAX_QUERIES, "tstar_owl_set_queries_many: every Q must be in 1..32");
        total += h_Q[i];
    }
    TextStage st;
    RC(st.fill("tstar_owl_set_queries_many", h_ids, h_am, total));
    // sequences per text forward: what the activation workspace holds (mpad rows of >= T_D floats; T_LEN rows per sequence)
    const int cap = (int)(h->mpad / T_LEN);
    TSTAR_REQUIRE(cap >= TSTAR_OWL_MAX_QUERIES, "tstar_owl_set_queries_many: workspace too small");
    RC(h->reserve_text_staging(cap, s));
    // ONE text forward per group of sets that fits the workspace: results equal one-by-one calls
    for (int i0 = 0, q0 = 0; i0 < n_sets;) {
        int i1 = i0, nseq = 0;
        while (i1 < n_sets && nseq + h_Q[i1] <= cap) nseq += h_Q[i1++];
        RC(text_forward(h, h_ids, st, q0, nseq, 1, s));
        RC(text_project(h, nseq, s));
        for (int off = 0; i0 < i1; ++i0) {
            RC(normalise_into_set(h, off, h_sets[i0], h_Q[i0], s));
            RC(enqueue_queries(h, h_sets[i0], st.qm.data() + q0 + off, h_w + q0 + off, h_Q[i0], s));
            off += h_Q[i0];
        }
        // the staging buffers are reused by the next group: wait for this one
        TSTAR_HIP_CHECK(hipStreamSynchronize(s));
        q0 += nseq;
    }
    return commit_queries(h, s);
}

int tstar_owl_set_query_embeds(tstar_owl* h, int query_set, const float* h_qe, const uint8_t* h_mask, const double* h_w,
                               int Q, void* stream) {
    TSTAR_REQUIRE(h && h_qe && h_mask && h_w, "tstar_owl_set_query_embeds: null argument");
    TSTAR_CHECK_SET(query_set, "tstar_owl_set_query_embeds");
    TSTAR_REQUIRE(Q >= 1 && Q <= TSTAR_OWL_MAX_QUERIES, "tstar_owl_set_query_embeds: Q must be in 1..32");
    hipStream_t s = (hipStream_t)stream;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->q_raw + (size_t)query_set * TSTAR_OWL_MAX_QUERIES * PROJ, h_qe,
                                   (size_t)Q * PROJ * sizeof(float), hipMemcpyHostToDevice, s));
    RC(enqueue_queries(h, query_set, h_mask, h_w, Q, s));
    return commit_queries(h, s);
}

int tstar_owl_set_class_weights(tstar_owl* h, int query_set, const double* h_w, int Q, void* stream) {
    TSTAR_REQUIRE(h && h_w, "tstar_owl_set_class_weights: null argument");
    TSTAR_CHECK_SET(query_set, "tstar_owl_set_class_weights");
    TSTAR_REQUIRE(Q == h->Q[query_set] && Q >= 1, "tstar_owl_set_class_weights: Q does not match the installed queries");
    hipStream_t s = (hipStream_t)stream;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h->qweight + (size_t)query_set * TSTAR_OWL_MAX_QUERIES, h_w, Q * sizeof(double),
                                   hipMemcpyHostToDevice, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

int tstar_owl_get_query_embeds(tstar_owl* h, int query_set, float* h_out, int Q, void* stream) {
    TSTAR_REQUIRE(h && h_out, "tstar_owl_get_query_embeds: null argument");
    TSTAR_CHECK_SET(query_set, "tstar_owl_get_query_embeds");
    TSTAR_REQUIRE(Q == h->Q[query_set], "tstar_owl_get_query_embeds: Q does not match the installed queries");
    hipStream_t s = (hipStream_t)stream;
    TSTAR_HIP_CHECK(hipMemcpyAsync(h_out, h->q_raw + (size_t)query_set * TSTAR_OWL_MAX_QUERIES * PROJ,
                                   (size_t)Q * PROJ * sizeof(float), hipMemcpyDeviceToHost, s));
    TSTAR_HIP_CHECK(hipStreamSynchronize(s));
    return TSTAR_OK;
}

// lane 1: allocated on first use (a one-off, like the resample tables) for forward chunks of min(max_batch, max(TSTAR_OWL_AUX_BATCH, B))
// images, and grown when a larger batch arrives (the device is drained first); lane 0 is the handle's own
static int ensure_lane(tstar_owl* h, int lane, int B) {
    auto& L = h->lane[lane];
    if (lane == 0) return TSTAR_OK;
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
    RC(ensure_lane(h, lane, B));
    int q_uniform = -1;                                   // the common Q when every image uses one set size
    RC(check_query_sets("tstar_owl_score", NO_QUERIES, h->Q, h_image_query_set, B, L.image_set, s, &q_uniform));
    TSTAR_REQUIRE(!d_logits || q_uniform > 0, "tstar_owl_score: raw logits need the same query count for every image");
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
        a.image_set = h_image_query_set ? L.image_set.p + b0 : nullptr;
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

// ---- frame records
size_t tstar_owl_records_frame_bytes(int family, int input_h, int input_w, int patch_size) {
    OwlGeom g;
    if (!owl_geom_family(family, input_h, input_w, patch_size, &g)) {
        set_error("tstar_owl_records_frame_bytes: unsupported family / input size (family 0: patch 32 or 16; family 1 (OWLv2): patch 16; each "
                  "side a positive multiple of the patch size; at most 3600 patches)");
        return 0;
    }
    return (size_t)g.np * RECORD_FLOATS_PER_PATCH * sizeof(float);
}

int tstar_owl_records_reserve(tstar_owl* h, int n_slots) {
    TSTAR_REQUIRE(h && n_slots >= 1, "tstar_owl_records_reserve: null handle or n_slots < 1");
    if (!h->has_vision) { set_error("tstar_owl_records_reserve: handle was created without vision weights (text-only)"); return TSTAR_ERR_STATE; }
    if (h->rec_pool) {
        if (n_slots == h->rec_slots) return TSTAR_OK;
        set_error("tstar_owl_records_reserve: the handle already holds a pool of " + std::to_string(h->rec_slots) + " records; it lives as long as the handle");
        return TSTAR_ERR_STATE;
    }
    const size_t bytes = (size_t)n_slots * record_stride_floats(h->geom.np) * sizeof(float);
    hipError_t e = hipMalloc(&h->rec_pool, bytes);
    if (e == hipSuccess) e = hipMemset(h->rec_pool, 0, bytes);          // a record never filled scores as zeros, not as whatever was there
    if (e == hipSuccess) e = hipDeviceSynchronize();                    // the zero fill ran on the null stream
    if (e != hipSuccess) {
        if (h->rec_pool) (void)hipFree(h->rec_pool);
        h->rec_pool = nullptr;
        set_error("tstar_owl_records_reserve: allocating " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
        return TSTAR_ERR_HIP;
    }
    h->rec_slots = n_slots;
    return TSTAR_OK;
}

int tstar_owl_records_slots(tstar_owl* h) {
    if (!h) { set_error("tstar_owl_records_slots: null handle"); return -1; }
    return h->rec_slots;
}

int tstar_owl_score_records(tstar_owl* h, int lane, const uint8_t* d_miss_images, int n_miss, int H, int W, const int32_t* h_miss_slots, int B,
                            const int32_t* h_slots, const int32_t* h_image_query_set, int box_w, int box_h, float* d_scores, int32_t* d_labels,
                            double* d_cell_conf, uint32_t* d_cell_mask, int32_t* d_n_kept, float* d_logits, float* d_objectness,
                            float* d_boxes_xyxy, float* d_boxes_cxcywh, void* stream) {
    const std::string fn = "tstar_owl_score_records";
    // every refusal comes before the first launch or copy
    TSTAR_REQUIRE(h, fn + ": null handle");
    TSTAR_REQUIRE(lane >= 0 && lane < TSTAR_OWL_LANES, fn + ": lane must be 0 or 1");
    TSTAR_REQUIRE(n_miss >= 0 && B >= 0 && n_miss + B >= 1 && B <= 65535, fn + ": n_miss and B must not be negative, one of them at least 1 (B at most 65535)");
    TSTAR_REQUIRE(h->rec_pool, fn + ": the handle holds no records (call tstar_owl_records_reserve first)");
    TSTAR_REQUIRE(!d_objectness, fn + ": OWLv2's objectness is not recorded (d_objectness must be NULL)");
    TSTAR_REQUIRE(n_miss == 0 || (d_miss_images && h_miss_slots && H >= 1 && W >= 1), fn + ": missing images need d_miss_images, h_miss_slots and their size");
    TSTAR_REQUIRE(B == 0 || (h_slots && d_scores && d_labels && d_cell_conf && d_cell_mask && box_w >= 1 && box_h >= 1),
                  fn + ": scored images need h_slots, d_scores, d_labels, d_cell_conf, d_cell_mask and the size the boxes are scaled to");
    {
        std::vector<char> seen(h->rec_slots, 0);
        for (int i = 0; i < n_miss; ++i) {
            TSTAR_REQUIRE(h_miss_slots[i] >= 0 && h_miss_slots[i] < h->rec_slots, fn + ": a slot of h_miss_slots is outside the pool");
            TSTAR_REQUIRE(!seen[h_miss_slots[i]], fn + ": h_miss_slots names a slot twice");
            seen[h_miss_slots[i]] = 1;
        }
        for (int b = 0; b < B; ++b) TSTAR_REQUIRE(h_slots[b] >= 0 && h_slots[b] < h->rec_slots, fn + ": a slot of h_slots is outside the pool");
    }
    if (n_miss > 0 && h->geom.family == TSTAR_OWL_FAMILY_OWLV2) {
        const Owlv2Plan vp = plan_owlv2_preprocess(H, W, h->geom.in_h, h->geom.in_w);
        if (vp.error) { set_error(vp.error); return TSTAR_ERR_ARG; }
    }
    for (int b = 0; b < B; ++b) {
        const int set = h_image_query_set ? h_image_query_set[b] : 0;
        TSTAR_CHECK_SET(set, fn);
        if (h->Q[set] == 0) { set_error(fn + ": " + NO_QUERIES); return TSTAR_ERR_ARG; }
    }
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[lane];
    if (n_miss > 0) RC(ensure_lane(h, lane, n_miss));
    int q_uniform = -1;
    if (B > 0) RC(check_query_sets(fn, NO_QUERIES, h->Q, h_image_query_set, B, h->rec_sets, s, &q_uniform));
    TSTAR_REQUIRE(!d_logits || q_uniform > 0, fn + ": raw logits need the same query count for every image");
    RC(h->rec_idx.reserve((size_t)n_miss + B, s));
    if (n_miss > 0) TSTAR_HIP_CHECK(hipMemcpyAsync(h->rec_idx.p, h_miss_slots, (size_t)n_miss * sizeof(int), hipMemcpyHostToDevice, s));
    if (B > 0) TSTAR_HIP_CHECK(hipMemcpyAsync(h->rec_idx.p + n_miss, h_slots, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    const OwlGeom& G = h->geom;
    const int NP = G.np;
    const size_t stride = record_stride_floats(NP);
    // 1. the missing images through the lane's usual forward chunks, each chunk's rows into the records named for its images
    for (int b0 = 0; b0 < n_miss; b0 += L.cap) {
        const int Bc = (n_miss - b0) < L.cap ? (n_miss - b0) : L.cap;
        OwlHeadTensors t;
        RC(owl_forward_heads(h, L, d_miss_images + (size_t)b0 * H * W * 3, Bc, H, W, true, &t, s));
        RecordFillArgs f{};
        f.feats = t.feats; f.cls = t.cls; f.boxh = t.bh2;
        f.shift_w = h->vw.shift_w; f.shift_b = h->vw.shift_b; f.scale_w = h->vw.scale_w; f.scale_b = h->vw.scale_b;
        f.box2_w = h->vw.box2_w; f.box2_b = h->vw.box2_b; f.box_bias = h->vw.box_bias;
        f.slots = h->rec_idx.p + b0; f.pool = h->rec_pool; f.stride = stride; f.n = Bc; f.np = NP;
        RC(record_fill(f, s));
    }
    if (B == 0) return TSTAR_OK;
    // 2. all B images from records, hits and fresh misses alike: there is no second path that scores a forward directly
    ScoreRecordsArgs a{};
    a.pool = h->rec_pool; a.stride = stride; a.slots = h->rec_idx.p + n_miss;
    a.image_set = h_image_query_set ? h->rec_sets.p : nullptr;
    a.qn = h->qn; a.qmask = h->qmask; a.setQ = h->d_setQ;
    a.scores = d_scores; a.labels = d_labels; a.logits = d_logits; a.xyxy = d_boxes_xyxy; a.cxcywh = d_boxes_cxcywh;
    a.B = B; a.np = NP; a.Q = q_uniform;
    box_scale(G, box_h, box_w, &a.box_sx, &a.box_sy);
    RC(score_records(a, s));
    // one cell: every kept detection falls in cell 0, where its clamped box centre puts it in tstar_owl_score too
    return cell_reduce(d_scores, d_labels, nullptr, h->qweight, a.image_set, B, NP, box_w, box_h, 1, 1, 0.005f, d_cell_conf, d_cell_mask, d_n_kept, s);
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
    RC(check_query_sets("tstar_owl_score", NO_QUERIES, h->Q, h_image_query_set, B, L.image_set, s, &q_uniform));
    TSTAR_REQUIRE(!d_logits || q_uniform > 0, "tstar_owl_debug_heads: raw logits need the same query count for every image");
    const int NP = h->geom.np;
    DetectRowsArgs a = detect_args(h);
    a.feats = d_feats; a.cls = d_cls; a.boxh = d_boxh;
    a.scores = d_scores; a.labels = d_labels; a.xyxy = d_boxes_xyxy; a.logits = d_logits; a.cxcywh = d_boxes_cxcywh;
    a.image_set = h_image_query_set ? L.image_set.p : nullptr;
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

// fn: the entry's name in messages
static int embed_image_queries_entry(const std::string& fn, tstar_owl* h, const uint8_t* d_images, int n, int H, int W, const float* h_query_boxes,
                                     float* h_embeds, int32_t* h_best, float* h_boxes_cxcywh, int32_t* h_n_selected, int32_t* h_status, void* stream) {
    TSTAR_REQUIRE(h && d_images && h_embeds && h_best && h_boxes_cxcywh && h_n_selected && h_status, fn + ": null argument");
    TSTAR_REQUIRE(n >= 1 && n <= 65535 && H >= 1 && W >= 1, fn + ": empty batch or image (n in 1..65535)");
    if (!h->has_vision) { set_error(fn + ": handle was created without vision weights (text-only)"); return TSTAR_ERR_STATE; }
    if (h->geom.family == TSTAR_OWL_FAMILY_OWLV2) {          // refusals before anything is launched
        const Owlv2Plan vp = plan_owlv2_preprocess(H, W, h->geom.in_h, h->geom.in_w);
        if (vp.error) { set_error(vp.error); return TSTAR_ERR_ARG; }
    }
    hipStream_t s = (hipStream_t)stream;
    auto& L = h->lane[0];                                     // the handle's own workspace, as the text tower
    const int NP = h->geom.np;
    void* d_buf = nullptr;
    // the staging allocation: the outputs, then (with query boxes) the boxes [n, 4]
    TSTAR_HIP_CHECK(hipMalloc(&d_buf, image_query_out_bytes(n) + (h_query_boxes ? (size_t)n * 4 * sizeof(float) : 0)));
    const ImageQueryOut o = image_query_out_at(d_buf, n);
    float* d_qboxes = h_query_boxes ? reinterpret_cast<float*>(static_cast<char*>(d_buf) + image_query_out_bytes(n)) : nullptr;
    int rc = TSTAR_OK;
    if (d_qboxes) {
        const hipError_t e = hipMemcpyAsync(d_qboxes, h_query_boxes, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { set_error(fn + ": " + hipGetErrorString(e)); rc = TSTAR_ERR_HIP; }
    }
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
        if (!rc) rc = image_query_select(t.cls, a.cxcywh, d_qboxes ? d_qboxes + (size_t)b0 * 4 : nullptr, Bc, NP, image_query_out_offset(o, b0), s);
    }
    return image_query_finish(fn.c_str(), rc, d_buf, o, n, h_embeds, h_best, h_boxes_cxcywh, h_n_selected, h_status, s);
}

int tstar_owl_embed_image_queries(tstar_owl* h, const uint8_t* d_images, int n, int H, int W, float* h_embeds, int32_t* h_best, float* h_boxes_cxcywh,
                                  int32_t* h_n_selected, int32_t* h_status, void* stream) {
    return embed_image_queries_entry("tstar_owl_embed_image_queries", h, d_images, n, H, W, nullptr, h_embeds, h_best, h_boxes_cxcywh, h_n_selected,
                                     h_status, stream);
}

int tstar_owl_embed_image_queries_box(tstar_owl* h, const uint8_t* d_images, int n, int H, int W, const float* h_query_boxes, float* h_embeds,
                                      int32_t* h_best, float* h_boxes_cxcywh, int32_t* h_n_selected, int32_t* h_status, void* stream) {
    return embed_image_queries_entry("tstar_owl_embed_image_queries_box", h, d_images, n, H, W, h_query_boxes, h_embeds, h_best, h_boxes_cxcywh,
                                     h_n_selected, h_status, stream);
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

}  // extern "C"
