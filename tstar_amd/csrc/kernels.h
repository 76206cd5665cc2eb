// Internal launcher declarations (not part of the C ABI; see include/tstar_hip.h).
#pragma once
#include "../../include/tstar_hip.h"
#include "common.h"
#include <utility>

namespace tstar {

enum { ACT_NONE = 0, ACT_QGELU = 1, ACT_GELU = 2 };

struct GemmArgs {
    const float* A;      // [M, lda] row-major, K contiguous
    const float* W;      // [N, K] row-major (nn.Linear layout)
    const __bf16* Wb;    // bfloat16 copy of W: what GEMM_W_BF16_EXACT and GEMM_W_BF16_2T read
    const void* Wp;      // fragment-packed three-plane copy of W (pack_weights_x3): what GEMM_W_F32X3 reads
    const void* Wq;      // optional fragment-packed copy of Wb (pack_weights_w2): the two-term mode's wide tile may stream its weights global -> VGPR
    float* C;            // [*, ldc]
    const float* bias;   // [N] or null
    const float* res;    // residual, same layout as C, or null (may alias C)
    const float* pos;    // patch-embed epilogue: position embedding [np+1, N], or null
    int M, N, K, lda, ldc;
    int act;             // ACT_*
    int patch_np;        // patches per image (576) for the patch-embed epilogue
    int tile_cfg;        // a GemmTileCfg value (below); crosses the C ABI as int
    int m_split;         // hybrid launch: rows [0, m_split) use 128-row tiles (set by the launcher)
    int group_m;         // row panels per super-panel of the tile order (gemm_f32.hip tile_mn); 0 = the library's default
    int wmode;           // a GemmWeightMode (below): the arithmetic of the launch; the plane it reads must be set (with_planes)
};
int gemm_f32(const GemmArgs& g, hipStream_t stream);

// GemmArgs::tile_cfg.  The numbers are fixed: the diagnostic C entry points, the tests and tools/sweep_*.py pass them as int.
enum GemmTileCfg {
    TILE_AUTO = -1,       // the launcher's choice (plan_gemm)
    TILE_128 = 0,         // pure grid of 128x128 block tiles
    TILE_64N = 1,         // pure grid of 64x128 block tiles
    TILE_64 = 2,          // pure grid of 64x64 block tiles
    TILE_HYBRID = 3,      // 128x128 tiles on the first half of the row tiles + 64x128 tail
    TILE_WIDE = 4,        // two-term bf16 / f32x3 modes: the 128x256 tile forced on every full 128-row panel
    TILE_NO_WIDE = 5,     // two-term bf16 / f32x3 modes: the 128x256 tile forced off
    TILE_WIDE_VW = 6,     // two-term bf16 mode: the 128x256 tile with weights global -> VGPR forced on every full panel
    TILE_HYBRID_N = 16,   // 16 + n: hybrid with n big row tiles (diagnostic, tile-policy sweeps)
};

// How a launch reads its weights; the values are the WMODE template argument of the kernels.
enum GemmWeightMode {
    GEMM_W_F32 = 0,       // native f32 MFMA
    GEMM_W_BF16_EXACT = 1,// bf16 weights, activations split exactly into three bf16 terms
    GEMM_W_BF16_2T = 3,   // bf16 weights, activations as two round-to-nearest bf16 terms (2 MFMA products per algorithmic product)
    GEMM_W_F32X3 = 4,     // fragment-packed three-plane weights, six products
};

// the GEMM mode of a TSTAR_WEIGHTS_* value of the C ABI; -1: not one
static inline int gemm_wmode_of(int weights_mode) {
    return weights_mode == TSTAR_WEIGHTS_F32 ? GEMM_W_F32 : weights_mode == TSTAR_WEIGHTS_BF16 ? GEMM_W_BF16_2T :
           weights_mode == TSTAR_WEIGHTS_BF16_EXACT ? GEMM_W_BF16_EXACT : weights_mode == TSTAR_WEIGHTS_F32X3 ? GEMM_W_F32X3 : -1;
}

// a launch on the f32 matrix alone: no converted weight plane, no patch epilogue, the launcher's tile choice
static inline GemmArgs gemm_args(const float* A, const float* W, float* C, const float* bias, const float* res, int M, int N, int K, int lda, int ldc,
                                 int act) {
    GemmArgs g{};
    g.A = A; g.W = W; g.C = C; g.bias = bias; g.res = res;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc; g.act = act; g.tile_cfg = TILE_AUTO; g.wmode = GEMM_W_F32;
    return g;
}

enum GemmKind {
    GEMM_GRID_128 = 0,    // pure grid of 128x128 tiles
    GEMM_GRID_64N = 1,    // pure grid of 64x128 tiles
    GEMM_GRID_64 = 2,     // pure grid of 64x64 tiles
    GEMM_HYBRID = 3,      // rows [0, m_split) in 128x128 tiles, the rest in 64x128 tiles
    GEMM_WIDE = 4,        // rows [0, m_split) in 128x256 tiles, the rest in 64x128 tiles
    GEMM_WIDE_VW = 5,     // the same with the wide tiles' weights streamed global -> VGPR (needs GemmArgs::Wq)
};

// What one launch does.  error != null: the arguments are refused (TSTAR_ERR_ARG) and the other fields mean nothing.
struct GemmPlan {
    int kind;             // GemmKind
    int m_split;          // GemmArgs::m_split of the launch (0 for a pure grid)
    int blocks;           // grid size
    int lds_bytes;        // dynamic LDS per block
    const char* error;
};

// The tile policy: pure integer arithmetic, no HIP call, no global state (tests/test_host_logic.py pins it on a host without a GPU).
// has_wq: a fragment-packed two-term plane (GemmArgs::Wq) exists.
GemmPlan plan_gemm(int wmode, int M, int N, int ldc, int patch_np, int tile_cfg, bool has_wq);

// Wb[i] = bfloat16(W[i]) (round to nearest even); n elements.  With Wlo != null also Wlo[i] = bfloat16(W[i] - Wb[i]).
int convert_f32_to_bf16(const float* W, __bf16* Wb, __bf16* Wlo, size_t n, hipStream_t s);

// two-term mode: Wb [N, K] bf16 -> the same values in MFMA-fragment order, 2 * N * K bytes (gemm_f32.hip)
int pack_weights_w2(const __bf16* Wb, void* Wq, int N, int K, hipStream_t s);
// THE shape rule of a Wq plane: the VGPR-weight wide tile covers 256 columns and a K tile is 32.  Whether a caller wants one is its own policy.
static inline bool w2_plane_shape_ok(int N, int K) { return N % 256 == 0 && K % 32 == 0; }

// f32x3 mode: W [N, K] f32 -> three exact bf16 planes in MFMA-fragment order, 6 * N * K bytes (gemm_f32.hip)
int pack_weights_x3(const float* W, void* Wp, int N, int K, hipStream_t s);

// The converted planes of ONE [N, K] weight matrix in ONE GemmWeightMode.  Owns them: move-only, freed by the destructor (hipFree
// waits for the launches that still read them).
struct WeightPlanes {
    __bf16* Wb = nullptr;          // GEMM_W_BF16_EXACT, GEMM_W_BF16_2T
    void* Wq = nullptr;            // GEMM_W_BF16_2T, where asked for and w2_plane_shape_ok
    void* Wp = nullptr;            // GEMM_W_F32X3
    int wmode = GEMM_W_F32, N = 0, K = 0;
    WeightPlanes() = default;
    WeightPlanes(WeightPlanes&& o) noexcept { swap(o); }              // (a declared move: no copy)
    WeightPlanes& operator=(WeightPlanes&& o) noexcept { swap(o); return *this; }
    ~WeightPlanes() { (void)hipFree(Wb); (void)hipFree(Wq); (void)hipFree(Wp); }
    void swap(WeightPlanes& o) { std::swap(Wb, o.Wb); std::swap(Wq, o.Wq); std::swap(Wp, o.Wp); std::swap(wmode, o.wmode); std::swap(N, o.N); std::swap(K, o.K); }
};

// The one builder (gemm_f32.hip): GEMM_W_F32 nothing; GEMM_W_BF16_EXACT Wb; GEMM_W_BF16_2T Wb, and Wq when want_w2_packed and
// w2_plane_shape_ok; GEMM_W_F32X3 Wp.  Enqueues on s and does not wait.  On any failure *out is empty and nothing is leaked.
int build_weight_planes(const float* d_W, int N, int K, int wmode, bool want_w2_packed, hipStream_t s, WeightPlanes* out);

// a launch in the mode of p, on its planes
static inline GemmArgs with_planes(GemmArgs g, const WeightPlanes& p) {
    g.wmode = p.wmode; g.Wb = p.Wb; g.Wq = p.Wq; g.Wp = p.Wp;
    return g;
}

// y[r,:] = LayerNorm(x[r,:]) * w + b over D (eps 1e-5, biased variance); D % 256 == 0, D <= 1024
int layernorm_f32(const float* x, float* y, const float* w, const float* b, int rows, int D, hipStream_t s);

// x[b,0,:] = cls + pos[0] (token row 0 of every image); x is [B*ntok, D]
int write_cls_rows(float* x, const float* cls, const float* pos, int B, int ntok, int D, hipStream_t s);

// feats[b,p,:] = LN_det( LN_post(x[b,1+p,:]) * LN_post(x[b,0,:]) )
int merge_cls_ln(const float* x, float* feats, const float* post_w, const float* post_b,
                 const float* det_w, const float* det_b, int B, int ntok, int D, hipStream_t s);

// multi-head self-attention over packed qkv [B*T, 3*D] (q | k | v, heads of 64) -> out [B*T, D]
// mode 0: full attention; mode 1: causal + key padding mask (key_mask [B,T] u8, 0 = masked)
int attention_f32(const float* qkv, float* out, int B, int T, int heads, int mode,
                  const uint8_t* key_mask, hipStream_t s);

// the same (mode 0 only) on the bf16 matrix pipe: every f32 operand as two bf16 terms, 3 products per MFMA step
int attention_split(const float* qkv, float* out, int B, int T, int heads, hipStream_t s);

// the same (mode 0 only) with EXACT operands: every f32 operand as three bf16 terms, six products per MFMA step (the f32x3 mode)
// order: block id -> (image, head, query tile).  1 = the query tiles of an (image, head) back to back on one XCD (xcd_remap_groups),
// 0 = linear, -1 = the library's choice (1 unless TSTAR_AX3_XCD_OFF is set).  Every block computes the same tile either way: same bits.
int attention_x3(const float* qkv, float* out, int B, int T, int heads, hipStream_t s, int order = -1);

}  // namespace tstar
