// The YOLO-World layer program (tstar_yolo_create, include/tstar_hip.h): its word layout, its typed form, and the one
// function that checks a program and decodes it.  HIP-free and header-only: it compiles under hipcc (yolo.hip, yolo_conv.hip)
// and as plain C++17 (the stand-alone checker yolo_program_check_main.cpp).  tstar_amd/yolo_world.py mirrors the word
// positions (W_* there) and packs the table this file reads.
//
// Every op is OP_WORDS int32 words; unused words are 0.  Word W_KIND selects the op:
//   OP_CONV    src, src_off, cin, dst, dst_off, cout, ks, stride, act, w_off, b_off, mode, aux, aux_off
//              k x k / stride conv (pad k / 2) of channels [src_off, src_off + cin) of buffer src into channels
//              [dst_off, dst_off + cout) of buffer dst; weights [cout][ks][ks][cin] at blob offset w_off, bias [cout] at
//              b_off (< 0: none); act YACT_*; mode MODE_*: the residual is read at channel aux_off of buffer aux, the
//              gate is buffer aux itself ([.., heads], aux_off 0)
//   OP_POOL5   buf, src_off, C, buf, dst_off             5 x 5 / stride 1 max pool inside one buffer (SPPF)
//   OP_UPCOPY  src, src_off, C, dst, dst_off, factor     channel-offset copy (factor 1) or nearest x2 upsample (2)
//   OP_ATTN    src, src_off, embed, dst, 0, heads, guide max-sigmoid gate of attention layer `guide`, one row of heads per
//                                                        source pixel into buffer dst
// All sums and products of words are formed in 64 bits: the words come from outside the library.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/tstar_hip.h"

namespace tstar {

constexpr int OP_WORDS = 24;
enum { OP_CONV = 0, OP_POOL5 = 1, OP_UPCOPY = 2, OP_ATTN = 3 };
enum { YACT_NONE = 0, YACT_SILU = 1 };
enum { MODE_PLAIN = 0, MODE_RESIDUAL = 1, MODE_ATTN_MUL = 2 };
// word positions; the last line names what words 3, 6 and 7 hold in the pool, up-copy and attention ops
enum {
    W_KIND = 0, W_SRC = 1, W_SRC_OFF = 2, W_CIN = 3, W_DST = 4, W_DST_OFF = 5, W_COUT = 6, W_KS = 7, W_STRIDE = 8, W_ACT = 9,
    W_W_OFF = 10, W_B_OFF = 11, W_MODE = 12, W_AUX = 13, W_AUX_OFF = 14,
    W_C = 3, W_EMBED = 3, W_FACTOR = 6, W_HEADS = 6, W_GUIDE = 7
};
// the rows of the other three tables
enum { BUF_H = 0, BUF_W = 1, BUF_C = 2, BUF_WORDS = 3 };
enum { GUIDE_EMBED = 0, GUIDE_HEADS = 1, GUIDE_W_OFF = 2, GUIDE_B_OFF = 3, GUIDE_BIAS_OFF = 4, GUIDE_WORDS = 5 };
enum { LEVEL_E_BUF = 0, LEVEL_R_BUF = 1, LEVEL_SIZE = 2, LEVEL_STRIDE = 3, LEVEL_PARAM_OFF = 4, LEVEL_WORDS = 8 };   // words 5 .. 7 are 0

constexpr int YOLO_IMG = 640;
constexpr int YOLO_REG_MAX = 16;
constexpr int YOLO_TEXT = 512;
constexpr int YOLO_MAX_Q = TSTAR_OWL_MAX_QUERIES;
constexpr size_t YOLO_GUIDE_LDS_BYTES = 96 * 1024;           // attn_kernel stages [YOLO_MAX_Q][embed] floats

// shared with the conv kernels (yolo_conv.hip)
constexpr int CBK = 16;                                      // input channels per K slice of the tiled forms
constexpr int DCH = 16;                                      // output channels per lane of the direct form
constexpr int DIRECT_MAX_GROUPS = 256;                       // ... whose cout / DCH channel groups share one 256-thread block
constexpr size_t DIRECT_LDS_BYTES = 64 * 1024;               // ... and whose whole weight matrix sits in LDS

struct YoloBuf { int H, W, C; };
struct YoloConvOp { int src, src_off, cin, dst, dst_off, cout, ks, stride, act, w_off, b_off, mode, aux, aux_off; };
struct YoloPoolOp { int buf, src_off, C, dst_off; };
struct YoloUpcopyOp { int src, src_off, C, dst, dst_off, factor; };
struct YoloAttnOp { int src, src_off, embed, dst, heads, guide; };
struct YoloOp {
    int kind;
    union { YoloConvOp conv; YoloPoolOp pool; YoloUpcopyOp up; YoloAttnOp attn; };
};
struct YoloGuide { int embed, heads, w_off, b_off, bias_off; };
struct YoloLevel { int e_buf, r_buf, size, stride, param_off; float logit_scale, bias; };
struct YoloProgram {
    std::vector<YoloBuf> bufs;
    std::vector<YoloOp> ops;
    std::vector<YoloGuide> guides;
    std::vector<YoloLevel> levels;
    int n_anchor = 0;
};

// ------------------------------------------------------------------ decisions the checker and the conv planner share
inline int conv_out_size(int in, int ks, int stride) { return (in + 2 * (ks / 2) - ks) / stride + 1; }

// the LDS-tiled, scalar-weight and halo forms read 16-byte quads of 16-channel slices; everything else is the direct form
inline bool conv_tiled(int cin, int src_ld, int src_off, int ks) {
    return cin % CBK == 0 && src_ld % 4 == 0 && src_off % 4 == 0 && (ks == 1 || ks == 3);
}

// Why the direct form cannot serve a conv (null: it can), worded for a program (after "malformed op N") and for a plan.
struct DirectRefusal { const char* in_program; const char* in_plan; };
inline const DirectRefusal* direct_form_error(int cin, int ks, int cout, int mode) {
    static const DirectRefusal fused = {": the direct form (cin % 16 != 0 or unaligned input channels) has no fused residual / gate",
                                        "yolo conv: the direct form has no fused residual / gate"};
    static const DirectRefusal size = {": the direct form (cin % 16 != 0 or unaligned input channels) needs cout % 16 == 0 and its weights in 64 KB of LDS",
                                       "yolo conv: the direct (small-K) form needs cout % 16 == 0 and its weights in 64 KB of LDS"};
    if (mode != MODE_PLAIN) return &fused;
    const long long K = (long long)ks * ks * cin;            // cout <= 4096 where the product is formed
    if (cout % DCH != 0 || cout / DCH > DIRECT_MAX_GROUPS || (unsigned long long)K * cout * 4 > DIRECT_LDS_BYTES) return &size;
    return nullptr;
}

// ------------------------------------------------------------------ check + decode
// The arguments of tstar_yolo_create behind `out`.  Returns "" and fills *prog, or the message tstar_yolo_create gives.
// Reads h_blob only for the two scalars of each head level.  Order: the shape of the call, buffers, attention layers, head
// levels, ops.
inline std::string decode_program(const float* h_blob, size_t n_blob, const int32_t* h_ops, int n_ops, int op_words, const int32_t* h_bufs,
                                  int n_bufs, const int32_t* h_guides, int n_guides, const int32_t* h_levels, int n_levels, int input_buf,
                                  int max_batch, YoloProgram* prog) {
#define TSTAR_YP_REQUIRE(cond, msg) do { if (!(cond)) return std::string(msg) + " (" #cond ")"; } while (0)
    TSTAR_YP_REQUIRE(h_blob && h_ops && h_bufs && h_levels && (h_guides || n_guides == 0), "tstar_yolo_create: null argument");
    TSTAR_YP_REQUIRE(op_words == OP_WORDS && n_ops >= 1 && n_bufs >= 1 && n_guides >= 0 && n_levels >= 1 && n_levels <= 8, "tstar_yolo_create: bad program shape");
    TSTAR_YP_REQUIRE(max_batch >= 1 && max_batch <= 1024, "tstar_yolo_create: max_batch must be in 1..1024");
    TSTAR_YP_REQUIRE(input_buf >= 0 && input_buf < n_bufs, "tstar_yolo_create: bad input buffer");
#undef TSTAR_YP_REQUIRE
    typedef long long i64;
    YoloProgram p;
    for (int i = 0; i < n_bufs; ++i) {
        const int32_t* row = h_bufs + (size_t)i * BUF_WORDS;
        const YoloBuf b{row[BUF_H], row[BUF_W], row[BUF_C]};
        if (b.H < 1 || b.W < 1 || b.C < 1) return "tstar_yolo_create: bad buffer shape";
        if ((i64)b.H * b.W > INT_MAX / max_batch) return "tstar_yolo_create: buffer too large for the kernels' 32-bit pixel index";
        p.bufs.push_back(b);
    }
    const YoloBuf& in = p.bufs[input_buf];
    if (in.H != YOLO_IMG || in.W != YOLO_IMG || in.C != 3) return "tstar_yolo_create: the input buffer must be 640 x 640 x 3";
    auto buf_ok = [&](int b) { return b >= 0 && b < n_bufs; };
    // rows x row_len floats at blob offset off
    auto off_ok = [&](i64 off, i64 rows, i64 row_len) {
        if (off < 0 || rows < 0 || row_len < 0 || (size_t)off > n_blob) return false;
        return row_len == 0 || (size_t)rows <= (n_blob - (size_t)off) / (size_t)row_len;
    };
    // channels [off, off + n) of a C-channel buffer
    auto chan_ok = [](i64 off, i64 n, int C) { return off >= 0 && off + n <= C; };

    for (int i = 0; i < n_guides; ++i) {
        const int32_t* row = h_guides + (size_t)i * GUIDE_WORDS;
        const YoloGuide g{row[GUIDE_EMBED], row[GUIDE_HEADS], row[GUIDE_W_OFF], row[GUIDE_B_OFF], row[GUIDE_BIAS_OFF]};
        if (g.embed < 1 || g.heads < 1 || g.embed % g.heads || !off_ok(g.w_off, g.embed, YOLO_TEXT) || !off_ok(g.b_off, g.embed, 1) ||
            !off_ok(g.bias_off, g.heads, 1) || (size_t)YOLO_MAX_Q * g.embed * sizeof(float) > YOLO_GUIDE_LDS_BYTES)
            return "tstar_yolo_create: malformed attention layer";
        p.guides.push_back(g);
    }
    i64 n_anchor = 0;
    for (int i = 0; i < n_levels; ++i) {
        const int32_t* row = h_levels + (size_t)i * LEVEL_WORDS;
        YoloLevel l{row[LEVEL_E_BUF], row[LEVEL_R_BUF], row[LEVEL_SIZE], row[LEVEL_STRIDE], row[LEVEL_PARAM_OFF], 0.f, 0.f};
        if (!buf_ok(l.e_buf) || !buf_ok(l.r_buf) || ((i64)l.size * l.size) % 16 != 0 || p.bufs[l.e_buf].C != YOLO_TEXT ||
            p.bufs[l.r_buf].C != 4 * YOLO_REG_MAX || p.bufs[l.e_buf].H != l.size || p.bufs[l.r_buf].H != l.size || !off_ok(l.param_off, 2, 1))
            return "tstar_yolo_create: malformed head level";
        n_anchor += (i64)l.size * l.size;
        if (n_anchor > INT_MAX / max_batch) return "tstar_yolo_create: malformed head level";   // the tail's row ids are int
        l.logit_scale = h_blob[l.param_off]; l.bias = h_blob[(size_t)l.param_off + 1];
        p.levels.push_back(l);
    }
    p.n_anchor = (int)n_anchor;

    for (int i = 0; i < n_ops; ++i) {
        const int32_t* w = h_ops + (size_t)i * op_words;
        YoloOp op{};
        op.kind = w[W_KIND];
        bool ok = true;
        const char* why = "";                                        // what the kernels cannot serve, where the op is otherwise well formed
        if (op.kind == OP_CONV) {
            const YoloConvOp c{w[W_SRC], w[W_SRC_OFF], w[W_CIN], w[W_DST], w[W_DST_OFF], w[W_COUT], w[W_KS], w[W_STRIDE], w[W_ACT],
                               w[W_W_OFF], w[W_B_OFF], w[W_MODE], w[W_AUX], w[W_AUX_OFF]};
            op.conv = c;
            ok = buf_ok(c.src) && buf_ok(c.dst) && c.cin >= 1 && c.cout >= 1 && (c.ks == 1 || c.ks == 3) && (c.stride == 1 || c.stride == 2) &&
                 chan_ok(c.src_off, c.cin, p.bufs[c.src].C) && chan_ok(c.dst_off, c.cout, p.bufs[c.dst].C) && p.bufs[c.dst].C % 4 == 0 &&
                 off_ok(c.w_off, c.cout, (i64)c.ks * c.ks * c.cin) && (c.b_off < 0 || off_ok(c.b_off, c.cout, 1)) &&
                 (c.mode == MODE_PLAIN || (buf_ok(c.aux) && c.aux_off >= 0));
            if (ok) {
                const YoloBuf &s = p.bufs[c.src], &d = p.bufs[c.dst];
                ok = conv_out_size(s.H, c.ks, c.stride) == d.H && conv_out_size(s.W, c.ks, c.stride) == d.W;
            }
            // what launch_conv would refuse at the first forward, or the kernels would get wrong silently: refused here instead
            // (tests/test_yolo_program_host.py plans every conv op of every accepted program)
            if (ok && (c.cout % 4 != 0 || c.dst_off % 4 != 0)) { ok = false; why = ": conv output channels and their offset must be multiples of 4"; }
            if (ok && c.mode != MODE_PLAIN && c.mode != MODE_RESIDUAL && c.mode != MODE_ATTN_MUL) { ok = false; why = ": unknown conv mode"; }
            if (ok && c.mode != MODE_PLAIN && (p.bufs[c.aux].H != p.bufs[c.dst].H || p.bufs[c.aux].W != p.bufs[c.dst].W)) {
                ok = false; why = ": the residual / gate buffer must have the output's map size";
            }
            if (ok && c.mode == MODE_RESIDUAL && (c.aux_off % 4 != 0 || p.bufs[c.aux].C % 4 != 0 || !chan_ok(c.aux_off, c.cout, p.bufs[c.aux].C))) {
                ok = false; why = ": the residual channels must be 16-byte aligned and inside their buffer";
            }
            if (ok && c.mode == MODE_ATTN_MUL && (c.aux_off != 0 || c.cout % p.bufs[c.aux].C != 0)) {
                ok = false; why = ": gated output channels must divide evenly among the heads of the gate buffer (read at offset 0)";
            }
            if (ok && !conv_tiled(c.cin, p.bufs[c.src].C, c.src_off, c.ks)) {
                if (const DirectRefusal* r = direct_form_error(c.cin, c.ks, c.cout, c.mode)) { ok = false; why = r->in_program; }
            }
        } else if (op.kind == OP_POOL5) {
            const YoloPoolOp q{w[W_SRC], w[W_SRC_OFF], w[W_C], w[W_DST_OFF]};
            op.pool = q;
            ok = buf_ok(q.buf) && w[W_DST] == q.buf && q.C >= 4 && q.C % 4 == 0 && q.src_off % 4 == 0 && q.dst_off % 4 == 0 && p.bufs[q.buf].C % 4 == 0 &&
                 chan_ok(q.src_off, q.C, p.bufs[q.buf].C) && chan_ok(q.dst_off, q.C, p.bufs[q.buf].C);
        } else if (op.kind == OP_UPCOPY) {
            const YoloUpcopyOp u{w[W_SRC], w[W_SRC_OFF], w[W_C], w[W_DST], w[W_DST_OFF], w[W_FACTOR]};
            op.up = u;
            ok = buf_ok(u.src) && buf_ok(u.dst) && (u.factor == 1 || u.factor == 2) && u.C >= 4 && u.C % 4 == 0 && u.src_off % 4 == 0 && u.dst_off % 4 == 0 &&
                 p.bufs[u.src].C % 4 == 0 && p.bufs[u.dst].C % 4 == 0 && chan_ok(u.src_off, u.C, p.bufs[u.src].C) &&
                 chan_ok(u.dst_off, u.C, p.bufs[u.dst].C) && (i64)p.bufs[u.src].H * u.factor == p.bufs[u.dst].H &&
                 (i64)p.bufs[u.src].W * u.factor == p.bufs[u.dst].W;
        } else if (op.kind == OP_ATTN) {
            const YoloAttnOp a{w[W_SRC], w[W_SRC_OFF], w[W_EMBED], w[W_DST], w[W_HEADS], w[W_GUIDE]};
            op.attn = a;
            ok = buf_ok(a.src) && buf_ok(a.dst) && a.guide >= 0 && a.guide < n_guides && a.heads >= 1 && a.embed % a.heads == 0 &&
                 p.bufs[a.dst].C == a.heads && chan_ok(a.src_off, a.embed, p.bufs[a.src].C);
            // attn_kernel takes embed and heads from the guide and writes one row of heads per source pixel
            if (ok && (p.guides[a.guide].embed != a.embed || p.guides[a.guide].heads != a.heads)) { ok = false; why = ": embed / heads differ from the op's attention layer"; }
            if (ok && (p.bufs[a.dst].H != p.bufs[a.src].H || p.bufs[a.dst].W != p.bufs[a.src].W)) { ok = false; why = ": the gate buffer must have the source's map size"; }
        } else ok = false;
        if (!ok) return "tstar_yolo_create: malformed op " + std::to_string(i) + why;
        p.ops.push_back(op);
    }
    *prog = std::move(p);
    return std::string();
}

}  // namespace tstar
