"""Helpers of tests/test_owl_front_reference.py (CPU) and tests/test_gpu_owl_front.py (GPU): the OWL-ViT / OWLv2 detector FRONT --
what owl_forward_heads runs between pre-processing and the first encoder layer, and the text tower of tstar_owl_set_queries.

  A  the patch-embedding GEMM (gemm_f32 with pos != nullptr: the PATCH epilogue) in every weight mode and tile form: the shapes,
     the tile_cfg values of every mode, the plans the launcher's own ladder must make, seeded inputs, the float64 product
  B  the tower entry on a handle: crafted class embedding / position table / pre-LayerNorm laid over the synthetic state dict
  C  the CLIP text tower restated in numpy float64 from HF's formulas (CLIPTextTransformer as OwlViTTextTransformer uses it:
     token + position embedding, 12 pre-LN layers under a causal + padding mask, quick-GELU, final LayerNorm, the row at the
     first maximum id, text_projection, x / |x|), one sequence at a time, and the query scenarios T1-T6
Nothing here is shared with the code under test or with oracle/owl_ref.py.
"""
import math

import numpy as np

from owl_tail_util import _unit, ln64

D, T_D, PROJ, T_LEN, T_LAYERS, T_HEADS, VOCAB = 768, 512, 512, 16, 12, 8, 49408

# ------------------------------------------------------------------------------------------------ A: the patch-embed epilogue
MODES = {"f32": 0, "bf16": 1, "bf16_exact": 3, "f32x3": 4}                 # TSTAR_WEIGHTS_*; "bf16" is the two-term mode
BF16_MODES = ("bf16", "bf16_exact")
PLAIN_ENTRY = {"f32": "tstar_gemm_f32_cfg", "bf16": "tstar_gemm_bf16w2", "bf16_exact": "tstar_gemm_bf16w", "f32x3": "tstar_gemm_f32x3"}
GRID_128, GRID_64N, GRID_64, HYBRID, WIDE, WIDE_VW = range(6)              # GemmKind, plan4[0] of tstar_gemm_plan
# every (mode, kind) launch_mode can launch for a patch problem
REACHABLE = ({(m, k) for m in MODES for k in (GRID_128, GRID_64N, GRID_64, HYBRID)} | {("bf16", WIDE), ("f32x3", WIDE), ("bf16", WIDE_VW)})

# S1: 37 patches per image divide no tile height, so every tile straddles image boundaries; M = 333 leaves 77 ragged rows in the last
#     128-row, 64-row and wide panel; K = 96 is an odd K-tile count (the peeled tile of the 64x64 ring)
# S2: every row its own image (ntok = 2, always position row 1)     S3: one image; N = 128 admits no wide tile
# S4: S1's rows at the width and depth of a /16 checkpoint
SHAPES = {"S1": dict(B=9, np=37, N=256, K=96), "S2": dict(B=130, np=1, N=256, K=64), "S3": dict(B=1, np=130, N=128, K=32),
          "S4": dict(B=9, np=37, N=768, K=768)}
SPARE_ROWS = 128                                                           # rows behind B * (np + 1) that must keep their bits
SENTINEL = 0x7FC0BEEF                                                      # a quiet NaN with a payload, compared as int32


def tile_cfgs(mode):
    """-1 = the launcher's choice, 0..2 the pure grids, 3 hybrid, 16 + n hybrid with n big row tiles; 4 / 5 the wide tile forced on /
    off (the modes that have one); 6 the wide tile with weights streamed global -> VGPR (two-term mode)."""
    return (-1, 0, 1, 2, 3, 16 + 1, 16 + 2) + ((4, 5) if mode in ("bf16", "f32x3") else ()) + ((6,) if mode == "bf16" else ())


def has_wq(mode, N):
    """The two-term mode's fragment-packed plane exists (tstar_gemm_bf16w2 and tstar_gemm_patch_embed make it for N % 256 == 0)."""
    return int(mode == "bf16" and N % 256 == 0)


# the launcher's own ladder: tile_cfg -1 at production M with a short K
LADDER = dict(np=576, N=768, K=64)
LADDER_B = (1, 8, 10, 16, 30, 38)
# B -> mode -> (kind, m_split), read off plan_gemm / pick_cfg (csrc/gemm_f32.hip); pinned by tests/test_owl_front_reference.py
_SAME = lambda plan: {m: plan for m in MODES}
LADDER_PLAN = {
    1: _SAME((GRID_64, 0)),                                                # 30 tiles of 128x128
    8: _SAME((GRID_64N, 0)),                                               # 216
    10: _SAME((HYBRID, 2816)),                                             # 270: one mixed wave, 22 of 45 row tiles big
    16: {**_SAME((GRID_128, 0)), "f32x3": (WIDE, 9216)},                   # 432; f32x3: 216 wide tiles, a CU each, m_split = M
    30: {**_SAME((HYBRID, 8576)), "f32x3": (WIDE, 17280)},                 # 810: half of 135 row tiles big; f32x3: 405 wide tiles
    38: {"f32": (HYBRID, 21760), "bf16_exact": (HYBRID, 21760), "bf16": (WIDE_VW, 21760), "f32x3": (WIDE, 21760)},   # two waves + tail
}


def gemm_plan(lib, mode, M, N, patch_np, tile_cfg):
    """(kind, m_split) of the patch problem [M, K] x [N, K]^T, or None where the launcher refuses it."""
    import ctypes as C
    out = (C.c_int * 4)()
    rc = lib.tstar_gemm_plan(MODES[mode], M, N, N, patch_np, tile_cfg, has_wq(mode, N), out)
    assert rc in (0, 1), rc
    return None if rc else (out[0], out[1])


def patch_cases():
    """Every (mode, B, np, N, K, tile_cfg) part A hands to tstar_gemm_patch_embed."""
    out = [(m, s["B"], s["np"], s["N"], s["K"], cfg) for s in SHAPES.values() for m in MODES for cfg in tile_cfgs(m)]
    return out + [(m, B, LADDER["np"], LADDER["N"], LADDER["K"], -1) for B in LADDER_B for m in MODES]


def patch_inputs(B, np_, N, K, seed):
    """A [B*np, K], W [N, K], pos [np+1, N] as float32 torch tensors: the inputs of test_gemm_f32x3 (rows scaled by 1e-3, columns by
    37, W * K**-0.5), a position table of std 0.02 with the class row (never to be read) and three patch rows at +-50."""
    import torch
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(B * np_, K, generator=g)
    A[::7] *= 1e-3
    A[:, ::5] *= 37.0
    W = torch.randn(N, K, generator=g) * K ** -0.5
    pos = torch.randn(np_ + 1, N, generator=g) * 0.02
    pos[0] += 50.0
    for r, v in ((1, -50.0), (np_, 50.0), ((1 + np_) // 2, -50.0)):
        pos[r] += v
    return A, W, pos


def patch_ref64(A, W, pos, B, np_, mode):
    """float64 A W^T + pos[1 + p] and sum |a w| + |pos| per patch row (b, p), both [B*np, N]; W rounded to bf16 first in the bf16 modes."""
    import torch
    W64 = (W.to(torch.bfloat16) if mode in BF16_MODES else W).to(torch.float64)
    A64, p64 = A.to(torch.float64), pos[1:].to(torch.float64)
    ref = ((A64 @ W64.t()).view(B, np_, -1) + p64).reshape(B * np_, -1)
    mag = ((A64.abs() @ W64.abs().t()).view(B, np_, -1) + p64.abs()).reshape(B * np_, -1)
    return ref, mag


# ------------------------------------------------------------------------------------------------ B: the tower entry on a handle
E2_CONST = 2.0                                              # a power of two: the bicubic weights at t = 0.5 are multiples of 1/32, every product and sum exact
E2_ROWS = dict(const=1, plus=3, minus=4)                    # patch indices of the special position rows (handles with np >= 6)


def bicubic_support(geometry, p):
    """Rows of the checkpoint's position table that torch's bicubic resampling (align_corners=False) reads for patch p of the run's
    grid: 4 x 4 taps around the source coordinate, clamped to the table."""
    g, G = geometry, geometry.grid

    def taps(i, n):
        f = math.floor((i + 0.5) * G / n - 0.5)
        return sorted({min(max(f + k, 0), G - 1) for k in (-1, 0, 1, 2)})

    i, j = divmod(p, g.gw)
    return [1 + r * G + c for r in taps(i, g.gh) for c in taps(j, g.gw)]


def crafted_front(geometry, seed=7):
    """HF state-dict entries of the vision tower's entry, to be laid over a synthetic state dict before ``pack_blob``: a class
    embedding and a class position row of visible size, a position table of std 0.02, pre-LayerNorm weights and biases that are
    not 1 / 0.  Where the run has at least 6 patches the table rows behind three of them are set so that the RUN's table (after the
    resampling to its grid) has a constant row (E2_CONST) and rows with mean +-1e3 and a spread near one, like the tail's M2."""
    g, rs, f = geometry, np.random.RandomState(seed), np.float32
    vm = g.prefix + "vision_model."
    pos = (0.02 * _unit(rs, g.grid * g.grid + 1, D)).astype(f)
    pos[0] = (0.3 * _unit(rs, D)).astype(f)
    if g.npatch >= 6:
        assert g.gh < g.grid and g.gw < g.grid
        sup = {k: bicubic_support(g, p) for k, p in E2_ROWS.items()}
        assert len(set(sum(sup.values(), []))) == 48                     # disjoint
        pos[sup["const"]] = E2_CONST
        pos[sup["plus"]] = (1e3 + _unit(rs, 16, D)).astype(f)
        pos[sup["minus"]] = (-1e3 + _unit(rs, 16, D)).astype(f)
    return {
        vm + "embeddings.class_embedding": (0.5 * _unit(rs, D)).astype(f),
        vm + "embeddings.position_embedding.weight": pos,
        vm + "pre_layernorm.weight": (1.0 + 0.2 * _unit(rs, D)).astype(f),
        vm + "pre_layernorm.bias": (0.1 * _unit(rs, D)).astype(f),
    }


def front_blob(family, patch_size, input_size, with_text=False, seed=0):
    """-> (geometry, state dict, vision blob, text blob or None, the entries the handle holds for the front)."""
    from tstar_amd import weights as W
    g = W.with_input_size(W.geometry_for_family(family, patch_size), input_size)
    sd = W.synthetic_state_dict(seed, "both" if with_text else "vision", geometry=g)
    crafted = crafted_front(g)
    assert set(crafted) <= set(sd)                                       # the keys as the checkpoint spells them
    sd.update(crafted)
    vb = W.pack_blob(sd, W.vision_spec(g), g)
    tb = W.pack_blob(sd, W.text_spec(g)) if with_text else None
    held = W.unpack_blob(vb, W.vision_spec(g))
    vm = g.prefix + "vision_model."
    w = dict(patch_w=np.ascontiguousarray(sd[vm + "embeddings.patch_embedding.weight"].reshape(D, g.patch_k)),
             class_emb=crafted[vm + "embeddings.class_embedding"], pos=held["pos_emb"].copy(),
             pre_ln_w=crafted[vm + "pre_layernorm.weight"], pre_ln_b=crafted[vm + "pre_layernorm.bias"])
    for k in ("patch_w", "class_emb", "pre_ln_w", "pre_ln_b"):
        assert np.array_equal(held[k].reshape(-1), w[k].reshape(-1)), k
    return g, sd, vb, tb, w


def embed_patches(geometry, B, seed=11):
    """Unit-variance patches [B*np, patch_k]; with the special position rows the patch under the constant row is zero (the GEMM adds
    exactly 0 to it)."""
    rs = np.random.RandomState(seed + B)
    x = _unit(rs, B * geometry.npatch, geometry.patch_k).astype(np.float32)
    if geometry.npatch >= 6:
        x[E2_ROWS["const"]] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ C: the text tower in float64
def to_bf16(a):
    """float32 -> the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


GEMM_WEIGHTS = ("qkv_w", "out_w", "fc1_w", "fc2_w", "text_proj")          # what a bf16 handle rounds (the embedding tables stay float32)


def bf16_text_weights(w):
    """The text blob's entries with the GEMM matrices rounded to bf16: what the two bf16 modes compute with."""
    return {k: (to_bf16(v) if k.endswith(GEMM_WEIGHTS) else v) for k, v in w.items()}


def first_max(ids):
    """Position of the first maximum id of every sequence (HF: input_ids.argmax(dim=-1))."""
    ids = np.asarray(ids)
    return np.array([min(t for t in range(ids.shape[1]) if ids[q, t] == ids[q].max()) for q in range(ids.shape[0])])


def text64(ids, am, w, prefix="owlvit."):
    """ids, am [Q, 16] integers, w: the text blob's entries -> dict(emb [Q,16,512] float32: token + position rows as float32 sums;
    pooled [Q,512] float64: the final LayerNorm's row at the first maximum id; embeds [Q,512] float64: projected, unit length).
    One sequence at a time, so a row's arithmetic does not depend on the other sequences of the call."""
    f = lambda a: np.asarray(a, np.float64)
    ids, am = np.asarray(ids, np.int64), np.asarray(am)
    Q = ids.shape[0]
    hd = T_D // T_HEADS
    emb32 = (w["tok_emb"][ids] + w["tpos_emb"][None, :, :]).astype(np.float32)
    t = np.arange(T_LEN)
    eos = first_max(ids)
    pooled = np.zeros((Q, T_D))
    for q in range(Q):
        x = f(w["tok_emb"][ids[q]]) + f(w["tpos_emb"])
        visible = (t[None, :] <= t[:, None]) & (am[q][None, :] != 0)   # [query, key]: causal and not padding
        assert visible.any(1).all()
        for i in range(T_LAYERS):
            p = f"{prefix}text_model.encoder.layers.{i}."
            h = ln64(x, w[p + "ln1_w"], w[p + "ln1_b"]) @ f(w[p + "qkv_w"]).T + f(w[p + "qkv_b"])
            qh, kh, vh = (h[:, k * T_D:(k + 1) * T_D].reshape(T_LEN, T_HEADS, hd).transpose(1, 0, 2) for k in range(3))
            s = qh @ kh.transpose(0, 2, 1) * hd ** -0.5
            s = np.where(visible[None], s, -np.inf)
            e = np.exp(s - s.max(-1, keepdims=True))
            o = ((e / e.sum(-1, keepdims=True)) @ vh).transpose(1, 0, 2).reshape(T_LEN, T_D)
            x = x + o @ f(w[p + "out_w"]).T + f(w[p + "out_b"])
            h = ln64(x, w[p + "ln2_w"], w[p + "ln2_b"]) @ f(w[p + "fc1_w"]).T + f(w[p + "fc1_b"])
            h = h / (1.0 + np.exp(-1.702 * h))                           # quick-GELU
            x = x + h @ f(w[p + "fc2_w"]).T + f(w[p + "fc2_b"])
        pooled[q] = ln64(x, w["final_ln_w"], w["final_ln_b"])[eos[q]]
    proj = pooled @ f(w["text_proj"]).T
    return dict(emb=emb32, pooled=pooled, embeds=proj / np.sqrt((proj * proj).sum(-1, keepdims=True)), eos=eos)


BOS, EOS = 49406, 49407


def _seq(tokens, valid=None):
    ids = np.zeros(T_LEN, np.int64)
    ids[:len(tokens)] = tokens
    am = np.zeros(T_LEN, np.int64)
    am[:len(tokens) if valid is None else valid] = 1
    return ids, am


def _stack(seqs):
    return np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs])


def case_t1():
    """Ids 0 and 49407, repeats inside a sequence and across sequences, every position used."""
    return _stack([_seq([BOS, 5, 5, 7, EOS]), _seq([0] * T_LEN), _seq([EOS] * T_LEN), _seq([BOS, 5, 5, 7, EOS, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 49405])])


def case_t2():
    """Queries 0 and 1 agree on tokens 0..3 with the maximum id at t = 3 and differ behind it (query 1 repeats the maximum at t = 9):
    under the causal mask their pooled rows are the same numbers.  Query 2 has its first maximum at t = 9."""
    head = [BOS, 320, 1125, EOS]
    return _stack([_seq(head + [7, 8, 9, 10, 11, 12], T_LEN), _seq(head + [900, 901, 902, 903, 904, EOS, 13], T_LEN),
                   _seq([BOS, 320, 1125, 2000, 900, 901, 902, 903, 904, EOS, 13], T_LEN)])


def case_t3():
    """A right-padded query (first maximum at t = 5), and the same with one interior zero in the attention mask (am[1] = 0)."""
    ids, am = _seq([BOS, 2368, 539, 320, 1929, EOS])
    am0 = am.copy()
    am0[1] = 0
    return np.stack([ids, ids]), np.stack([am, am0])


def case_t4():
    """16 valid tokens, the maximum at t = 15."""
    return _stack([_seq([BOS] + list(range(1000, 1014)) + [EOS])])


def case_t5(Q, seed=17):
    """Q right-padded random queries of 3..16 tokens: BOS, words, EOS."""
    rs = np.random.RandomState(seed + Q)
    seqs = []
    for _ in range(Q):
        n = int(rs.randint(3, T_LEN + 1))
        seqs.append(_seq([BOS] + [int(v) for v in rs.randint(1, BOS, n - 2)] + [EOS]))
    return _stack(seqs)


def case_t6():
    """Queries 1 and 3 start with id 0: padding queries (their logits are -FLT_MAX whatever their embedding is)."""
    return _stack([_seq([BOS, 320, 2368, EOS]), _seq([0] * T_LEN, 1), _seq([BOS, 1125, EOS]), _seq([0, 320, EOS], 3)])
