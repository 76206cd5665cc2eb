"""Helpers of tests/test_attention_forms_reference.py (CPU) and tests/test_gpu_attention_forms.py (GPU): operands for the three attention
kernels (csrc/attention_f32.hip, attention_split.hip, attention_x3.h) whose softmax(Q K^T / 8) V has a CLOSED FORM, that closed form, the
kernel form a T selects restated as arithmetic on T, and the case table.  Nothing here is shared with the code under test.

The indicator family, for one (image, head), head_dim 64:
  K[k][d] in {0, 1}: dimension d names the key set S_d = {k : K[k][d] = 1};
  Q[q] = C_Q e_d(q), one non-zero, C_Q = 2048;
  V[k][d'] a non-zero integer, |V| <= 2000.
Every score is ONE product fl(C_Q sc) K[k][d(q)], sc = fl(log2(e) / 8), every other term of the contraction is an exact zero, so no order
of the contraction can move it: the MFMA chains, the VALU straggler key, the VALU straggler query of the f32 kernel's 16-query tail, the
six-product three-term path (C_Q is a power of two, so C_Q sc is sc's significand and its three bfloat16 terms add back to it exactly) and
the three-product two-term path (which carries the SAME 16-bit q in the MFMAs and in the straggler).  The keys of S_d(q) tie bit for bit at
about 369 (log2 units), every other valid key scores 0 and weighs exp2(-369) = 0 exactly (float32 has nothing below 2^-149), masked keys
score -inf.  The accumulator then holds an integer sum of V below 2^24 (exact in float32; integer V up to 2000 is two bfloat16 terms, and
its three terms are integers) and the normaliser is the number of keys.  The output is the MEAN OF V over S_d(q) intersected with the valid
keys, or over all valid keys where that intersection is empty.  Valid: k < T; in mode 1 also k <= q and key_mask[k] != 0.

What is asserted (check_indicator):
  * the number of keys averaged is a power of two (1 included): the output equals the float64 mean BIT FOR BIT (int32 views) -- 1 / l or
    a division by l is exact, and so is the product;
  * otherwise |out - mean64| <= 2^-22 mean(|V|) over those keys: the sum S is exact; the kernels form S * fl(1 / l) or fl(S / l): one
    rounding in the reciprocal (relative 2^-24), one in the product (2^-24), together at most 2^-23 (1 + 2^-24) |S| / l < 2^-22 |mean|, and
    |mean| <= mean(|V|).

V "collision-free": a head has up to 577 x 64 (key, dim) pairs and |V| <= 2000 leaves 4000 non-zero values, so all pairs cannot differ
once T > 62.  What a swapped, shifted or mis-addressed element needs is that pairs which share a key or share a dim differ; V[k][d] =
perm[(64 k + d + off) mod 3999] over 3999 distinct values gives that for every T here (64 is invertible mod 3999; a row is 64 consecutive
residues), and for T <= 62 no two pairs of the head collide at all.  Zero is left out of the alphabet so that no output is a signed zero.

The graded family: same Q, K in {1, 255/256, 254/256, 253/256} (bfloat16-exact) on some keys of a dim, zero elsewhere.  The weights are
about 2^(-1.44 j): neither 0 nor 1.  The top level comes late -- in the last MFMA tile (even dims) or on key T - 1 (odd dims) -- so the
alpha rescale and the merge of partial states carry real factors.  Expected: float64 softmax attention on the float32 operands
(attention64); bound: the existing test_attention_* bounds times max |V| (GRADED_TOL).
"""
import zlib

import numpy as np

HD, KB, QB = 64, 32, 128                       # head_dim, keys per tile, queries per block
C_Q = 2048.0
V_MAX = 2000
V_ALPHABET = np.array([v for v in range(-V_MAX, V_MAX) if v != 0], np.int64)      # 3999 values, odd count
GUARD_ROWS = 64
SENTINEL = 0x7FC0BEEF                          # a quiet NaN with a payload, compared as int32
SC32 = np.float32(0.125) * np.float32(1.44269504088896340736)                    # the kernels' log2(e) / 8
KERNELS = ("f32", "split", "x3")
ENTRY = {"f32": "tstar_attention_f32", "split": "tstar_attention_split", "x3": "tstar_attention_x3"}
LEVELS = (1.0, 255.0 / 256, 254.0 / 256, 253.0 / 256)
GRADED_TOL = {"f32": 2e-5, "x3": 2e-5, "split": 2e-4}                            # tests/test_gpu_kernels.py test_attention_full / _x3 / _split
REL_BOUND = 2.0 ** -22

T_TABLE = (1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 160, 161, 193, 255, 257, 320, 337)
T_LONG = 577
# (T, B, heads), mode 0, every kernel
CASES = tuple((T, 2, 2) for T in T_TABLE) + ((T_LONG, 1, 2),)
MODE1_T = (1, 16, 33, 77, 130)
MODE1_B, MODE1_HEADS = 4, 2
T16_OFF_T = (65, 193)                          # the TSTAR_ATTN_T16=0 child
N_NAMED = 16                                   # dims 0 .. 15 carry the named sets, 16 .. 63 seeded sets of 1, 2, 4, 8 keys
NAMED = ("last", "first", "ends", "empty", "last_tile_first", "each_tile", "tile_firsts", "last_tile_only", "last_mfma_tile_only",
         "shares_all", "share_only_0", "share_only_1", "share_only_2", "share_only_3", "pair16", "pair4")
ALIASES = {"masked_last_and_0": "ends"}        # the last valid key of a masked tile together with key 0 IS {0, T - 1}


# ------------------------------------------------------------------------------------------------ forms, restated from the launch code
def mfma_tiles(T, mode=0):
    """Key tiles the MFMA loop runs: the straggler key of T = 32 n + 1 is not one of them (mode 0)."""
    return T // KB if (mode == 0 and T % KB == 1) else -(-T // KB)


def forms(kernel, T, mode=0, t16=True):
    """(key form, query form) of a launch.  Key side: mode 0 folds key T - 1 in with VALU ops when T % 32 == 1, masks the last tile for any
    other T % 32 != 0 and runs it unmasked at T % 32 == 0; the x3 kernel runs its tiles in pairs while three more remain (kb + 3 < nkb)
    and peels the last one to three, so below four tiles it has the peeled form only.  Mode 1 (f32 only) masks every tile.  Query side:
    the last 128-query block holds (T - 1) % 128 + 1 queries in 32-query wave tiles; the f32 kernel sends T % 128 == 65 through the
    16-query tail workgroup unless TSTAR_ATTN_T16=0."""
    assert kernel in KERNELS and T >= 1 and (mode == 0 or kernel == "f32")
    if mode == 1:
        key = "causal_one_tile" if T <= KB else "causal_multi_tile"
    else:
        key = {1: "straggler", 0: "unmasked"}.get(T % KB, "masked")
        if kernel == "x3":
            key += "/paired" if mfma_tiles(T) >= 4 else "/peeled"
    in_last = (T - 1) % QB + 1
    if kernel == "f32" and mode == 0 and t16 and T % QB == 65:
        query = "tail16"
    elif in_last == 1:
        query = "one_query"
    else:
        query = "inactive_waves" if -(-in_last // 32) < 4 else "all_waves"
    return key, query


def reachable_forms(kernel):
    """Every key form and every query form a T >= 1 can select in `kernel`, over both modes (knob at its default)."""
    keys, queries = set(), set()
    for mode in ((0, 1) if kernel == "f32" else (0,)):
        for T in range(1, 4 * QB + 1):
            k, q = forms(kernel, T, mode)
            keys.add(k)
            queries.add(q)
    return keys, queries


def table_rows(kernel):
    """[(T, mode)] of the case table that run `kernel`."""
    return [(T, 0) for T, _, _ in CASES] + ([(T, 1) for T in MODE1_T] if kernel == "f32" else [])


# ------------------------------------------------------------------------------------------------ key sets
def named_sets(T):
    """name -> sorted tuple of keys; what does not fit below T is dropped (a set may end up empty: a uniform mean)."""
    last = T - 1
    lt = last // KB                              # the tile that holds key T - 1
    lm = max(T - 2, 0) // KB                     # the last tile of the MFMA loop when T - 1 is the straggler
    ts = mfma_tiles(T) // 2                      # a middle tile: the straggler QUERY's per-wave key shares (keys 8 w .. 8 w + 7)
    tp = min(1, lt)

    def clip(ks):
        return tuple(sorted({int(k) for k in ks if 0 <= k < T}))

    s = {"last": (last,), "first": (0,), "ends": clip((0, last)), "empty": (),
         "last_tile_first": (KB * lt,),
         "each_tile": clip(KB * t + (5 + 7 * t) % min(KB, T - KB * t) for t in range(lt + 1)),
         "tile_firsts": clip(KB * t for t in range(lt + 1)),
         "last_tile_only": clip((KB * lt + (last - KB * lt) // 2, last)),
         "last_mfma_tile_only": clip((KB * lm + 1 % min(KB, T - KB * lm), KB * lm + 6 % min(KB, T - KB * lm))),
         "shares_all": clip(KB * ts + 8 * w + (3 * w + 1) % 8 for w in range(4)),
         "pair16": clip((KB * tp + 3, KB * tp + 19)),
         "pair4": clip((KB * tp + 9, KB * tp + 13))}
    for w in range(4):
        s[f"share_only_{w}"] = clip((KB * ts + 8 * w + 2, KB * ts + 8 * w + 7))
    assert set(s) == set(NAMED)
    return s


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) % (1 << 31))


def head_sets(T, seed):
    """The 64 key sets of a head: NAMED on dims 0 .. 15, seeded sets of 1, 2, 4, 8 keys behind them."""
    ns = named_sets(T)
    sets = [ns[n] for n in NAMED]
    rs = _rs("fill", T, seed)
    for d in range(N_NAMED, HD):
        n = min((1, 2, 4, 8)[(d - N_NAMED) % 4], T)
        sets.append(tuple(sorted(int(k) for k in rs.choice(T, n, replace=False))))
    return sets


def make_v(T, seed):
    rs = _rs("v", T, seed)
    perm = rs.permutation(V_ALPHABET)
    off = int(rs.randint(0, len(perm)))
    idx = (HD * np.arange(T)[:, None] + np.arange(HD)[None, :] + off) % len(perm)
    return perm[idx].astype(np.float32)


def query_dims(T, rot, fill=False):
    """d(q).  Named rounds: (q + rot) % 16, so every aligned group of 16 queries (a 16-query wave tile of the tail workgroup, half a
    32-query wave tile) meets every named set, and query T - 1 meets them all over rot = 0 .. 15.  The fill round walks dims 16 .. 63."""
    q = np.arange(T)
    return (N_NAMED + (7 * q + rot) % (HD - N_NAMED)) if fill else (q + rot) % N_NAMED


class Head:
    """One (image, head): Q, K, V [T, 64] float32, the sets behind K (indicator) or the level index per (key, dim) (graded), d(q)."""

    def __init__(self, T, K, V, qd, sets=None):
        self.T, self.K, self.V, self.qd, self.sets = T, K, V, np.asarray(qd), sets
        self.Q = np.zeros((T, HD), np.float32)
        self.Q[np.arange(T), self.qd] = C_Q


def indicator_head(T, seed, rot, fill=False):
    sets = head_sets(T, seed)
    K = np.zeros((T, HD), np.float32)
    for d, ks in enumerate(sets):
        K[list(ks), d] = 1.0
    return Head(T, K, make_v(T, seed), query_dims(T, rot, fill), sets)


def graded_head(T, seed, rot):
    rs = _rs("graded", T, seed)
    K = np.zeros((T, HD), np.float32)
    lm = max(T - 2, 0) // KB
    for d in range(HD):
        ks = rs.choice(T, min(T, 10), replace=False)
        K[ks, d] = np.array(LEVELS, np.float32)[rs.randint(1, 4, len(ks))]
        top = T - 1 if d % 2 else KB * lm + int(rs.randint(0, min(KB, T - KB * lm)))
        K[top, d] = 1.0
    return Head(T, K, make_v(T, seed), (np.arange(T) * 5 + rot) % HD)


def rounds(B, heads, mode=0):
    """[(fill, rot(b, h))] of the indicator launches of a case: the named rotations 0 .. 15 are spread over the (image, head) pairs of as
    many launches as that takes (mode 1: over the heads only, every image has a mask of its own), then one fill round."""
    per = heads if mode == 1 else B * heads
    out = []
    for r in range(-(-N_NAMED // per)):
        out.append((False, (lambda b, h, r=r: (r * per + (h if mode == 1 else b * heads + h)) % N_NAMED)))
    out.append((True, lambda b, h: 11 * (b * heads + h)))
    return out


def launch_heads(kind, T, B, heads, rnd=0, mode=0):
    """{(b, h): Head} of one launch.  kind: "indicator" (round rnd of rounds()) or "graded"."""
    out = {}
    fill, rot = rounds(B, heads, mode)[rnd] if kind == "indicator" else (False, None)
    for b in range(B):
        for h in range(heads):
            seed = (kind, rnd, b, h)
            out[b, h] = indicator_head(T, seed, rot(b, h), fill) if kind == "indicator" else graded_head(T, seed, 16 * (b * heads + h) + rnd)
    return out


def pack_qkv(hd, T, B, heads):
    """{(b, h): Head} -> the fused projection [B * T, 3 * heads * 64] (q | k | v)."""
    D = heads * HD
    qkv = np.zeros((B, T, 3, heads, HD), np.float32)
    for (b, h), x in hd.items():
        qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = x.Q, x.K, x.V
    return qkv.reshape(B * T, 3 * D)


def head_rows(out, b, h, T, heads):
    """The [T, 64] block of (image b, head h) in an output [B * T, heads * 64]."""
    return out.reshape(-1, T, heads, HD)[b, :, h]


# ------------------------------------------------------------------------------------------------ masks
def mode1_key_masks(T):
    """[4, T] uint8: lengths 1, T, and two in between, right-padded; the last image's valid part has holes (1, 0, 1, 1, 0, ...)."""
    lens = mode1_lengths(T)
    km = np.zeros((MODE1_B, T), np.uint8)
    for i, n in enumerate(lens):
        km[i, :n] = 1
    km[3, :lens[3]] = np.resize(np.array([1, 0, 1, 1, 0], np.uint8), lens[3])
    return km


def mode1_lengths(T):
    return [1, T, max(1, (T + 2) // 3), max(1, (2 * T + 2) // 3)]


def valid_matrix(T, mode=0, key_mask=None):
    """valid[q][k]."""
    v = np.ones((T, T), bool)
    if mode == 1:
        v &= np.tril(np.ones((T, T), bool))
        v &= (np.asarray(key_mask) != 0)[None, :]
    return v


# ------------------------------------------------------------------------------------------------ expectations
class Expected:
    def __init__(self, mean, count, absmean, compared):
        self.mean, self.count, self.absmean, self.compared = mean, count, absmean, compared


def closed_form(K, V, qd, valid):
    """The closed form on explicit operands: K [n, 64] 0/1, V [n, 64] integers, d(q) [m], valid [m, n].  -> Expected: float64 mean [m, 64],
    keys averaged [m], mean |V| over them [m, 64], rows with a valid key [m]."""
    member = (K[:, qd].T != 0) & valid
    member = np.where(member.any(1)[:, None], member, valid)
    cnt = member.sum(1)
    compared = cnt > 0
    c = np.maximum(cnt, 1)[:, None].astype(np.float64)
    Vi = np.rint(V).astype(np.float64)                                   # integer sums below 2^24: exact in float64, in any order
    m = member.astype(np.float64)
    return Expected((m @ Vi) / c, cnt, (m @ np.abs(Vi)) / c, compared)


def expected_indicator(head, valid):
    return closed_form(head.K, head.V, head.qd, valid)


def attention64(Q, K, V, valid):
    """Plain float64 softmax(Q K^T / 8 + mask) V on float32 operands; rows without a valid key come out as NaN."""
    s = (Q.astype(np.float64) @ K.astype(np.float64).T) * 0.125
    s = np.where(valid, s, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.exp(s - s.max(1, keepdims=True))
        return (p @ V.astype(np.float64)) / p.sum(1, keepdims=True)


def is_pow2(n):
    n = np.asarray(n)
    return (n > 0) & ((n & (n - 1)) == 0)


def check_indicator(got, exp, what=""):
    """got [T, 64] float32 against Expected.  -> (rows compared bit for bit, rows compared by the 2^-22 bound).  Raises AssertionError."""
    got = np.ascontiguousarray(got, np.float32)
    bit = exp.compared & is_pow2(exp.count)
    bnd = exp.compared & ~is_pow2(exp.count)
    want32 = exp.mean.astype(np.float32)
    assert np.array_equal(want32[bit].astype(np.float64), exp.mean[bit]), f"{what}: a power-of-two mean is not a float32"
    bad = (got.view(np.int32) != want32.view(np.int32)).any(1) & bit
    if bad.any():
        q = int(np.flatnonzero(bad)[0])
        d = int(np.flatnonzero(got[q].view(np.int32) != want32[q].view(np.int32))[0])
        raise AssertionError(f"{what}: row {q} (mean over {int(exp.count[q])} keys) differs in bits at dim {d}: got {got[q, d]!r}, want {want32[q, d]!r}; "
                             f"{int(bad.sum())} of {int(bit.sum())} bitwise rows differ")
    with np.errstate(invalid="ignore"):
        over = ~(np.abs(got.astype(np.float64) - exp.mean) <= REL_BOUND * exp.absmean)
    over = over.any(1) & bnd
    if over.any():
        q = int(np.flatnonzero(over)[0])
        e = np.abs(got[q].astype(np.float64) - exp.mean[q])
        d = int(np.nanargmax(np.where(np.isnan(e), np.inf, e) / exp.absmean[q]))
        raise AssertionError(f"{what}: row {q} (mean over {int(exp.count[q])} keys) dim {d}: got {got[q, d]!r}, want {exp.mean[q, d]!r}, "
                             f"bound {REL_BOUND * exp.absmean[q, d]:.3e}; {int(over.sum())} of {int(bnd.sum())} bounded rows are outside")
    return int(bit.sum()), int(bnd.sum())


def differs_beyond_bound(wrong, exp):
    """Rows of a wrong model's output (float64 [T, 64]) that check_indicator would refuse."""
    with np.errstate(invalid="ignore"):
        d = ~(np.abs(wrong - exp.mean) <= REL_BOUND * exp.absmean)
    return d.any(1) & exp.compared


def graded_error(got, head, valid, kernel):
    """-> (largest |got - float64 reference| over rows with a valid key, the bound GRADED_TOL x max |V|)."""
    ref = attention64(head.Q, head.K, head.V, valid)
    rows = valid.any(1)
    g = np.asarray(got, np.float64)[rows]
    if not np.isfinite(g).all():
        return float("inf"), GRADED_TOL[kernel] * float(np.abs(head.V).max())
    return float(np.abs(g - ref[rows]).max()), GRADED_TOL[kernel] * float(np.abs(head.V).max())


# ------------------------------------------------------------------------------------------------ wrong-kernel models
# Each returns the float64 output [T, 64] a kernel with that defect would give on an indicator head (through the same closed form on
# changed operands), and names the T it concerns.  tests/test_attention_forms_reference.py asserts that check_indicator would notice.
def _cf(K, V, qd, valid):
    return closed_form(K, V, qd, valid).mean


def model_masked_keys_counted(head, valid, zeros=False):
    """The keys T .. 32 ceil(T / 32) - 1 of a masked last tile weigh in: as copies of row T - 1 (f32, split) or as zero rows (x3)."""
    T = head.T
    pad = -(-T // KB) * KB - T
    K = np.concatenate([head.K, np.repeat(head.K[-1:] * (not zeros), pad, 0)])
    V = np.concatenate([head.V, np.repeat(head.V[-1:] * (not zeros), pad, 0)])
    return _cf(K, V, head.qd, np.concatenate([valid, np.repeat(valid[:, -1:], pad, 1)], 1))


def model_last_key_dropped(head, valid):
    v = valid.copy()
    v[:, -1] = False
    return _cf(head.K, head.V, head.qd, v)


def model_last_key_twice(head, valid):
    return _cf(np.concatenate([head.K, head.K[-1:]]), np.concatenate([head.V, head.V[-1:]]), head.qd, np.concatenate([valid, valid[:, -1:]], 1))


def model_causal_strict(head, key_mask):
    """k < q instead of k <= q (mode 1)."""
    T = head.T
    return _cf(head.K, head.V, head.qd, np.tril(np.ones((T, T), bool), -1) & (np.asarray(key_mask) != 0)[None, :])


def model_mask_mod_tile(head, key_mask):
    """key_mask read at k mod 32 (mode 1)."""
    T = head.T
    km = np.asarray(key_mask)[np.arange(T) % KB]
    return _cf(head.K, head.V, head.qd, valid_matrix(T, 1, km))


def model_share_dropped(head, valid, w):
    """Wave w's share of the straggler query (keys 8 w .. 8 w + 7 of every MFMA tile) never reaches the merge (f32 tail workgroup)."""
    T = head.T
    v = valid.copy()
    k = np.arange(T)
    v[T - 1, (k < mfma_tiles(T) * KB) & ((k % KB) // 8 == w)] = False
    return _cf(head.K, head.V, head.qd, v)


def model_keys_swapped(head, valid, dist):
    """V rows k and k + dist of a tile change places (k % (2 dist) < dist, both below T): a wrong LDS row rotation / key permutation."""
    T = head.T
    k = np.arange(T)
    lo = k[((k % KB) % (2 * dist) < dist) & (k + dist < T)]
    V = head.V.copy()
    V[lo], V[lo + dist] = head.V[lo + dist], head.V[lo]
    return _cf(head.K, V, head.qd, valid)


def model_row_late(head, valid):
    """Output row q written at q + 1 (row 0 keeps what row T - 1 would have been given)."""
    return np.roll(_cf(head.K, head.V, head.qd, valid), 1, 0)
