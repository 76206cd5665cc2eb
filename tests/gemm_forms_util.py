"""Helpers of tests/test_gemm_forms_reference.py (CPU) and tests/test_gpu_gemm_forms.py (GPU): operands for gemm_f32 (csrc/gemm_f32.hip)
whose result is EXACT in float32 whatever the order of the accumulation, and that result per weight mode as an int64 sum.

The family.  Every non-zero operand is s * (1 + u 2^-9 + v 2^-18), s = +-1, (u, v) in (0,0), (1,0), (1,1); its three round-to-nearest
bfloat16 terms are s, s u 2^-9, s v 2^-18 (computed here by `split3`, a restatement of the documented split, never assumed).  W is dense
in the family, A holds at most NNZ = 8 non-zeros per row.  Every product a mode forms is then a multiple of 2^-18, and the sum of the
absolute products of one output element stays below 8.04; with a bias and a residual that are multiples of 2^-18 below 3.96 in magnitude
every partial sum, in any order, is a multiple of 2^-18 below 16 = 2^22 units: 22 significand bits, float32 has 24.  A change of the K
order or of the MFMA order cannot move such a result; a missing, doubled or mis-paired product must.

Crafted rows (row m of every case, by m % 32): 0 = values that TIE in the first rounding (low half 0x8000), 1 = exact bfloat16 values
(1 + j 2^-7, any j), 2 = zeros.  They are outside the family (multiples of 2^-8 / 2^-7 below 2), so they carry 4 non-zeros, and those sit
on the COARSE columns k % 4 == 3, where W takes the patterns (0,0) and (1,0) only: their products are multiples of 2^-17 and the bound
above holds for them too (tests/test_gemm_forms_reference.py asserts all of it on the operands themselves).  M = 1 has room for row 0 only.
In IDENTITY_CASE the first 128 rows of W are an identity block: columns 0..127 of C are A's own columns where the mode carries all 24
bits, which shows the tie rows reassembled.

Nothing here is shared with the code under test.
"""
import zlib

import numpy as np

MODES = {"f32": 0, "bf16": 1, "bf16_exact": 3, "f32x3": 4}                 # TSTAR_WEIGHTS_*; "bf16" is the two-term mode
ENTRY = {"f32": "tstar_gemm_f32_cfg", "bf16": "tstar_gemm_bf16w2", "bf16_exact": "tstar_gemm_bf16w", "f32x3": "tstar_gemm_f32x3"}
GRID_128, GRID_64N, GRID_64, HYBRID, WIDE, WIDE_VW = range(6)              # GemmKind, plan4[0] of tstar_gemm_plan
# every (mode, kind) launch_mode can launch
REACHABLE = ({(m, k) for m in MODES for k in (GRID_128, GRID_64N, GRID_64, HYBRID)} | {("bf16", WIDE), ("f32x3", WIDE), ("bf16", WIDE_VW)})

NNZ = 8
UNIT = 18                                                                  # operand terms are counted in units of 2^-18, products in 2^-36
PATTERNS = ((0, 0), (1, 0), (1, 1))                                        # (0, 1) is excluded: its products would reach 2^-36
LIMIT_UNITS = 1 << 22                                                      # sum |products| + |bias| + |residual| of an element, in 2^-18
BIAS_MAX = int(3.96 * (1 << UNIT))                                         # |bias|, |residual| in 2^-18: 8.04 + 2 * 3.96 < 16
GUARD_ROWS = 64                                                            # rows behind M that must keep their bits
SENTINEL = 0x7FC0BEEF                                                      # a quiet NaN with a payload, compared as int32

# name -> (M, N, K)
CASES = {f"k{K}": (300, 256, K) for K in (32, 64, 96, 160)}                # 2 full 128-row panels + 44 ragged rows; 1 wide / 2 narrow column tiles; 1, 2, 3, 5 K tiles
CASES["n384"] = (129, 384, 64)                                             # N % 256 != 0: the wide tile must fall back
CASES.update({f"m{M}": (M, 256, 64) for M in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)})
CASES["long768"] = (130, 256, 768)                                         # the long loop on sparse rows
CASES["long3072"] = (130, 256, 3072)
LONG_K = 768                                                               # from here on: non-zeros on the K-tile edges
IDENTITY_CASE = "k160"
# tile_cfg -1 at these sizes: at most 6 tiles of 128x128 and at most 3 wide ones -- pick_cfg's first rung, in every mode
AUTO_PLAN = {name: (GRID_64, 0) for name in CASES}

EPILOGUES = ("none", "bias", "bias_res", "bias_res_inplace")


def tile_cfgs(mode, M):
    """-1 = the launcher's choice, 0..2 the pure grids, 3 hybrid, 16 + n hybrid with n big row tiles (one, and every full panel); 4 / 5 the
    wide tile forced on / off (the modes that have one); 6 the wide tile with weights streamed global -> VGPR (two-term mode)."""
    cfgs = (-1, 0, 1, 2, 3, 17, 16 + (M + 127) // 128) + ((4, 5) if mode in ("bf16", "f32x3") else ()) + ((6,) if mode == "bf16" else ())
    return tuple(dict.fromkeys(cfgs))


def has_wq(mode, N):
    """The two-term mode's fragment-packed plane exists (tstar_gemm_bf16w2 makes it for N % 256 == 0; tstar_gemm_bf16w_pre has none)."""
    return int(mode == "bf16" and N % 256 == 0)


def gemm_plan(lib, mode, M, N, tile_cfg, wq=None):
    """(kind, m_split) of [M, K] x [N, K]^T, or None where the launcher refuses it."""
    import ctypes as C
    out = (C.c_int * 4)()
    rc = lib.tstar_gemm_plan(MODES[mode], M, N, N, 0, tile_cfg, has_wq(mode, N) if wq is None else wq, out)
    assert rc in (0, 1), rc
    return None if rc else (out[0], out[1])


# ------------------------------------------------------------------------------------------------ the split, restated
def bf16_rn(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split3(a):
    """a0 = bf16_rn(a), a1 = bf16_rn(a - a0), a2 = a - a0 - a1, the subtractions in float32."""
    a = np.asarray(a, np.float32)
    a0 = bf16_rn(a)
    r1 = (a - a0).astype(np.float32)
    a1 = bf16_rn(r1)
    return a0, a1, (r1 - a1).astype(np.float32)


def units(x):
    """float32 -> int64 count of 2^-18; refuses what is not a multiple."""
    s = np.asarray(x, np.float64) * float(1 << UNIT)
    i = np.rint(s).astype(np.int64)
    assert np.array_equal(i.astype(np.float64), s), "not a multiple of 2^-18"
    return i


def from_units(i):
    """int64 count of 2^-18 -> float32, refusing a value float32 cannot hold."""
    f = (np.asarray(i, np.int64).astype(np.float64) / float(1 << UNIT))
    out = f.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), f)
    return out


# ------------------------------------------------------------------------------------------------ operands
def _family(rs, shape, patterns=PATTERNS):
    p = rs.randint(0, len(patterns), shape)
    u = np.array([q[0] for q in patterns])[p]
    v = np.array([q[1] for q in patterns])[p]
    s = 1 - 2 * rs.randint(0, 2, shape)
    return (s * ((1 << UNIT) + u * (1 << 9) + v)).astype(np.float64) / float(1 << UNIT)


def row_kind(m):
    return {0: "tie", 1: "bf16", 2: "zero"}.get(m % 32, "family")


def rows_of(M, kind):
    return [m for m in range(M) if row_kind(m) == kind]


def _coarse_ks(K, c):
    if K >= LONG_K:
        return [15, 31, K - 33, K - 1]
    return [4 * ((c + 5 * i) % (K // 4)) + 3 for i in range(4)]


def make_operands(name, nnz=NNZ):
    """-> dict(A [M, K], W [N, K], bias [N], res [M, N]) float32, seeded by the case name.  nnz: non-zeros of a family row (the reference
    test builds a 16 to show that the 22-bit condition notices)."""
    M, N, K = CASES[name]
    rs = np.random.RandomState(zlib.crc32(name.encode()) % (1 << 31))
    W = _family(rs, (N, K))
    coarse = np.arange(K) % 4 == 3
    W[:, coarse] = _family(rs, (N, int(coarse.sum())), PATTERNS[:2])
    if name == IDENTITY_CASE:
        W[:128] = np.eye(128, K)
    A = np.zeros((M, K))
    j = 0                                                                  # running count of family rows
    for m in range(M):
        kind = row_kind(m)
        if kind == "family":
            if K < LONG_K:
                ks = [(nnz * j + i) % K for i in range(nnz)]               # K / nnz rows cover every k
            elif j % 2 == 0:
                ks = ([0, 15, 16, 31, 32, K - 33, K - 32, K - 1] + list(range(40, 40 + max(0, nnz - 8))))[:nnz]     # the K-tile edges
            else:                                                          # one non-zero in each of 8 consecutive K tiles, walking through K
                jj, nk = j // 2, K // 32
                ks = [32 * ((8 * jj + i) % nk) + (7 * jj + 5 * i) % 32 for i in range(8)]
            A[m, ks] = _family(rs, len(ks))
            j += 1
        elif kind != "zero":
            ks = _coarse_ks(K, m // 32)
            sign = 1 - 2 * rs.randint(0, 2, 4)
            jbits = rs.randint(0, 128, 4)
            if kind == "tie":                                              # (j << 16) | 0x3F808000: 1 + j 2^-7 + 2^-8
                A[m, ks] = sign * ((jbits.astype(np.uint32) << 16) | 0x3F808000).astype(np.uint32).view(np.float32).astype(np.float64)
            else:
                A[m, ks] = sign * (1.0 + jbits / 128.0)
    bias = rs.randint(-BIAS_MAX, BIAS_MAX + 1, N) / float(1 << UNIT)
    res = rs.randint(-BIAS_MAX, BIAS_MAX + 1, (M, N)) / float(1 << UNIT)
    out = dict(A=A, W=W, bias=bias, res=res)
    for k, v in out.items():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), k
    return {k: v.astype(np.float32) for k, v in out.items()}


def weights_for(mode, W):
    """What the mode's entry is handed: the native f32 tile multiplies a by w itself, so its W keeps the (0,0) pattern only (sign(w), the
    value the bf16 modes round w to)."""
    return np.sign(W).astype(np.float32) if mode == "f32" else W


def activation_operands(ops):
    """The (0,0) pattern only: the pre-activation value is exact and the same number in all four modes."""
    return dict(ops, A=np.sign(ops["A"]).astype(np.float32), W=np.sign(ops["W"]).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the expected value, int64
def term_pairs(mode, A, W):
    """[(A term, W term)] as int64 counts of 2^-18: the operand-term products the mode forms, summed over k.
    f32x3: the six with ka + kw <= 2.  bf16_exact: (a0 + a1 + a2) bf16_rn(w).  bf16: (a0 + a1) bf16_rn(w).  f32: a w."""
    if mode == "f32x3":
        at, wt = [units(t) for t in split3(A)], [units(t) for t in split3(W)]
        return [(at[ka], wt[kw]) for ka in range(3) for kw in range(3) if ka + kw <= 2]
    if mode == "f32":
        return [(units(A), units(W))]
    wb = units(bf16_rn(W))
    a0, a1, a2 = (units(t) for t in split3(A))
    return [(a0, wb), (a1, wb)] + ([(a2, wb)] if mode == "bf16_exact" else [])


def _sparse_matmul(Ai, Wi):
    """Ai [M, K] (few non-zeros per row) times Wi [N, K]^T in int64."""
    out = np.zeros((Ai.shape[0], Wi.shape[0]), np.int64)
    m, k = np.nonzero(Ai)
    np.add.at(out, m, Ai[m, k, None] * Wi[:, k].T)
    return out


def product_units(mode, A, W):
    """sum over k and over the mode's term products, [M, N] int64 in units of 2^-36."""
    return sum(_sparse_matmul(a, w) for a, w in term_pairs(mode, A, W))


def expected(mode, ops, epilogue):
    """The float32 C of the mode for operands `ops` (W as weights_for hands it over) under one of EPILOGUES."""
    p = product_units(mode, ops["A"], weights_for(mode, ops["W"]))
    assert not (p & ((1 << UNIT) - 1)).any()
    t = p >> UNIT
    if epilogue != "none":
        t = t + units(ops["bias"])[None, :]
    if epilogue.startswith("bias_res"):
        t = t + units(ops["res"])
    return from_units(t)


def magnitude_units(mode, ops):
    """max over the output elements of sum |products| (2^-36 units, rounded up to 2^-18) + max |bias| + max |residual|."""
    A, W = ops["A"], weights_for(mode, ops["W"])
    mag = sum(_sparse_matmul(np.abs(a), np.abs(w)) for a, w in term_pairs(mode, A, W))
    return int(-(-mag.max() >> UNIT)) + int(np.abs(units(ops["bias"])).max()) + int(np.abs(units(ops["res"])).max())


# ------------------------------------------------------------------------------------------------ activations, float64
def qgelu64(v):
    v = np.asarray(v, np.float64)
    return v / (1.0 + np.exp(-1.702 * v))


def gelu64(v):
    import math
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + np.vectorize(math.erf)(v / math.sqrt(2.0)))


QGELU_REL = 2.0 ** -17                                                     # |got - want| <= 2^-17 |want|
GELU_ABS_PER_V = 2.0 ** -21                                                # |got - want| <= 2^-21 |v|
