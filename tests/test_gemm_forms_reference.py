"""CPU: the operand family and the case table of tests/test_gpu_gemm_forms.py do what tests/gemm_forms_util.py says they do, so that
the GPU test cannot pass vacuously: the terms are bfloat16 values, every product is a multiple of 2^-18, the 22-bit condition holds
(and notices 16 non-zeros per row), a float32 accumulation in any order returns the int64 sum, the modes' expected values differ
from each other where they should, every k is used, and the table reaches every kernel form launch_mode can launch."""
import numpy as np
import pytest

import gemm_forms_util as G


@pytest.fixture(scope="module")
def ops():
    return {name: G.make_operands(name) for name in G.CASES}


def test_split_terms_of_the_family():
    """s (1 + u 2^-9 + v 2^-18) -> s, s u 2^-9, s v 2^-18, by the restated split; the tie and bf16 rows need two terms and one."""
    for s in (1.0, -1.0):
        for u, v in G.PATTERNS:
            a = np.float32(s * (1 + u * 2.0 ** -9 + v * 2.0 ** -18))
            assert [float(t) for t in G.split3(a)] == [s, s * u * 2.0 ** -9, s * v * 2.0 ** -18]
    tie = np.array([0x3F808000, 0x3F818000], np.uint32).view(np.float32)      # 1 + 2^-8 -> 1 (even), 1 + 2^-7 + 2^-8 -> 1 + 2^-6 (even)
    t0, t1, t2 = G.split3(tie)
    assert t0.tolist() == [1.0, 1.0 + 2.0 ** -6] and t1.tolist() == [2.0 ** -8, -2.0 ** -8] and not t2.any()
    assert G.bf16_rn(np.float32(1 + 2.0 ** -7 + 2.0 ** -9)) == np.float32(1 + 2.0 ** -7)     # below the tie: down


def test_case_table_is_the_issue_s():
    assert [G.CASES[f"k{K}"] for K in (32, 64, 96, 160)] == [(300, 256, K) for K in (32, 64, 96, 160)]
    assert G.CASES["n384"] == (129, 384, 64)
    assert [G.CASES[f"m{M}"][0] for M in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)] == [1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    assert G.CASES["long768"] == (130, 256, 768) and G.CASES["long3072"] == (130, 256, 3072) and len(G.CASES) == 17
    for M, N, K in G.CASES.values():
        assert N % 128 == 0 and K % 32 == 0
    assert G.tile_cfgs("f32", 300) == (-1, 0, 1, 2, 3, 17, 19) and G.tile_cfgs("bf16_exact", 1) == (-1, 0, 1, 2, 3, 17)
    assert G.tile_cfgs("f32x3", 300) == (-1, 0, 1, 2, 3, 17, 19, 4, 5) and G.tile_cfgs("bf16", 129) == (-1, 0, 1, 2, 3, 17, 18, 4, 5, 6)


@pytest.mark.parametrize("name", list(G.CASES))
def test_operands_are_what_the_util_says(ops, name):
    o = ops[name]
    M, N, K = G.CASES[name]
    A, W = o["A"], o["W"]
    assert A.shape == (M, K) and W.shape == (N, K) and o["bias"].shape == (N,) and o["res"].shape == (M, N)
    assert (np.count_nonzero(A, axis=1) <= G.NNZ).all()
    fam = {np.float32(s * (1 + u * 2.0 ** -9 + v * 2.0 ** -18)) for s in (1, -1) for u, v in G.PATTERNS}
    dense = W if name != G.IDENTITY_CASE else W[128:]
    assert set(np.unique(dense)) == fam                                       # dense in the family, every pattern and sign present
    if name == G.IDENTITY_CASE:
        assert np.array_equal(W[:128], np.eye(128, K, dtype=np.float32))
    # every term of every operand is a bfloat16 value, and the three add up to the operand
    for x in (A, W):
        t = G.split3(x)
        for term in t:
            assert np.array_equal(G.bf16_rn(term), term)
        assert np.array_equal(sum(term.astype(np.float64) for term in t), x.astype(np.float64))
    # the crafted rows
    for m in range(M):
        kind, row = G.row_kind(m), A[m]
        nz = row[row != 0]
        if kind == "family":
            assert len(nz) == G.NNZ and set(nz) <= fam
        elif kind == "zero":
            assert len(nz) == 0
        else:
            assert len(nz) == 4 and (np.nonzero(row)[0] % 4 == 3).all()       # on the coarse columns
            low = nz.view(np.uint32) & 0xFFFF
            assert (low == (0x8000 if kind == "tie" else 0)).all()
    if M >= 3:
        assert G.rows_of(M, "tie") and G.rows_of(M, "bf16") and G.rows_of(M, "zero")
    assert G.row_kind(0) == "tie"                                             # what M = 1 holds
    # the coarse columns of W carry no third term
    assert not G.split3(W[:, 3::4])[2].any()
    # every k is used (short K, from K / 8 family rows on); long K: the K-tile edges, and every K = 16 step of the loop
    used = np.nonzero(A.any(axis=0))[0]
    if K < G.LONG_K and M >= 63:
        assert len(used) == K
    if K >= G.LONG_K:
        assert {0, 15, 16, 31, 32, K - 33, K - 32, K - 1} <= set(used)
        assert set(used // 16) == set(range(K // 16))


@pytest.mark.parametrize("mode", list(G.MODES))
@pytest.mark.parametrize("name", list(G.CASES))
def test_products_are_exact_in_any_order(ops, name, mode):
    """Every product the mode forms is a multiple of 2^-18; the 22-bit condition holds; a float32 accumulation of the individual
    products, the bias and the residual in three random orders returns the int64 sum."""
    o = ops[name]
    A, W = o["A"], G.weights_for(mode, o["W"])
    m, k = np.nonzero(A)
    piles = []
    for at, wt in G.term_pairs(mode, A, W):
        p = at[m, k, None] * wt[:, k].T                                       # [nnz, N] individual products, 2^-36
        assert not (p & ((1 << G.UNIT) - 1)).any()
        piles.append(p >> G.UNIT)
    assert G.magnitude_units(mode, o) <= G.LIMIT_UNITS
    M, N, K = G.CASES[name]
    # [M, slots, N] float32: the products of row m in slots, then bias and residual
    per_row = np.bincount(m, minlength=M)
    slot = np.concatenate([np.arange(c) for c in per_row]) if len(m) else np.zeros(0, int)
    width = max(int(per_row.max()), 1)
    P = np.zeros((M, len(piles) * width + 2, N), np.float32)
    for i, p in enumerate(piles):
        P[m, i * width + slot] = G.from_units(p)
    P[:, -2] = o["bias"][None, :]
    P[:, -1] = o["res"]
    want = G.expected(mode, o, "bias_res")
    rs = np.random.RandomState(len(name) + G.MODES[mode])
    for _ in range(3):
        acc = np.zeros((M, N), np.float32)
        for s in rs.permutation(P.shape[1]):
            acc = (acc + P[:, s]).astype(np.float32)
        assert np.array_equal(acc.view(np.int32), want.view(np.int32))


def test_sixteen_non_zeros_trip_the_condition():
    """The family loosened to 16 non-zeros per row: 16.06 > 16, with or without bias and residual."""
    wide = G.make_operands("k64", nnz=16)
    assert (np.count_nonzero(wide["A"], axis=1) == 16).any()
    for mode in G.MODES:
        assert G.magnitude_units(mode, wide) > G.LIMIT_UNITS
        assert G.magnitude_units(mode, dict(wide, bias=np.zeros_like(wide["bias"]), res=np.zeros_like(wide["res"]))) > G.LIMIT_UNITS


@pytest.mark.parametrize("name", list(G.CASES))
def test_modes_differ_where_they_should(ops, name):
    """The six-product value is not the true product, the two-term value not the exact one: a seventh product, a fifth only, or a third
    activation term where two belong moves some element of every case.  (M = 1 is the tie row: two terms carry it whole, and on the
    coarse columns the six products are the true product -- its value is pinned, but these two differences need a family row.)"""
    o = ops[name]
    A, W = o["A"], o["W"]
    x3 = G.product_units("f32x3", A, W)
    true = G._sparse_matmul(G.units(A), G.units(W))
    exact, two = G.product_units("bf16_exact", A, W), G.product_units("bf16", A, W)
    assert np.array_equal(exact, G.product_units("f32", A, G.weights_for("f32", W)))
    if G.CASES[name][0] == 1:
        assert np.array_equal(x3, true) and np.array_equal(exact, two)
        return
    assert (x3 != true).any() and (two != exact).any() and (x3 != exact).any()
    # dropping any one of the six products, or doubling it, moves some element
    for a, w in G.term_pairs("f32x3", A, W):
        assert G._sparse_matmul(a, w).any()


def test_identity_case_reproduces_the_tie_rows(ops):
    o = ops[G.IDENTITY_CASE]
    M, N, K = G.CASES[G.IDENTITY_CASE]
    tie = G.rows_of(M, "tie")
    assert len(tie) >= 8 and (o["A"][tie][:, 128:] == 0).all()                # all their non-zeros meet the identity block
    for mode in ("f32x3", "bf16_exact", "f32"):
        assert np.array_equal(G.expected(mode, o, "none")[:, :128].view(np.int32), o["A"][:, :128].view(np.int32))
    a0, a1, _ = G.split3(o["A"])
    assert np.array_equal(G.expected("bf16", o, "none")[:, :128], (a0 + a1)[:, :128])
    assert (G.expected("bf16", o, "none")[:, :128] != o["A"][:, :128]).any()    # the family rows' third term


def test_activation_operands_are_exact_in_every_mode(ops):
    for name in ("k96", "m1", "long768"):
        act = G.activation_operands(ops[name])
        assert set(np.unique(act["A"])) <= {-1.0, 0.0, 1.0} and set(np.unique(act["W"])) <= {-1.0, 0.0, 1.0}
        v = G.expected("f32", act, "bias")
        for mode in ("bf16", "bf16_exact", "f32x3"):
            assert np.array_equal(G.expected(mode, act, "bias"), v)
        assert np.abs(v).max() <= 16.1


def test_activation_references():
    v = np.array([-12.0, -1.0, 0.0, 0.5, 3.0, 12.0])
    assert np.allclose(G.qgelu64(v), v / (1 + np.exp(-1.702 * v)), rtol=0, atol=0)
    assert abs(G.gelu64(1.0) - 0.8413447460685429) < 1e-15 and G.gelu64(0.0) == 0.0 and abs(G.gelu64(-1.0) + 0.15865525393145707) < 1e-15


def test_case_table_reaches_every_kernel_form():
    """Through tstar_gemm_plan (pure, no GPU): the (case, mode, tile_cfg) of the GPU test reach kinds 128, 64N, 64 and hybrid in all four
    weight modes, the wide tile in the two-term and f32x3 modes, the wide tile with streamed weights in the two-term mode only -- hybrid
    and wide each with m_split > 0 and a ragged rest -- and tile_cfg -1 lands where AUTO_PLAN says."""
    from tstar_amd import _lib
    lib = _lib.load()
    reached, ragged, refused = set(), set(), set()
    for name, (M, N, K) in G.CASES.items():
        for mode in G.MODES:
            for cfg in G.tile_cfgs(mode, M):
                plan = G.gemm_plan(lib, mode, M, N, cfg)
                if plan is None:
                    refused.add((name, mode, cfg))
                    continue
                kind, m_split = plan
                reached.add((mode, kind))
                if kind >= G.HYBRID and 0 < m_split < M and (M - m_split) % 64 != 0:
                    ragged.add((mode, kind))
                if cfg == -1:
                    assert plan == G.AUTO_PLAN[name], (name, mode, plan)
            assert G.gemm_plan(lib, mode, M, N, 6, wq=0) is None                  # the pre-packed entry has no fragment-packed plane
    assert reached == G.REACHABLE
    assert ragged == {(m, k) for m, k in G.REACHABLE if k >= G.HYBRID}
    # only tile_cfg 6 is ever refused: without a full 128-row panel, or where N % 256 != 0
    assert refused == {(name, "bf16", 6) for name, (M, N, K) in G.CASES.items() if M < 128 or N % 256}
