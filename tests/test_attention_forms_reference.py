"""CPU companion of tests/test_gpu_attention_forms.py: the crafted attention operands are what tests/attention_forms_util.py says, their
closed form is the softmax attention, the conditions that make it exact hold on the operands themselves, every kernel form is reached by
the case table, and a kernel with one of the listed defects could not pass check_indicator."""
import numpy as np
import pytest

import attention_forms_util as U

torch = pytest.importorskip("torch")


def _launches(kind, T, B, heads, mode=0):
    n = len(U.rounds(B, heads, mode)) if kind == "indicator" else 1
    for rnd in range(n):
        yield rnd, U.launch_heads(kind, T, B, heads, rnd, mode)


def _mode0_heads(kind, T_list=None):
    for T, B, heads in U.CASES:
        if T_list is None or T in T_list:
            for rnd, hd in _launches(kind, T, B, heads):
                for bh, x in hd.items():
                    yield T, rnd, bh, x


def _mode1_heads(kind):
    for T in U.MODE1_T:
        km = U.mode1_key_masks(T)
        for rnd, hd in _launches(kind, T, U.MODE1_B, U.MODE1_HEADS, 1):
            for (b, h), x in hd.items():
                yield T, rnd, (b, h), x, km[b]


# ------------------------------------------------------------------------------------------------ the table and the forms
def test_case_table_is_the_issue_s():
    assert [c[0] for c in U.CASES] == [1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 160, 161, 193, 255, 257, 320, 337, 577]
    assert all((B, heads) == (2, 2) for T, B, heads in U.CASES if T != 577) and U.CASES[-1] == (577, 1, 2)
    assert U.MODE1_T == (1, 16, 33, 77, 130) and U.MODE1_B == 4
    assert U.T16_OFF_T == (65, 193)
    assert U.C_Q == 2048.0 and U.V_MAX == 2000 and U.GUARD_ROWS == 64
    assert U.GRADED_TOL == {"f32": 2e-5, "x3": 2e-5, "split": 2e-4} and U.REL_BOUND == 2.0 ** -22
    for T in U.MODE1_T:
        lens = U.mode1_lengths(T)
        km = U.mode1_key_masks(T)
        assert lens[0] == 1 and lens[1] == T and all(1 <= n <= T for n in lens)
        if T >= 16:
            assert 1 < lens[2] < lens[3] < T
        assert (km[:3].sum(1) == lens[:3]).all() and all((km[i, :lens[i]] == 1).all() for i in range(3))      # right-padded
        assert km[:, 0].all()                                                                              # key 0 valid everywhere
        assert (km[3, :lens[3]] == np.resize([1, 0, 1, 1, 0], lens[3])).all() and not km[3, lens[3]:].any()
        if T >= 16:
            assert (km[3, :lens[3]] == 0).any()


def test_forms_restate_the_launch_code():
    f = U.forms
    assert f("f32", 577) == ("straggler", "tail16") and f("f32", 577, t16=False) == ("straggler", "inactive_waves")
    assert f("split", 577) == ("straggler", "inactive_waves") and f("x3", 577) == ("straggler/paired", "inactive_waves")
    assert f("f32", 65) == ("straggler", "tail16") and f("f32", 65, mode=1) == ("causal_multi_tile", "inactive_waves")
    assert f("f32", 1) == ("straggler", "one_query") and f("f32", 129) == ("straggler", "one_query")
    assert f("f32", 337) == ("masked", "inactive_waves") and f("f32", 128) == ("unmasked", "all_waves") and f("f32", 97) == ("straggler", "all_waves")
    assert f("f32", 96) == ("unmasked", "inactive_waves") and f("f32", 16, 1) == ("causal_one_tile", "inactive_waves")
    # x3: pairs run while kb + 3 < nkb, so from four MFMA tiles on; 97 = 3 tiles + the straggler, 127 = 4 tiles
    assert f("x3", 97)[0] == "straggler/peeled" and f("x3", 127)[0] == "masked/paired" and f("x3", 96)[0] == "unmasked/peeled"
    assert f("x3", 129)[0] == "straggler/paired" and f("x3", 128)[0] == "unmasked/paired"
    assert [U.mfma_tiles(T) for T in (1, 32, 33, 34, 577)] == [0, 1, 1, 2, 18] and U.mfma_tiles(33, 1) == 2


@pytest.mark.parametrize("kernel", U.KERNELS)
def test_every_reachable_form_is_hit_twice(kernel):
    keys, queries = U.reachable_forms(kernel)
    assert ("tail16" in queries) == (kernel == "f32") and len(keys) == (6 if kernel == "x3" else 5 if kernel == "f32" else 3)
    hit_k = {k: 0 for k in keys}
    hit_q = {q: 0 for q in queries}
    for T, mode in U.table_rows(kernel):
        k, q = U.forms(kernel, T, mode)
        hit_k[k] += 1
        hit_q[q] += 1
    assert min(hit_k.values()) >= 2, hit_k
    assert min(hit_q.values()) >= 2, hit_q
    # the knob-off child sends both of its T through the generic last block
    if kernel == "f32":
        assert all(U.forms("f32", T) == ("straggler", "tail16") and U.forms("f32", T, t16=False)[1] == "inactive_waves" for T in U.T16_OFF_T)


# ------------------------------------------------------------------------------------------------ the operands
def _wave_tiles(T, kernel_t16):
    """Query ranges that one wave scores with MFMAs: 32-query tiles, and the 16-query tiles of the f32 tail workgroup."""
    tiles = [range(q0, min(q0 + 32, T)) for q0 in range(0, T, 32)]
    if kernel_t16 and T % 128 == 65:
        tiles += [range(T - 65 + 16 * w, T - 65 + 16 * w + 16) for w in range(4)]
    return tiles


@pytest.mark.parametrize("T,B,heads", U.CASES)
def test_indicator_operands_are_what_the_util_says(T, B, heads):
    named_at_last = set()
    fill_seen = set()
    for rnd, hd in _launches("indicator", T, B, heads):
        fill = U.rounds(B, heads)[rnd][0]
        for x in hd.values():
            assert x.K.dtype == x.V.dtype == x.Q.dtype == np.float32 and x.K.shape == x.V.shape == x.Q.shape == (T, 64)
            assert np.isin(x.K, (0.0, 1.0)).all()
            assert ((x.Q != 0).sum(1) == 1).all() and (x.Q[np.arange(T), x.qd] == 2048.0).all()
            Vi = x.V.astype(np.int64)
            assert (Vi == x.V).all() and (np.abs(Vi) <= 2000).all() and (Vi != 0).all()
            # collision-free: along every key row and along every dim column; below 63 keys over the whole head
            assert all(len(set(r)) == 64 for r in Vi) and all(len(set(c)) == T for c in Vi.T)
            if T <= 62:
                assert len(set(Vi.ravel())) == T * 64
            ns = U.named_sets(T)
            for d, ks in enumerate(x.sets):
                assert tuple(np.flatnonzero(x.K[:, d])) == ks
                if d < U.N_NAMED:
                    assert ks == ns[U.NAMED[d]]
                else:
                    assert len(ks) == min((1, 2, 4, 8)[(d - 16) % 4], T) and len(set(ks)) == len(ks)
            if fill:
                fill_seen |= set(x.qd.tolist())
                assert (x.qd >= U.N_NAMED).all()
                continue
            for tile in _wave_tiles(T, True):
                if len(tile) >= U.N_NAMED:
                    assert set(x.qd[list(tile)].tolist()) == set(range(U.N_NAMED)), "a wave tile misses a named set"
            named_at_last.add(int(x.qd[T - 1]))
    assert named_at_last == set(range(U.N_NAMED)), "query T - 1 does not meet every named set"
    if T >= 48:
        assert fill_seen == set(range(U.N_NAMED, 64))


@pytest.mark.parametrize("T", sorted({c[0] for c in U.CASES} | set(U.MODE1_T)))
def test_named_sets_are_the_listed_ones(T):
    s = U.named_sets(T)
    last, lt = T - 1, (T - 1) // 32
    assert s["last"] == (last,) and s["first"] == (0,) and set(s["ends"]) == {0, last} and s["empty"] == ()
    assert s[U.ALIASES["masked_last_and_0"]] == s["ends"]
    assert s["last_tile_first"] == (32 * lt,)
    assert len(s["each_tile"]) == lt + 1 and [k // 32 for k in s["each_tile"]] == list(range(lt + 1))
    assert s["tile_firsts"] == tuple(range(0, T, 32))
    assert all(k // 32 == lt for k in s["last_tile_only"]) and last in s["last_tile_only"]
    if T >= 8:
        lm = (T - 2) // 32
        assert len(s["last_mfma_tile_only"]) == min(2, T - 32 * lm) == 2 and all(k // 32 == lm for k in s["last_mfma_tile_only"])
    if T >= 32:
        ts = U.mfma_tiles(T) // 2
        assert ts < U.mfma_tiles(T) or T == 33
        assert sorted((k - 32 * ts) // 8 for k in s["shares_all"]) == [0, 1, 2, 3]
        for w in range(4):
            assert len(s[f"share_only_{w}"]) == 2 and all((k - 32 * ts) // 8 == w for k in s[f"share_only_{w}"])
    if T >= 64:
        a, b = s["pair16"]
        c, d = s["pair4"]
        assert b - a == 16 and a // 32 == b // 32 and d - c == 4 and c // 32 == d // 32
    assert all(all(0 <= k < T for k in ks) for ks in s.values())


@pytest.mark.parametrize("T,B,heads", U.CASES)
def test_graded_operands(T, B, heads):
    lv = np.array(U.LEVELS, np.float32)
    import struct
    for v in lv:                                            # bfloat16-exact: the low 16 bits of the float32 are zero
        assert struct.unpack("<I", struct.pack("<f", float(v)))[0] & 0xFFFF == 0
    assert list(lv * 256) == [256, 255, 254, 253]
    for _, hd in _launches("graded", T, B, heads):
        for x in hd.values():
            assert np.isin(x.K, np.concatenate([[0.0], lv])).all()
            assert ((x.Q != 0).sum(1) == 1).all() and (x.Q.max(1) == 2048.0).all()
            lm = max(T - 2, 0) // 32
            for d in range(64):
                top = np.flatnonzero(x.K[:, d] == 1.0)
                assert len(top) == 1, "one top-level key per dim"
                assert top[0] == T - 1 if d % 2 else top[0] // 32 == lm                   # on the straggler key / in the last MFMA tile
                if T >= 16:
                    assert (np.isin(x.K[:, d], lv[1:])).sum() >= 8                        # weights that are neither 0 nor 1
            if T >= 64:
                assert len(set(x.qd.tolist())) == 64


# ------------------------------------------------------------------------------------------------ the closed form
def _torch_attention(Q, K, V, valid):
    s = (torch.from_numpy(Q).double() @ torch.from_numpy(K).double().T) * 0.125
    s = s + torch.zeros_like(s).masked_fill(~torch.from_numpy(valid), float("-inf"))
    return (torch.softmax(s, dim=-1) @ torch.from_numpy(V).double()).numpy()


def _assert_closed_form(x, valid, what):
    exp = U.expected_indicator(x, valid)
    rows = exp.compared
    assert (rows == valid.any(1)).all()
    ref = _torch_attention(x.Q, x.K, x.V, valid)
    err = np.abs(ref[rows] - exp.mean[rows])
    assert (err <= 1e-9 * np.maximum(np.abs(exp.mean[rows]), 1.0)).all(), (what, err.max())
    if what[1] == 0:                                        # the numpy reference the graded family uses says the same (first round)
        assert np.allclose(U.attention64(x.Q, x.K, x.V, valid)[rows], ref[rows], rtol=1e-12, atol=1e-9)
    return exp


def test_closed_form_is_softmax_attention_mode0():
    uniform = set()
    for T, rnd, bh, x in _mode0_heads("indicator"):
        exp = _assert_closed_form(x, U.valid_matrix(T), (T, rnd, bh))
        assert exp.compared.all()
        if (exp.count == T).any():
            uniform.add(T)
    assert uniform == {c[0] for c in U.CASES}, "a T without a uniform row (the empty set)"


def test_closed_form_is_softmax_attention_mode1():
    seen_bound = seen_bit = 0
    for T, rnd, bh, x, km in _mode1_heads("indicator"):
        valid = U.valid_matrix(T, 1, km)
        assert valid[:, 0].all()                            # key 0 is valid for every query: every row is compared
        exp = _assert_closed_form(x, valid, (T, rnd, bh))
        seen_bit += int(U.is_pow2(exp.count).sum())
        seen_bound += int((~U.is_pow2(exp.count)).sum())
    assert seen_bit > 1000 and seen_bound > 1000


# ------------------------------------------------------------------------------------------------ the exactness conditions
def _bf16_rn(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32)


def test_exactness_conditions_hold_on_the_operands():
    # the tied score: ONE product, far enough above 0 that exp2 of the gap is below float32's smallest subnormal
    s = np.float32(U.C_Q) * U.SC32
    assert float(s) == U.C_Q * float(U.SC32) and 368 < s < 370, "C_Q sc is exact (a power of two times sc)"
    assert -float(s) < -149 - 24
    # its three bfloat16 terms (x3) add back to it exactly; its two terms (split) are the 16-bit q both split paths use
    t0 = _bf16_rn(s)
    t1 = _bf16_rn(np.float32(s - t0))
    t2 = _bf16_rn(np.float32(np.float32(s - t0) - t1))
    assert np.float32(np.float32(t2 + t1) + t0) == s and np.float32(np.float32(t0 + t1) + t2) == s
    assert float(t0[0]) + float(t1[0]) > 149 + 24
    for gen in (_mode0_heads("indicator"), ((T, r, bh, x) for T, r, bh, x, _ in _mode1_heads("indicator"))):
        for T, rnd, bh, x in gen:
            Vi = x.V.astype(np.int64)
            # every partial sum of V over any subset of the keys is bounded by the sum of |V|: below 2^24
            assert np.abs(Vi).sum(0).max() < 1 << 24
            hi = _bf16_rn(x.V)
            lo = _bf16_rn(x.V - hi)
            assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), x.V.astype(np.float64)), "V is two bfloat16 terms"
            assert np.array_equal(hi, np.rint(hi)) and np.array_equal(lo, np.rint(lo)), "and they are integers"
    # power-of-two means are float32 values (check_indicator asserts it per row as well)
    x = U.launch_heads("indicator", 577, 1, 2)[0, 0]
    exp = U.expected_indicator(x, U.valid_matrix(577))
    bit = U.is_pow2(exp.count)
    assert bit.any() and (~bit).any()
    assert np.array_equal(exp.mean[bit].astype(np.float32).astype(np.float64), exp.mean[bit])


def test_check_indicator_accepts_the_closed_form_and_its_roundings():
    x = U.launch_heads("indicator", 193, 2, 2)[1, 1]
    exp = U.expected_indicator(x, U.valid_matrix(193))
    S = np.rint(exp.mean * exp.count[:, None]).astype(np.float32)                       # the exact integer sums
    for got in ((S * (np.float32(1) / exp.count.astype(np.float32))[:, None]).astype(np.float32),      # sum * fl(1 / l), the 32-query forms
                (S / exp.count.astype(np.float32)[:, None]).astype(np.float32)):                        # fl(sum / l), the straggler merge
        nbit, nbnd = U.check_indicator(got, exp)
        assert nbit > 0 and nbnd > 0 and nbit + nbnd == 193
    bad = exp.mean.astype(np.float32)
    bad[5, 7] = np.nextafter(bad[5, 7], np.float32(np.inf))
    assert U.is_pow2(exp.count[5])
    with pytest.raises(AssertionError):
        U.check_indicator(bad, exp)
    bad = exp.mean.astype(np.float32)
    bad[0, 0] = np.float32("nan")
    with pytest.raises(AssertionError):
        U.check_indicator(bad, exp)
    q = int(np.flatnonzero(~U.is_pow2(exp.count))[0])
    bad = exp.mean.astype(np.float32)
    bad[q, 3] += np.float32(4 * U.REL_BOUND) * np.float32(exp.absmean[q, 3])
    with pytest.raises(AssertionError):
        U.check_indicator(bad, exp)


# ------------------------------------------------------------------------------------------------ wrong-kernel models
def _noticed(model, T, B, heads, mode=0, per_image=False, **kw):
    """The model changes the expectation beyond the asserted bound at one row at least -- of some launch of the case, or (per_image) of
    every image that `kw` selects."""
    hit = {}
    for rnd, hd in _launches("indicator", T, B, heads, mode):
        km = U.mode1_key_masks(T) if mode else None
        for (b, h), x in hd.items():
            valid = U.valid_matrix(T, mode, km[b] if mode else None)
            exp = U.expected_indicator(x, valid)
            wrong = model(x, km[b] if kw.get("takes_mask") else valid, *kw.get("args", ()))
            hit[b] = hit.get(b, False) or bool(U.differs_beyond_bound(wrong[:T], exp).any())
    return hit if per_image else any(hit.values())


MODE0 = [(T, B, heads) for T, B, heads in U.CASES]


def test_model_masked_keys_counted():
    for T, B, heads in MODE0:
        if T % 32 not in (0, 1):
            assert _noticed(U.model_masked_keys_counted, T, B, heads), T
            assert _noticed(U.model_masked_keys_counted, T, B, heads, args=(True,)), T


def test_model_last_key_dropped_or_doubled():
    for T, B, heads in MODE0:
        if T >= 2:
            assert _noticed(U.model_last_key_dropped, T, B, heads), T
            assert _noticed(U.model_last_key_twice, T, B, heads), T


def test_model_causal_strict_and_mask_mod_tile():
    for T in U.MODE1_T:
        if T >= 2:
            hit = _noticed(U.model_causal_strict, T, U.MODE1_B, U.MODE1_HEADS, 1, per_image=True, takes_mask=True)
            assert all(hit.values()), (T, hit)
        if T > 32:
            hit = _noticed(U.model_mask_mod_tile, T, U.MODE1_B, U.MODE1_HEADS, 1, per_image=True, takes_mask=True)
            lens = U.mode1_lengths(T)
            # noticed in every image whose mask is not periodic in the tile: all but the full-length one
            assert all(hit[b] for b in range(4) if lens[b] < T), (T, hit)


def test_model_share_dropped():
    for T, B, heads in MODE0:
        if U.forms("f32", T)[1] == "tail16":
            for w in range(4):
                assert _noticed(U.model_share_dropped, T, B, heads, args=(w,)), (T, w)


def test_model_keys_swapped():
    for T, B, heads in MODE0:
        if T >= 17:
            assert _noticed(U.model_keys_swapped, T, B, heads, args=(16,)), T
        if T >= 5:
            assert _noticed(U.model_keys_swapped, T, B, heads, args=(4,)), T


def test_model_row_late():
    for T, B, heads in MODE0:
        if T >= 2:
            assert _noticed(U.model_row_late, T, B, heads), T
    for T in U.MODE1_T:
        if T >= 2:
            assert _noticed(U.model_row_late, T, U.MODE1_B, U.MODE1_HEADS, 1), T
