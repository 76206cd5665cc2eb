"""The OWL-ViT / OWLv2 detector FRONT, kernel by kernel, through the diagnostic entries tstar_gemm_patch_embed,
tstar_owl_debug_embed and tstar_owl_debug_text (the launches owl_forward_heads and tstar_owl_set_queries make, same arguments).

A  The patch-embedding GEMM -- gemm_f32 with pos != nullptr: the PATCH epilogue remaps GEMM row (b, p) to token row
   b (np + 1) + 1 + p, adds position row 1 + p and leaves the class-token rows alone -- in all four weight modes and every tile
   form (three grids, hybrid, the wide tile and the wide tile with streamed weights, each with its guarded last panel).  The
   reference is BIT EQUALITY with float32(C + pos[1 + p]), C from the public plain entry of the same mode (the PATCH epilogue
   computes acc + 0.f and then + pos; the plain one stores acc + 0.f; single float32 additions, nothing to contract), on a token
   buffer pre-filled with a NaN payload whose class-token rows and 128 spare rows must keep their bits.  S1..S4 run every
   tile_cfg of every mode; the launcher's own ladder runs tile_cfg -1 at production M, and the form tstar_gemm_plan reports is
   asserted next to each result (owl_front_util.LADDER_PLAN, pinned on the CPU by tests/test_owl_front_reference.py).
   S1..S4 are also held against a float64 product by the criteria tests/test_gpu_kernels.py applies to each mode, with |pos|
   added to the magnitude term, so the test stands without the plain kernel.
B  The tower entry on handles of three small geometries in every weight mode: the patch rows bit-equal to (plain GEMM of the mode
   on the state dict's patch_w) + the handle's -- resampled -- position rows, the class rows to class_emb + pos[0]; the in-place
   pre-LayerNorm bit-equal to tstar_layernorm_f32 out of place and within owl_tail_util.bound of float64.
C  The text tower against the numpy float64 tower of owl_front_util (the bf16 modes against the tower with the GEMM weights
   rounded to bf16), bound = owl_tail_util.bound with oracle/owl_ref.text_query_embeds as the float32 yardstick.
   The two-term mode ("bf16") carries the activations of the vision tower as two bf16 terms (2^-17 relative per GEMM), which a
   float32 yardstick cannot meet over the text tower's 49 GEMMs (measured 7.3e-07 ... 1.1e-06 against bounds of 3.4e-07 ... 5.0e-07);
   the text tower of such a handle therefore runs the exact three-term split on the same bf16 plane, and its embeddings equal the
   bf16_exact handle's bit for bit (test_two_term_handle_runs_the_text_tower_exactly).

Every tolerance-based check prints kernel error / float32 yardstick's error -> bound under `pytest -s`; profiles/owl_front_tests.md has
the table of one run.  Nothing is fitted to what the kernels return.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import owl_front_util as Fr
import owl_tail_util as T

pytestmark = pytest.mark.gpu


def library_shapes():
    """(mode, B, np, N, K, tile_cfg) of every tstar_gemm_patch_embed call of part A, so that a test without a GPU
    (tests/test_host_logic.py::test_every_patch_embed_form_is_gpu_tested) can ask the launch plan which kernel each one runs."""
    return Fr.patch_cases()


@pytest.fixture(scope="module")
def lib():
    from tstar_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------ A: the PATCH epilogue
@functools.lru_cache(maxsize=None)
def _inputs(B, np_, N, K):
    return tuple(t.cuda() for t in Fr.patch_inputs(B, np_, N, K, seed=B * 131 + np_ + N + K))


def _plain(lib, mode, dA, dW, M, N, K, cfg=-1):
    """C [M, N] of the public no-bias entry of the mode (every tile choice of a mode gives the same bits: tests/test_gpu_kernels.py)."""
    from tstar_amd import _lib
    dC = torch.full((M, N), float("nan"), device="cuda")
    _lib.check(getattr(lib, Fr.PLAIN_ENTRY[mode])(dA.data_ptr(), dW.data_ptr(), dC.data_ptr(), None, None, M, N, K, 0, cfg, _st()))
    torch.cuda.synchronize()
    return dC


def _sentinel(B, np_, N):
    return torch.full((B * (np_ + 1) + Fr.SPARE_ROWS, N), Fr.SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _want(dC, dpos, B, np_, N):
    """The token buffer the entry must leave: float32(C + pos[1 + p]) in the patch rows, the sentinel everywhere else."""
    w = _sentinel(B, np_, N)
    w[:B * (np_ + 1)].view(B, np_ + 1, N)[:, 1:] = dC.view(B, np_, N) + dpos[1:]
    return w


def _patch_embed(lib, dA, dW, dpos, B, np_, N, K, mode, cfg):
    dX = _sentinel(B, np_, N)
    rc = lib.tstar_gemm_patch_embed(dA.data_ptr(), dW.data_ptr(), dX.data_ptr(), dpos.data_ptr(), B, np_, N, K, Fr.MODES[mode], cfg, _st())
    torch.cuda.synchronize()
    return rc, dX


def _bit_report(dX, want, B, np_, label):
    """None when the token buffer has the wanted bits, else what differs."""
    if torch.equal(_bits(dX), _bits(want)):
        return None
    ntok = np_ + 1
    bad = (_bits(dX) != _bits(want)).any(1).cpu().numpy()
    rows = np.flatnonzero(bad)
    spare = rows[rows >= B * ntok]
    tok = rows[rows < B * ntok]
    cls, patch = tok[tok % ntok == 0], tok[tok % ntok != 0]
    return (f"{label}: {len(patch)} patch rows differ from float32(C + pos) (first (b, p): {[(int(r) // ntok, int(r) % ntok - 1) for r in patch[:6]]}), "
                         f"{len(cls)} class-token rows written (images {[int(r) // ntok for r in cls[:6]]}), {len(spare)} spare rows written")


def _assert_same_bits(dX, want, B, np_, label):
    report = _bit_report(dX, want, B, np_, label)
    assert report is None, report


def _judge64(lib, mode, name, s, out):
    """The criterion tests/test_gpu_kernels.py applies to the mode (test_gemm_tile_configs / test_gemm_bf16_weights_exact_split /
    test_gemm_bf16_weights_two_term / the `worst` criterion of test_gemm_f32x3), against float64 A W^T + pos."""
    B, np_, N, K = s["B"], s["np"], s["N"], s["K"]
    dA, dW, dpos = _inputs(B, np_, N, K)
    ref, mag = Fr.patch_ref64(dA.cpu(), dW.cpu(), dpos.cpu(), B, np_, mode)
    out = out.cpu().to(torch.float64)
    assert torch.isfinite(out).all()

    def rows_of(mode32, dW32):
        rc, dX = _patch_embed(lib, dA, dW32, dpos, B, np_, N, K, mode32, -1)
        assert rc == 0
        return dX[:B * (np_ + 1)].view(B, np_ + 1, N)[:, 1:].reshape(B * np_, N).cpu().to(torch.float64)

    if mode == "f32":
        err, lim = (out - ref).abs().max().item(), 3e-5 * max(1.0, ref.abs().max().item())
        print(f"A {name} f32: max err {err:.3g} < {lim:.3g}")
        assert err < lim
    elif mode == "bf16_exact":
        err = ((out - ref).abs() / mag).max().item()
        err32 = ((rows_of("f32", dW.to(torch.bfloat16).to(torch.float32)) - ref).abs() / mag).max().item()   # the native f32 tile on the same bf16-valued weights
        print(f"A {name} bf16_exact: max err / (sum|aw| + |pos|) {err:.3g} < 1e-6 and < 3 x {err32:.3g} + 1e-7")
        assert err < 1e-6 and err < 3 * err32 + 1e-7, (err, err32)
    elif mode == "bf16":
        err = ((out - ref).abs() / mag).max().item()
        rms = ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
        print(f"A {name} bf16: max err / (sum|aw| + |pos|) {err:.3g} < 2^-17 + 1e-6; rms {rms:.3g} < 8e-6")
        assert err < 2.0 ** -17 + 1e-6 and rms < 8e-6, (err, rms)
    else:
        worst = ((out - ref).abs() / mag).max().item()
        worst32 = ((rows_of("f32", dW) - ref).abs() / mag).max().item()
        print(f"A {name} f32x3: max err / (sum|aw| + |pos|) {worst:.3g} < 2^-19 and < 2 x {worst32:.3g} + 2^-23")
        assert worst < 2.0 ** -19 and worst < 2 * worst32 + 2.0 ** -23, (worst, worst32)


@pytest.mark.parametrize("mode", list(Fr.MODES))
@pytest.mark.parametrize("name", list(Fr.SHAPES))
def test_a_patch_epilogue_every_tile(lib, name, mode):
    """S1..S4 in one weight mode at every tile_cfg the mode accepts: the token buffer equals float32(C_plain + pos) in its patch rows
    and the sentinel elsewhere, bit for bit; a tile_cfg the plan refuses is refused by the entry, which then launches nothing."""
    s = Fr.SHAPES[name]
    B, np_, N, K = s["B"], s["np"], s["N"], s["K"]
    M = B * np_
    dA, dW, dpos = _inputs(B, np_, N, K)
    want = _want(_plain(lib, mode, dA, dW, M, N, K), dpos, B, np_, N)
    assert torch.isfinite(want[:B * (np_ + 1)].view(B, np_ + 1, N)[:, 1:]).all()
    kinds, first, wrong = set(), None, []
    for cfg in Fr.tile_cfgs(mode):
        plan = Fr.gemm_plan(lib, mode, M, N, np_, cfg)
        rc, dX = _patch_embed(lib, dA, dW, dpos, B, np_, N, K, mode, cfg)
        if plan is None:
            assert rc == 1 and b"tstar_gemm_patch_embed" in lib.tstar_last_error(), (cfg, rc, lib.tstar_last_error())
            assert (_bits(dX) == Fr.SENTINEL).all(), cfg
            continue
        assert rc == 0, (cfg, lib.tstar_last_error())
        wrong.append(_bit_report(dX, want, B, np_, f"{name} {mode} tile_cfg {cfg} (kind {plan[0]}, m_split {plan[1]})"))
        kinds.add(plan[0])
        first = dX if first is None else first
    assert not any(wrong), "\n".join(w for w in wrong if w)
    want_kinds = {0, 1, 2, 3} | ({4} if mode in ("bf16", "f32x3") and N % 256 == 0 else set()) | ({5} if mode == "bf16" and N % 256 == 0 else set())
    assert kinds == want_kinds, kinds
    _judge64(lib, mode, name, s, first[:B * (np_ + 1)].view(B, np_ + 1, N)[:, 1:].reshape(M, N))


@pytest.mark.parametrize("mode", list(Fr.MODES))
@pytest.mark.parametrize("B", Fr.LADDER_B)
def test_a_launchers_own_ladder(lib, B, mode):
    """tile_cfg -1 at production M (576 patches, N = 768) and K = 64: the form the launcher picks for this batch in this mode -- asserted
    against the expected table, so that a change of launch policy fails here instead of hollowing the case out -- gives the same bits."""
    np_, N, K = Fr.LADDER["np"], Fr.LADDER["N"], Fr.LADDER["K"]
    M = B * np_
    plan = Fr.gemm_plan(lib, mode, M, N, np_, -1)
    assert plan == Fr.LADDER_PLAN[B][mode], (plan, Fr.LADDER_PLAN[B][mode])
    dA, dW, dpos = _inputs(B, np_, N, K)
    want = _want(_plain(lib, mode, dA, dW, M, N, K, cfg=2 if plan[0] == Fr.GRID_64N else 1), dpos, B, np_, N)   # the plain entry on another tile
    rc, dX = _patch_embed(lib, dA, dW, dpos, B, np_, N, K, mode, -1)
    assert rc == 0, lib.tstar_last_error()
    _assert_same_bits(dX, want, B, np_, f"ladder B={B} {mode} (kind {plan[0]}, m_split {plan[1]})")


# --------------------------------------------------------------------------------------------- B: the tower entry on a handle
GEOMETRIES = {"vit32": ("owlvit", None, (64, 96), 7), "vit16": ("owlvit", 16, (16, 16), 2), "v2": ("owlv2", None, (16, 16), 2)}


@functools.lru_cache(maxsize=None)
def _front_blob(geom, with_text=False):
    family, patch, size, ntok = GEOMETRIES[geom]
    g, sd, vb, tb, w = Fr.front_blob(family, patch, size, with_text)
    assert g.ntok == ntok
    return g, vb, tb, w


def _scorer(geom, mode, with_text=False, max_batch=4):
    from tstar_amd.owl import OwlScorer
    family, patch, size, _ = GEOMETRIES[geom]
    g, vb, tb, w = _front_blob(geom, with_text)
    return SimpleNamespace(scorer=OwlScorer(vb, tb, max_batch=max_batch, weights_mode=mode, patch_size=patch, input_size=size, family=family), g=g, w=w)


def _embed(lib, env, dP, B, stage):
    from tstar_amd import _lib
    rows = B * env.g.ntok
    dx = torch.full((rows + 8, Fr.D), Fr.SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    _lib.check(lib.tstar_owl_debug_embed(env.scorer._h, dP.data_ptr(), B, stage, dx.data_ptr(), _st()), "tstar_owl_debug_embed")
    torch.cuda.synchronize()
    assert (_bits(dx[rows:]) == Fr.SENTINEL).all()
    return dx[:rows]


@pytest.mark.parametrize("mode", list(Fr.MODES))
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_e_tower_entry(lib, geom, mode):
    """E1 (stage 0) and E2 (stage 1) at B = 1 and 3 on one handle."""
    from tstar_amd import _lib
    env = _scorer(geom, mode)
    try:
        g, w = env.g, env.w
        npatch, ntok, pk = g.npatch, g.ntok, g.patch_k
        dW, dpos = _dev(w["patch_w"]), _dev(w["pos"])
        dlw, dlb = _dev(w["pre_ln_w"]), _dev(w["pre_ln_b"])
        cls_row = _dev((w["class_emb"] + w["pos"][0]).astype(np.float32))
        for B in (1, 3):
            dP = _dev(Fr.embed_patches(g, B))
            x0 = _embed(lib, env, dP, B, 0)
            # E1: the handle's weight plane of its mode, its patch_k, its (resampled) position table
            C = _plain(lib, mode, dP, dW, B * npatch, Fr.D, pk)
            want = torch.empty((B, ntok, Fr.D), device="cuda")
            want[:, 1:] = C.view(B, npatch, Fr.D) + dpos[1:]
            want[:, 0] = cls_row
            diff = (_bits(x0) != _bits(want.view(B * ntok, Fr.D))).any(1).nonzero().flatten().tolist()
            assert not diff, f"E1 {geom} {mode} B={B}: token rows {diff[:8]} differ"
            # E2: the pre-LayerNorm in place = out of place, and both within the bound of float64
            x1 = _embed(lib, env, dP, B, 1)
            y = torch.full_like(x0, float("nan"))
            _lib.check(lib.tstar_layernorm_f32(x0.data_ptr(), y.data_ptr(), dlw.data_ptr(), dlb.data_ptr(), B * ntok, Fr.D, _st()))
            torch.cuda.synchronize()
            assert torch.equal(_bits(x1), _bits(y)), f"E2 {geom} {mode} B={B}: in place differs from out of place"
            x0h = x0.cpu().numpy()
            ref = T.ln64(x0h, w["pre_ln_w"], w["pre_ln_b"])
            f32 = torch.nn.functional.layer_norm(torch.from_numpy(x0h), (Fr.D,), torch.from_numpy(w["pre_ln_w"]), torch.from_numpy(w["pre_ln_b"]), 1e-5).numpy()
            b, m = T.bound(f32, ref)
            got = x1.cpu().numpy()
            e = float(np.abs(got - ref).max())
            print(f"E2 {geom} {mode} B={B}: {e:.2g} / {m:.2g} -> {b:.2g}")
            assert np.isfinite(got).all() and e <= b, (e, b)
            if npatch >= 6:
                r = {k: 1 + p for k, p in Fr.E2_ROWS.items()}
                assert (x0h[r["const"]] == np.float32(Fr.E2_CONST)).all()                     # zero patch: 0 + the constant position row
                assert abs(float(x0h[r["plus"]].mean()) - 1e3) < 1 and abs(float(x0h[r["minus"]].mean()) + 1e3) < 1
                assert np.array_equal(got[r["const"]].view(np.uint32), w["pre_ln_b"].view(np.uint32))   # zero variance: the bias exactly
    finally:
        env.scorer.close()


# ------------------------------------------------------------------------------------------------------------ C: the text tower
@pytest.fixture(scope="module", params=list(Fr.MODES))
def txt(request):
    """A handle of one weight mode with both towers (a text-only handle runs in float32 only): OWL-ViT B/32 at 64 x 96."""
    env = _scorer("vit32", request.param, with_text=True, max_batch=1)
    env.mode, env.rounded = request.param, request.param in Fr.BF16_MODES
    yield env
    env.scorer.close()


@functools.lru_cache(maxsize=None)
def _text_weights():
    """The text blob's entries, as the handles of `txt` hold them."""
    from tstar_amd import weights as W
    g, vb, tb, w = _front_blob("vit32", True)
    return W.unpack_blob(tb, W.text_spec(g))


CASES = dict(t1=Fr.case_t1, t2=Fr.case_t2, t3=Fr.case_t3, t4=Fr.case_t4, t5_1=lambda: Fr.case_t5(1), t5_32=lambda: Fr.case_t5(32))


@functools.lru_cache(maxsize=None)
def _text_ref(case, rounded):
    """(ids, am, float64 tower, float32 yardstick) of a scenario, computed once; the bf16 modes against the tower with rounded GEMM weights."""
    from oracle import owl_ref
    w = _text_weights()
    w = Fr.bf16_text_weights(w) if rounded else w
    ids, am = CASES[case]()
    return ids, am, Fr.text64(ids, am, w), owl_ref.text_query_embeds(ids, am, w).numpy()


def _debug_text(lib, env, ids, am, stage):
    from tstar_amd import _lib
    ids32, am32 = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(am, np.int32)
    Q = ids32.shape[0]
    n = Q * (Fr.T_LEN if stage == 0 else 1)
    out = np.full((n + 2, Fr.T_D), np.float32(-7.0))
    _lib.check(lib.tstar_owl_debug_text(env.scorer._h, ids32.ctypes.data, am32.ctypes.data, Q, stage, out.ctypes.data, _st()), "tstar_owl_debug_text")
    assert (out[n:] == np.float32(-7.0)).all()
    return out[:n]


def _final(env, case):
    """Install the scenario in slot 0, read the unit vectors back, hold them to the bound.  -> (got, float64, bound)"""
    ids, am, r, f32 = _text_ref(case, env.rounded)
    env.scorer.set_queries(ids, am, [1.0] * len(ids))
    got = env.scorer.get_query_embeds()
    b, m = T.bound(f32, r["embeds"])
    e = float(np.abs(got - r["embeds"]).max())
    print(f"{case} {env.mode}: embeds {e:.2g} / {m:.2g} -> {b:.2g}")
    assert np.isfinite(got).all() and e <= b, (case, env.mode, e, m, b)
    return got, r, b


def test_t1_embedding_rows(lib, txt):
    """T1: stage 0 is tok[id] + pos[t] in float32, bit for bit (ids 0 and 49407, repeats); installs nothing."""
    ids, am, r, _ = _text_ref("t1", txt.rounded)
    before = dict(txt.scorer.Qs)
    got = _debug_text(lib, txt, ids, am, 0)
    assert np.array_equal(got.view(np.uint32), r["emb"].reshape(-1, Fr.T_D).view(np.uint32))
    assert txt.scorer.Qs == before


def test_t2_first_maximum(lib, txt):
    """T2: two queries that agree up to their first maximum id (t = 3) pool bit-equal rows whatever follows -- a repeat of the maximum
    at t = 9 included; a query whose first maximum is at t = 9 pools another row; all three match float64."""
    ids, am, r, _ = _text_ref("t2", txt.rounded)
    pooled = _debug_text(lib, txt, ids, am, 1)
    assert np.array_equal(pooled[0].view(np.uint32), pooled[1].view(np.uint32))
    assert np.abs(pooled[2] - pooled[0]).max() > 0.1
    got, r, b = _final(txt, "t2")
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)) and np.abs(got[2] - got[0]).max() > 100 * b


def test_t3_attention_mask(lib, txt):
    """T3: a right-padded query and the same with an interior zero in its mask, both against float64; the zero moves the answer by more
    than the bound."""
    got, r, b = _final(txt, "t3")
    assert np.abs(got[0] - got[1]).max() > b and np.abs(r["embeds"][0] - r["embeds"][1]).max() > b


def test_t4_sixteen_tokens(lib, txt):
    """T4: 16 valid tokens, the maximum at t = 15."""
    _final(txt, "t4")


@pytest.mark.parametrize("Q", [1, 32])
def test_t5_query_counts(lib, txt, Q):
    """T5: the no-bias GEMM form at M = Q (text projection) and the tower at Q x 16 rows, Q = 1 and 32."""
    got, r, b = _final(txt, f"t5_{Q}")
    assert got.shape == (Q, Fr.PROJ)


def test_two_term_handle_runs_the_text_tower_exactly(lib):
    """The text tower of a two-term ("bf16") handle splits its activations exactly, as the bf16_exact mode does everywhere: pooled rows
    and unit vectors of the two handles are the same bits (T4 and T5 at Q = 32)."""
    got = {}
    for mode in Fr.BF16_MODES:
        env = _scorer("vit32", mode, with_text=True, max_batch=1)
        try:
            for case in ("t4", "t5_32"):
                ids, am = CASES[case]()
                pooled = _debug_text(lib, env, ids, am, 1)
                env.scorer.set_queries(ids, am, [1.0] * len(ids))
                got[mode, case] = (pooled, env.scorer.get_query_embeds())
        finally:
            env.scorer.close()
    for case in ("t4", "t5_32"):
        for a, b in zip(got["bf16", case], got["bf16_exact", case]):
            assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), case


def test_t6_padding_queries(lib):
    """T6: ids[q, 0] == 0 marks a padding query: once the set is installed, the tail gives its logits -FLT_MAX on every row."""
    from tstar_amd import _lib
    env = _scorer("vit32", "f32", with_text=True, max_batch=1)
    try:
        ids, am = Fr.case_t6()
        env.scorer.set_queries(ids, am, [1.0] * 4)
        npatch = env.g.npatch
        feats, cls, boxh = (_dev(a) for a in T._rows(np.random.RandomState(3), npatch))
        scores = torch.full((npatch,), float("nan"), device="cuda")
        labels = torch.full((npatch,), -7, dtype=torch.int32, device="cuda")
        xyxy = torch.full((npatch, 4), float("nan"), device="cuda")
        lg = torch.full((npatch, 4), float("nan"), device="cuda")
        _lib.check(lib.tstar_owl_debug_heads(env.scorer._h, feats.data_ptr(), cls.data_ptr(), boxh.data_ptr(), 1, 95, 200, None, scores.data_ptr(),
                                             labels.data_ptr(), xyxy.data_ptr(), lg.data_ptr(), None, None, None, _st()), "tstar_owl_debug_heads")
        torch.cuda.synchronize()
        lg = lg.cpu().numpy()
        assert (lg[:, [1, 3]] == np.float32(T.F32_MIN)).all()
        assert np.isfinite(lg[:, [0, 2]]).all() and (lg[:, [0, 2]] > np.float32(T.F32_MIN)).all()
        assert np.isin(labels.cpu().numpy(), [0, 2]).all()
    finally:
        env.scorer.close()
