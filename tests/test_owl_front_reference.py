"""CPU pins of tests/owl_front_util.py, which the GPU tests of the detector front (tests/test_gpu_owl_front.py) are built on: every
plan the launcher's ladder is expected to make equals tstar_gemm_plan's; the shapes of part A reach every (mode, kind) form; the
crafted position table gives the run's table its constant row and its rows with mean +-1e3; the float64 text tower agrees with
oracle/owl_ref.text_query_embeds within float32 rounding, and its pooled rows have the causal property of scenario T2 exactly."""
import numpy as np
import pytest
import torch

import owl_front_util as Fr
import owl_tail_util as T
from oracle import owl_ref
from tstar_amd import weights as W


@pytest.fixture(scope="module")
def lib():
    from tstar_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("B", Fr.LADDER_B)
def test_ladder_plans(lib, B):
    """The (kind, m_split) table of owl_front_util.LADDER_PLAN, row by row, against the launcher's own plan."""
    M = B * Fr.LADDER["np"]
    for mode in Fr.MODES:
        assert Fr.gemm_plan(lib, mode, M, Fr.LADDER["N"], Fr.LADDER["np"], -1) == Fr.LADDER_PLAN[B][mode], (B, mode)


def test_ladder_reaches_every_form_on_its_own():
    """Without a forced tile: all three grids and the hybrid launch in every mode, wide in f32x3, wide with streamed weights in the
    two-term mode; the hybrid and wide launches with a big part and a tail.  Two forms are reached by S1..S4's forced tiles only: the
    two-term mode's plain wide form (tile_cfg 4) and f32x3's 128x128 grid (the wide tile takes its place at B = 16)."""
    reached = {(m, Fr.LADDER_PLAN[B][m][0]) for B in Fr.LADDER_B for m in Fr.MODES}
    assert reached == Fr.REACHABLE - {("bf16", Fr.WIDE), ("f32x3", Fr.GRID_128)}
    for m in Fr.MODES:
        assert any(0 < Fr.LADDER_PLAN[B][m][1] < B * Fr.LADDER["np"] for B in Fr.LADDER_B)


def test_small_shapes_plans(lib):
    """S1..S4 at every tile_cfg of every mode: the forced forms are the forms asked for; the only refusals are tile_cfg 6 without a
    wide tile (S3: N = 128)."""
    for name, s in Fr.SHAPES.items():
        M = s["B"] * s["np"]
        for mode in Fr.MODES:
            for cfg in Fr.tile_cfgs(mode):
                p = Fr.gemm_plan(lib, mode, M, s["N"], s["np"], cfg)
                if p is None:
                    assert cfg == 6 and s["N"] % 256 != 0, (name, mode, cfg)
                    continue
                kind, m_split = p
                wide_ok = s["N"] % 256 == 0
                want = {0: Fr.GRID_128, 1: Fr.GRID_64N, 2: Fr.GRID_64, 3: Fr.HYBRID, 17: Fr.HYBRID, 18: Fr.HYBRID, 5: Fr.GRID_64,
                        -1: Fr.GRID_64, 4: Fr.WIDE if wide_ok else Fr.GRID_64, 6: Fr.WIDE_VW}[cfg]
                assert kind == want, (name, mode, cfg, p)
                if kind in (Fr.HYBRID, Fr.WIDE, Fr.WIDE_VW):
                    assert 0 < m_split <= M and m_split % 128 == 0


def test_patch_inputs_are_what_the_issue_asks_for():
    A, Wt, pos = Fr.patch_inputs(9, 37, 256, 96, 1)
    assert A.shape == (333, 96) and Wt.shape == (256, 96) and pos.shape == (38, 256)
    big = (pos.abs().mean(1) > 40).nonzero().flatten().tolist()
    assert big == [0, 1, 19, 37]
    A2, _, pos2 = Fr.patch_inputs(130, 1, 256, 64, 2)
    assert pos2.shape == (2, 256) and (pos2.abs().mean(1) > 40).all()
    assert torch.equal(A, Fr.patch_inputs(9, 37, 256, 96, 1)[0])
    ref, mag = Fr.patch_ref64(A, Wt, pos, 9, 37, "f32")
    want = torch.nn.functional.linear(A, Wt).view(9, 37, 256) + pos[1:]
    assert (ref.view(9, 37, 256) - want).abs().max() < 3e-5 * max(1.0, float(want.abs().max()))
    assert (mag >= ref.abs() * (1 - 1e-12)).all()
    refb, _ = Fr.patch_ref64(A, Wt, pos, 9, 37, "bf16")
    assert 1e-4 < (refb - ref).abs().max() / ref.abs().max() < 2.0 ** -7


# ------------------------------------------------------------------------------------------------------------------- part B
def test_crafted_table_gives_the_run_its_special_rows():
    """OWL-ViT B/32 at 64 x 96 (2 x 3 patches of a 24 x 24 table): after the resampling patch 1's row is exactly E2_CONST, patches
    3 and 4 have mean +-1e3 and a spread of 0.5 .. 1, the other rows are ordinary, and the class row is the crafted one."""
    g, sd, vb, tb, w = Fr.front_blob("owlvit", None, (64, 96))
    assert (g.npatch, g.ntok) == (6, 7) and w["pos"].shape == (7, Fr.D) and w["patch_w"].shape == (Fr.D, 3072)
    pos = w["pos"]
    crafted = Fr.crafted_front(g)
    assert np.array_equal(pos[0], crafted["owlvit.vision_model.embeddings.position_embedding.weight"][0])
    assert (pos[1 + Fr.E2_ROWS["const"]] == np.float32(Fr.E2_CONST)).all()
    for k, m in (("plus", 1e3), ("minus", -1e3)):
        r = pos[1 + Fr.E2_ROWS[k]].astype(np.float64)
        assert abs(r.mean() - m) < 0.2 and 0.5 < r.std() < 1.0, (k, r.mean(), r.std())
    for p in (0, 2, 5):
        assert np.abs(pos[1 + p]).max() < 0.1 and pos[1 + p].std() > 0.005
    # the table is the resampled one: another row of the native table behind a patch changes that patch's row only
    other = dict(sd)
    key = "owlvit.vision_model.embeddings.position_embedding.weight"
    other[key] = sd[key].copy()
    other[key][Fr.bicubic_support(g, 5)[5]] += 1.0
    pos2 = W.unpack_blob(W.pack_blob(other, W.vision_spec(g), g), W.vision_spec(g))["pos_emb"]
    changed = np.flatnonzero((pos2 != pos).any(1)).tolist()
    assert changed == [6]


@pytest.mark.parametrize("family,patch,size,ntok", [("owlvit", 16, (16, 16), 2), ("owlv2", None, (16, 16), 2)])
def test_small_geometries(family, patch, size, ntok):
    g, sd, vb, tb, w = Fr.front_blob(family, patch, size)
    assert g.ntok == ntok and w["pos"].shape == (ntok, Fr.D) and w["patch_w"].shape == (Fr.D, 768)
    x = Fr.embed_patches(g, 3)
    assert x.shape == (3, 768) and abs(float(x.std()) - 1.0) < 0.05


def test_bound_of_the_in_place_layernorm_is_the_tails():
    """E2's yardstick: float32 torch's layer_norm against ln64 on rows like the stage-0 output (a constant row, rows with mean
    +-1e3), through owl_tail_util.bound."""
    g, sd, vb, tb, w = Fr.front_blob("owlvit", None, (64, 96))
    x = (w["pos"] + 0.0).astype(np.float32)
    y32 = torch.nn.functional.layer_norm(torch.from_numpy(x), (Fr.D,), torch.from_numpy(w["pre_ln_w"]), torch.from_numpy(w["pre_ln_b"]), 1e-5).numpy()
    ref = T.ln64(x, w["pre_ln_w"], w["pre_ln_b"])
    b, m = T.bound(y32, ref)
    assert 0 < m < 1e-3 and b >= 4 * m
    assert np.array_equal(ref[1 + Fr.E2_ROWS["const"]], w["pre_ln_b"].astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------- part C
@pytest.fixture(scope="module")
def text_w():
    sd = W.synthetic_state_dict(0, "text")
    return W.unpack_blob(W.pack_blob(sd, W.text_spec()), W.text_spec())


@pytest.mark.parametrize("rounded", [False, True])
def test_text_tower_agrees_with_oracle(text_w, rounded):
    """|float64 tower - oracle/owl_ref.text_query_embeds| on every scenario: within float32 rounding (1e-6 on unit vectors; measured
    2e-7), with the float32 weights and with the GEMM weights rounded to bf16 on both sides."""
    w = Fr.bf16_text_weights(text_w) if rounded else text_w
    if rounded:
        assert not np.array_equal(w["text_proj"], text_w["text_proj"]) and np.array_equal(w["tok_emb"], text_w["tok_emb"])
    for name, (ids, am) in dict(t1=Fr.case_t1(), t2=Fr.case_t2(), t3=Fr.case_t3(), t4=Fr.case_t4(), t5=Fr.case_t5(4), t6=Fr.case_t6()).items():
        r = Fr.text64(ids, am, w)
        got = owl_ref.text_query_embeds(ids, am, w).numpy()
        e = float(np.abs(got - r["embeds"]).max())
        print(f"{name}: oracle vs float64 {e:.2g}")
        assert e < 1e-6, (name, e)
        assert np.allclose(np.linalg.norm(r["embeds"], axis=1), 1.0, atol=1e-12)
        assert np.array_equal(r["eos"], ids.argmax(-1))
        assert np.array_equal(r["emb"], (torch.from_numpy(w["tok_emb"])[torch.from_numpy(ids)] + torch.from_numpy(w["tpos_emb"])).numpy())


def test_bf16_rounding_is_visible(text_w):
    """The rounding of the checkpoint moves the embeddings by far more than float32 arithmetic does: a bf16 handle has to be measured
    against the tower with rounded weights."""
    ids, am = Fr.case_t5(4)
    a, b = Fr.text64(ids, am, text_w)["embeds"], Fr.text64(ids, am, Fr.bf16_text_weights(text_w))["embeds"]
    assert np.abs(a - b).max() > 1e-4


def test_t2_causal_property_is_exact_in_float64(text_w):
    ids, am = Fr.case_t2()
    assert Fr.first_max(ids).tolist() == [3, 3, 9] and (am == 1).all()
    assert (ids[0, :4] == ids[1, :4]).all() and (ids[0, 4:11] != ids[1, 4:11]).all() and ids[1, 9] == ids[1, 3]
    r = Fr.text64(ids, am, text_w)
    assert np.array_equal(r["pooled"][0], r["pooled"][1])
    assert np.abs(r["pooled"][2] - r["pooled"][0]).max() > 0.1


def test_t3_mask_changes_the_answer(text_w):
    ids, am = Fr.case_t3()
    assert Fr.first_max(ids).tolist() == [5, 5] and am[0].tolist() == [1] * 6 + [0] * 10 and am[1].tolist() == [1, 0] + [1] * 4 + [0] * 10
    r = Fr.text64(ids, am, text_w)
    f32 = owl_ref.text_query_embeds(ids, am, text_w).numpy()
    b, _ = T.bound(f32, r["embeds"])
    assert np.abs(r["embeds"][0] - r["embeds"][1]).max() > 100 * b
    # padding behind the first maximum is never seen by the pooled row
    am_full = np.ones_like(am)
    assert np.array_equal(Fr.text64(ids[:1], am_full[:1], text_w)["pooled"], r["pooled"][:1])


def test_scenarios_are_what_the_issue_asks_for():
    ids, am = Fr.case_t1()
    assert 0 in ids and 49407 in ids and (ids[0, 1] == ids[0, 2]) and ids.min() >= 0 and ids.max() < Fr.VOCAB
    ids, am = Fr.case_t4()
    assert (am == 1).all() and Fr.first_max(ids).tolist() == [15]
    for Q in (1, 32):
        ids, am = Fr.case_t5(Q)
        assert ids.shape == (Q, 16) and (am[:, 0] == 1).all() and (ids[:, 0] > 0).all()
        assert ((ids == Fr.EOS).sum(1) == 1).all() and (am.sum(1) == Fr.first_max(ids) + 1).all()
    ids, am = Fr.case_t6()
    assert (ids[:, 0] == 0).tolist() == [False, True, False, True] and (am[:, 0] == 1).all()
