"""The OWL-ViT / OWLv2 detector TAIL -- write_cls_rows, merge_cls_ln (csrc/rowops.hip), l2norm_rows_kernel behind
set_query_embeds, detect_rows, row_dot768 and cell_reduce (csrc/heads.hip) -- on crafted inputs, kernel by kernel, through the
diagnostic entries tstar_owl_debug_merge / tstar_owl_debug_heads / tstar_cell_reduce (the launchers tstar_owl_score calls, same
arguments), against the float64 restatement of tests/owl_tail_util.py (pinned on the CPU by tests/test_owl_tail_reference.py).

Two module-scoped scorers with crafted tail weights laid over the synthetic state dict: OWL-ViT B/32 at input 64 x 96 (np = 6,
ntok = 7; B = 3 gives 18 rows, so the fifth block of four waves is half full) and OWLv2 B/16 at input 16 x 16 (np = 1, ntok = 2;
box scale max(H, W), objectness, a post-LayerNorm without bias).

Bit-exact: every cell output and n_kept; labels on crafted ties, masks and degenerate rows; class-token rows and sentinels;
-FLT_MAX logits and the 0.0 score of a fully masked set.  Everything else is compared with float64 under
    bound = 4 x (worst error of the same formulas in float32 torch against float64) + one float32 ulp of the largest magnitude,
computed per scenario and quantity by owl_tail_util.bound: the 4 x covers the kernels' wave-shuffle summation order against
torch's; the ulp term is there because over a few dozen elements the measured figure can be zero by luck (a saturated sigmoid is
exactly 1.0 in float32), and no float32 result can be asked to be closer than its own spacing.

Measured on an MI355X (HIP error / float32-torch error -> bound; the float32 figure varies a little with the CPU torch runs on, so
the bound is recomputed on every run and every test prints all three under `pytest -s`; profiles/owl_tail_tests.md has the table):
    D1 random        logits 2.1e-07 / 3.9e-07 -> 1.8e-06   scores 3.8e-08 / 1.1e-07 -> 5.3e-07   xyxy 2.2e-05 / 2.5e-05 -> 1.3e-04 px
    D2 masks (Q=32)  logits 1.9e-07 / 4.8e-07 -> 2.2e-06   scores 5.7e-08 / 1.2e-07 -> 6.0e-07
    D3 ties          logits 3.7e-07 / 6.6e-07 -> 3.0e-06   D4 mixed sets: scores 5.3e-08 / 7.7e-08 -> 4.2e-07
    D5 zero rows     logits 3.4e-07 / 5.6e-07 -> 2.5e-06
    D6 ELU           logits 3.5e-07 / 1.1e-06 -> 4.5e-06; relative, rows -1e-3 .. 5: 2.1e-07 / 6.4e-07 -> 2.7e-06; row -20: exactly -0
    D7 boxes         OWL-ViT xyxy 6.1e-06 / 6.9e-05 -> 3.1e-04 px; OWLv2 xyxy 5.5e-06 / 4.8e-05 -> 2.1e-04 px
    D8 row_dot768    1 row 4.0e-07 / 1.6e-07 -> 1.1e-06; 18 rows 9.3e-07 / 1.9e-06 -> 8.9e-06
    M1 merge         ntok 7: 1.1e-06 / 8.0e-07 -> 3.8e-06; ntok 2: 7.3e-07 / 8.1e-07 -> 3.8e-06
    M2               rows with mean 1e3: 1.3e-04 / 1.3e-04 -> 5.2e-04; zero product: 6.1e-07 / 5.0e-07 -> 2.5e-06
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import owl_tail_util as T

pytestmark = pytest.mark.gpu


def _scorer(family, input_size, max_batch, sets, slots):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    g = W.with_input_size(W.geometry_for_family(family), input_size)
    crafted = T.crafted_tail(family)
    sd = W.synthetic_state_dict(0, "vision", geometry=g)
    sd.update(crafted)
    vb = W.pack_blob(sd, W.vision_spec(g), g)
    held = W.unpack_blob(vb, W.vision_spec(g))
    w = T.tail_weights(crafted, g)
    for k, v in w.items():                                   # the handle holds the crafted tail
        assert np.array_equal(held[k].reshape(-1), np.asarray(v).reshape(-1)), k
    w["pos0"] = held["pos_emb"][0].copy()
    s = OwlScorer(vb, None, max_batch=max_batch, input_size=input_size, family=family)
    for slot in slots:
        s.set_query_embeds(*sets[slot], slot=slot)
    return SimpleNamespace(scorer=s, w=w, sets=sets, np=g.npatch, ntok=g.ntok, family=family)


@pytest.fixture(scope="module")
def vit():
    e = _scorer("owlvit", (64, 96), 4, T.query_sets(), range(7))
    assert (e.np, e.ntok) == (6, 7)
    yield e
    e.scorer.close()


@pytest.fixture(scope="module")
def v2():
    e = _scorer("owlv2", (16, 16), 18, T.query_sets(), [1])
    assert (e.np, e.ntok) == (1, 2)
    yield e
    e.scorer.close()


@pytest.fixture(scope="module")
def lib():
    from tstar_amd import _lib
    return _lib, _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_heads(env, case, logits=True, cxcywh=True, obj_hidden=None):
    from tstar_amd import _lib
    rows = case["feats"].shape[0]
    B = rows // env.np
    qs = {len(env.sets[s][1]) for s in case["sets"]}
    f, c, b = _dev(case["feats"]), _dev(case["cls"]), _dev(case["boxh"])
    scores = torch.full((rows,), float("nan"), device="cuda")
    labels = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    xyxy = torch.full((rows, 4), float("nan"), device="cuda")
    lg = torch.full((rows, qs.copy().pop()), float("nan"), device="cuda") if logits else None
    cw = torch.full((rows, 4), float("nan"), device="cuda") if cxcywh else None
    oh = _dev(obj_hidden) if obj_hidden is not None else None
    ob = torch.full((rows,), float("nan"), device="cuda") if obj_hidden is not None else None
    sets = np.ascontiguousarray(case["sets"], dtype=np.int32)
    rc = _lib.load().tstar_owl_debug_heads(env.scorer._h, f.data_ptr(), c.data_ptr(), b.data_ptr(), B, case["H"], case["W"],
                                           None if not sets.any() else sets.ctypes.data, scores.data_ptr(), labels.data_ptr(), xyxy.data_ptr(),
                                           _lib.ptr(lg), _lib.ptr(cw), _lib.ptr(oh), _lib.ptr(ob), _st())
    _lib.check(rc, "tstar_owl_debug_heads")
    torch.cuda.synchronize()
    out = dict(scores=scores.cpu().numpy(), labels=labels.cpu().numpy(), xyxy=xyxy.cpu().numpy())
    if logits:
        out["logits"] = lg.cpu().numpy()
    if cxcywh:
        out["cxcywh"] = cw.cpu().numpy()
    if ob is not None:
        out["objectness"] = ob.cpu().numpy()
    return out


def check_detect(name, env, case, out):
    """Every output of one detect_rows call against float64 under the measured bound; padded queries' logits exactly -FLT_MAX;
    labels equal to the float64 argmax wherever its top-2 margin exceeds the logit bound.  -> (float64 result, share of rows whose
    label was not compared, logit bound)."""
    r64, r32 = T.detect64(case, env.w, env.sets, env.np, env.family), T.detect_f32(case, env.w, env.sets, env.np, env.family)
    real = np.concatenate([m.reshape(-1) for m in T.unmasked(case, env.sets, env.np)])
    ref_lg, f32_lg = np.concatenate([l.reshape(-1) for l in r64["logits"]]), np.concatenate([l.reshape(-1) for l in r32["logits"]])
    bl, ml = T.bound(f32_lg, ref_lg, real)
    line = [f"{name}:"]
    if "logits" in out:
        got = out["logits"].reshape(-1)
        el = float(np.abs(got - ref_lg)[real].max()) if real.any() else 0.0
        line.append(f"logits {el:.2g} / {ml:.2g} -> {bl:.2g}")
        assert el <= bl
        assert (got[~real] == np.float32(T.F32_MIN)).all()
    for k in ("scores", "xyxy") + (("cxcywh",) if "cxcywh" in out else ()):
        bk, mk = T.bound(r32[k], r64[k])
        ek = float(np.abs(out[k] - r64[k]).max())
        line.append(f"{k} {ek:.2g} / {mk:.2g} -> {bk:.2g}")
        assert np.isfinite(out[k]).all() and ek <= bk, (k, ek, bk)
    clear = r64["margin"] > bl
    assert np.array_equal(out["labels"][clear], r64["labels"][clear])
    print(" ".join(line) + f"; labels compared on {int(clear.sum())} of {len(clear)} rows")
    return r64, float((~clear).mean()), bl


# ------------------------------------------------------------------------------------------------------------ detect_rows
def test_d1_random_and_optional_outputs(vit):
    """D1: B = 3, Q = 4, every output; without the logits / cxcywh pointers no other output bit changes."""
    case = T.case_d1(vit.np)
    out = run_heads(vit, case)
    _, excluded, _ = check_detect("D1", vit, case, out)
    assert excluded <= 0.05
    bare = run_heads(vit, case, logits=False, cxcywh=False)
    for k in ("scores", "labels", "xyxy"):
        assert np.array_equal(out[k].view(np.uint32), bare[k].view(np.uint32)), k


def test_d2_masked_queries(vit):
    """D2: Q = 32 with padded queries first, in the middle and last (rows whose class embedding IS a padded query would pick it
    without the mask) and a zero query vector; then a set with every query padded: label 0, score exactly 0.0, logits -FLT_MAX."""
    case = T.case_d2(vit.np, vit.sets, 0)
    out = run_heads(vit, case)
    r64, _, bl = check_detect("D2 Q=32", vit, case, out)
    assert not np.isin(out["labels"], [0, 15, 31]).any()
    free = T.class_logits64(case["feats"][:3], case["cls"][:3], vit.sets[0][0], np.ones(32, np.uint8), vit.w).argmax(-1)
    assert free.tolist() == [0, 15, 31]                      # ... which the unmasked argmax would have been
    zero_q = out["logits"][:, 7].astype(np.float64)          # sim = 0: shift * scale
    want = T.shift64(case["feats"], vit.w) * T._elu_plus_one(T.scale_pre64(case["feats"], vit.w))
    assert np.abs(zero_q - want).max() <= bl
    allpad = T.case_d2(vit.np, vit.sets, 3)
    o = run_heads(vit, allpad)
    assert (o["labels"] == 0).all() and (o["scores"].view(np.uint32) == 0).all()
    assert (o["logits"] == np.float32(T.F32_MIN)).all()
    check_detect("D2 all padded", vit, allpad, o)


def test_d3_ties_take_the_lower_index(vit):
    """D3: queries 3 / 17 and 0 / 31 are duplicates; on rows where they win the two logits are bit-equal and the label is the lower one."""
    case = T.case_d3(vit.np, vit.sets)
    out = run_heads(vit, case)
    check_detect("D3", vit, case, out)
    lg = out["logits"].view(np.uint32)
    assert np.array_equal(lg[:, 3], lg[:, 17]) and np.array_equal(lg[:, 0], lg[:, 31])
    assert (out["labels"][:6] == 3).all() and (out["labels"][6:12] == 0).all()
    best = out["logits"].max(-1)
    assert (out["logits"][:6, 17] == best[:6]).all() and (out["logits"][6:12, 31] == best[6:12]).all()      # the duplicates tie for the maximum


def test_d4_mixed_query_sets(vit):
    """D4: image -> set [2, 0, 2, 5] (Q = 3 / 32 / 3 / 1, each with its own mask), no logits: every image against its own set."""
    case = T.case_d4(vit.np)
    out = run_heads(vit, case, logits=False)
    r64, _, _ = check_detect("D4", vit, case, out)
    lab = out["labels"].reshape(4, vit.np)
    assert (lab[0] != 1).all() and (lab[2] != 1).all() and (lab[3] == 0).all() and not np.isin(lab[1], [0, 15, 31]).any()
    assert lab[1].max() > 2                                  # the Q = 32 image is not scored against a three-query set
    with pytest.raises(Exception, match="same query count"):
        run_heads(vit, case, logits=True)


def test_d5_zero_class_row(vit):
    """D5: an all-zero class embedding makes every real logit shift * scale: bit-equal, and the label is the first unpadded query."""
    case = T.case_d5(vit.np)
    out = run_heads(vit, case)
    check_detect("D5", vit, case, out)
    z = case["zero_rows"]
    assert (out["labels"][z] == 2).all()
    lg = out["logits"][z].view(np.uint32)
    assert np.array_equal(lg[:, 2], lg[:, 3])


def test_d6_elu_branches(vit):
    """D6: scale pre-activations -20, -1e-3, 0 (to float32 rounding), 1e-3 and 5.  Rows 1-4: RELATIVE logit error under
    4 x float32 torch's + one ulp.  (After the `+ 1` both expm1(x) and exp(x) - 1 round to the same float32 to within an ulp, so a
    relative bound at scale ~ 1 is what the logits can show.)  Row 0: ELU + 1 = 2.06e-9 is below float32's spacing at 1, the
    float32 sum is 0 or a few 2^-24: absolute error under 4 x float32 torch's + one ulp of 1.0 times the largest |sim + shift|."""
    case = T.case_d6(vit.np, vit.w)
    out = run_heads(vit, case)
    r64, _, _ = check_detect("D6", vit, case, out)
    r32 = T.detect_f32(case, vit.w, vit.sets, vit.np, vit.family)
    ref, f32, got = r64["logits"][0], r32["logits"][0].astype(np.float64), out["logits"].astype(np.float64)
    rel = lambda a: np.abs(a[1:5] - ref[1:5]) / np.abs(ref[1:5])
    b_rel = 4 * rel(f32).max() + T.EPS32
    print(f"D6: relative logit error rows 1-4 {rel(got).max():.2g} / {rel(f32).max():.2g} -> {b_rel:.2g}; row 0 logits {got[0]} (float64 {ref[0]})")
    assert rel(got).max() <= b_rel
    factor = np.abs(ref[0]).max() / float(T._elu_plus_one(T.scale_pre64(case["feats"][:1], vit.w))[0])
    assert np.abs(got[0] - ref[0]).max() <= 4 * np.abs(f32[0] - ref[0]).max() + T.EPS32 * factor


def _check_boxes(env, case, out):
    r64 = T.detect64(case, env.w, env.sets, env.np, env.family)
    assert np.isfinite(out["cxcywh"]).all() and np.isfinite(out["xyxy"]).all()
    assert (out["cxcywh"][0] == 1.0).all()                   # +100: 1 / (1 + 3.8e-44)
    assert (out["cxcywh"][1] >= 0).all() and (out["cxcywh"][1] < 1e-37).all()       # -100: 3.8e-44 or flushed to 0
    assert np.abs(out["cxcywh"][2] - 0.5).max() < 1e-4
    assert (out["cxcywh"][4, :2] == 1.0).all() and (out["cxcywh"][4, 2:] < 1e-37).all()
    return r64


def test_d7_saturated_boxes_owlvit(vit):
    """D7: pre-sigmoid box values of +-100 and 0 reached THROUGH a box_bias of up to 9.2; finite, saturated, and the corner form
    scaled by (W, H)."""
    H, W = 95, 200
    case = T.case_d7(vit.np, vit.w, H, W)
    out = run_heads(vit, case)
    check_detect("D7 OWL-ViT", vit, case, out)
    _check_boxes(vit, case, out)
    assert np.allclose(out["xyxy"][0], [0.5 * W, 0.5 * H, 1.5 * W, 1.5 * H], rtol=1e-6)
    assert np.allclose(out["xyxy"][4], [W, H, W, H], rtol=1e-6)


def test_d7_saturated_boxes_owlv2(v2):
    """D7 on the OWLv2 handle: both axes scaled by max(H, W), so a 2:1 image has centres beyond its short side."""
    H, W = 50, 100
    case = T.case_d7(v2.np, v2.w, H, W)
    out = run_heads(v2, case)
    check_detect("D7 OWLv2", v2, case, out)
    _check_boxes(v2, case, out)
    assert np.allclose(out["xyxy"][0], [0.5 * W, 0.5 * W, 1.5 * W, 1.5 * W], rtol=1e-6)
    assert out["xyxy"][4, 1] > H                             # the centre's y: 100 on an image 50 high
    vit_scaled = T.detect64(case, v2.w, v2.sets, v2.np, "owlvit")["xyxy"]
    assert np.abs(out["xyxy"] - vit_scaled).max() > 10       # (W, H) scaling would be another answer


@pytest.mark.parametrize("rows", [1, 18])
def test_d8_row_dot768(v2, rows):
    """D8: the objectness dense2 on 1 row and on 18 (the fifth block half full), against float64."""
    case = T.case_random(v2.np, rows, [1] * rows, 28)
    rs = np.random.RandomState(29 + rows)
    hid = (T._unit(rs, rows, T.D) * rs.uniform(0.1, 4.0, (rows, 1))).astype(np.float32)
    out = run_heads(v2, case, obj_hidden=hid)
    ref = T.row_dot64(hid, v2.w)
    b, m = T.bound(T.row_dot_f32(hid, v2.w), ref)
    e = float(np.abs(out["objectness"] - ref).max())
    print(f"D8 rows={rows}: {e:.2g} / {m:.2g} -> {b:.2g}")
    assert e <= b
    bare = run_heads(v2, case)
    for k in ("scores", "labels", "xyxy", "logits"):
        assert np.array_equal(out[k].view(np.uint32), bare[k].view(np.uint32)), k


# ------------------------------------------------------------------------------------------- write_cls_rows / merge_cls_ln
def run_merge(env, x, B, write_cls):
    from tstar_amd import _lib
    dx = _dev(x)
    feats = torch.full((B * env.np, T.D), float("nan"), device="cuda")
    _lib.check(_lib.load().tstar_owl_debug_merge(env.scorer._h, dx.data_ptr(), B, int(write_cls), feats.data_ptr(), _st()), "tstar_owl_debug_merge")
    torch.cuda.synchronize()
    return dx.cpu().numpy(), feats.cpu().numpy()


def _check_merge(name, env, x, B, got):
    ref = T.merge64(x, B, env.ntok, env.w)
    b, m = T.bound(T.merge_f32(x, B, env.ntok, env.w), ref)
    e = float(np.abs(got - ref).max())
    print(f"{name}: {e:.2g} / {m:.2g} -> {b:.2g}")
    assert np.isfinite(got).all() and e <= b
    return ref


@pytest.mark.parametrize("which", ["vit", "v2"])
def test_m1_merge_and_cls_rows(vit, v2, which):
    """M1: B = 3 at ntok = 7 (18 rows; row / np picks the image) and at ntok = 2, a distinct class-token row per image, against
    float64; then with write_cls: the class-token rows are bit-equal to class_emb + pos[0], every other row keeps its bits."""
    env = vit if which == "vit" else v2
    B = 3
    x = T.case_m1(B, env.ntok)
    after, feats = run_merge(env, x, B, False)
    assert np.array_equal(after.view(np.uint32), x.view(np.uint32))
    ref = _check_merge(f"M1 ntok={env.ntok}", env, x, B, feats)
    other = x.reshape(B, env.ntok, T.D).copy()
    other[:, 0] = other[[1, 2, 0], 0]                        # with another image's class token the answer is another one
    assert np.abs(T.merge64(other.reshape(-1, T.D), B, env.ntok, env.w) - ref).max() > 0.1
    after, feats = run_merge(env, x, B, True)
    cls_row = (env.w["class_emb"] + env.w["pos0"]).astype(np.float32)
    a3, x3 = after.reshape(B, env.ntok, T.D), x.reshape(B, env.ntok, T.D)
    for b in range(B):
        assert np.array_equal(a3[b, 0].view(np.uint32), cls_row.view(np.uint32))
    assert np.array_equal(a3[:, 1:].view(np.uint32), x3[:, 1:].view(np.uint32))
    _check_merge(f"M1 ntok={env.ntok} after write_cls", env, after, B, feats)


def test_m2_constant_rows_and_large_means(vit):
    """M2 at ntok = 7: constant token rows have zero variance -- the post-LayerNorm gives its bias exactly, whatever the constant
    (their outputs are bit-equal); rows with mean +-1e3 and unit spread need the two-pass variance (E[x^2] - mean^2 in float32 loses the
    spread below 1e6 * 2^-24)."""
    x = T.case_m2(vit.ntok)
    _, feats = run_merge(vit, x, 1, False)
    _check_merge("M2", vit, x, 1, feats)
    assert np.array_equal(feats[0].view(np.uint32), feats[1].view(np.uint32)) and np.array_equal(feats[0].view(np.uint32), feats[2].view(np.uint32))
    e = T.ln64(x[:1], vit.w["post_ln_w"], vit.w["post_ln_b"])
    bias_path = T.ln64(vit.w["post_ln_b"].astype(np.float64) * e, vit.w["det_ln_w"], vit.w["det_ln_b"])[0]
    ref = T.merge64(x, 1, vit.ntok, vit.w)
    assert np.abs(ref[0] - bias_path).max() < 1e-6          # up to the LayerNorm's epsilon: the restatement says the same


def test_m2_all_zero_product(v2):
    """M2 on the OWLv2 handle (post-LayerNorm bias 0): a constant patch row normalises to exactly 0, its product with the class
    token is all zero, and the detection LayerNorm of a zero row is its bias -- exactly."""
    x = T.case_m1(3, v2.ntok, seed=33)
    x[1], x[3] = 3.0, -0.5                                   # the patch rows of images 0 and 1
    _, feats = run_merge(v2, x, 3, False)
    bias = v2.w["det_ln_b"].view(np.uint32)
    assert np.array_equal(feats[0].view(np.uint32), bias) and np.array_equal(feats[1].view(np.uint32), bias)
    _check_merge("M2 zero product", v2, x, 3, feats)


# ------------------------------------------------------------------------------------------------------------- cell_reduce
def run_cells(c, expect_rc=0):
    from tstar_amd import _lib
    lib = _lib.load()
    B, npatch = c["scores"].shape
    ncell = c["rows"] * c["cols"]
    s, l, x = _dev(c["scores"].astype(np.float32)), _dev(c["labels"].astype(np.int32)), _dev(c["xyxy"].astype(np.float32))
    n_out = min(ncell, 8192)
    conf = torch.full((B, n_out), -1.0, dtype=torch.float64, device="cuda")
    mask = torch.full((B, n_out), -1, dtype=torch.int32, device="cuda")
    kept = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    wts = np.ascontiguousarray(c["weights"], dtype=np.float64)
    sets = None if c["image_set"] is None else np.ascontiguousarray(c["image_set"], dtype=np.int32)
    rc = lib.tstar_cell_reduce(s.data_ptr(), l.data_ptr(), x.data_ptr(), wts.ctypes.data, wts.shape[0], None if sets is None else sets.ctypes.data,
                               B, npatch, c["W"], c["H"], c["rows"], c["cols"], C.c_float(float(c["thr"])), conf.data_ptr(), mask.data_ptr(),
                               kept.data_ptr(), _st())
    assert rc == expect_rc, (rc, lib.tstar_last_error())
    torch.cuda.synchronize()
    return conf.cpu().numpy(), mask.cpu().numpy().view(np.uint32), kept.cpu().numpy()


def check_cells(c):
    conf, mask, kept = run_cells(c)
    rconf, rmask, rkept = T.cell_reduce_ref(c["scores"], c["labels"], c["xyxy"], c["weights"], c["image_set"], c["W"], c["H"], c["rows"], c["cols"], c["thr"])
    bad = np.flatnonzero((conf.view(np.uint64) != rconf.view(np.uint64)).any(1) | (mask != rmask).any(1))
    report = [(int(b), c["xyxy"][b].tolist(), np.flatnonzero(conf[b]).tolist(), np.flatnonzero(rconf[b]).tolist()) for b in bad[:6]]
    assert len(bad) == 0, f"{len(bad)} images differ (image, boxes, kernel's cells, numpy's cells): {report}"
    assert np.array_equal(kept, rkept)
    return conf, mask, kept


@pytest.mark.parametrize("size,n", T.C1_AXES)
def test_c1_borders(size, n):
    """C1: box centres on, just below and just above every cell border of a non-representable cell size (degenerate boxes and
    boxes whose float32 sum rounds), up to and beyond the image edge; both axes; bit-exact against numpy 1.26's float64
    floor_divide.  Negative centres are out of contract (a centre is a sigmoid times a positive size; the reference would index
    the map from its end) and are not fed.  On the parent commit (floor(cx / cw)): (800, 6) puts cx = 400.0 into cell 3 (numpy:
    2); (800, 15) 160.0 / 320.0 / 480.0 / 640.0 into 3 / 6 / 9 / 12 (numpy: 2 / 5 / 8 / 11); (800, 24) 100.0, 200.0, ... likewise."""
    diff = [d for d in T.c1_differing() if d[:2] == (size, n)]
    if (size, n) in ((800, 6), (800, 15), (800, 24)):
        assert diff                                          # the case cannot silently go dead
    c = T.c1_case(size, n)
    assert (T.c1_centres(size, n) >= 0).all() and (T.c1_centres(size, n) > size).any()
    _, _, kept = check_cells(c)
    assert (kept == 2).all()
    print(f"C1 ({size}, {n}): {len(c['scores'])} images; centres where floor(a / b) gives another cell: {sorted({d[2:] for d in diff})}")


def test_c1_table_is_alive():
    assert (800, 6, 400.0, 2, 3) in T.c1_differing()


def test_c2_threshold():
    """C2: float32(0.005) and the float32 below it are not kept, the float32 above it is."""
    c = T.c2_case()
    conf, mask, kept = check_cells(c)
    assert kept.tolist() == [3] and mask[0].tolist() == [0, 0, 1 << 2, 0, 1 << 4, 1 << 5]


def test_c3_reduction():
    """C3: 600 detections per image (three passes of 256 threads) into three cells; float64 products with weights 0.7, 1/3, 1.0;
    the mask ORs every label, 31 included; images 0 / 1 / 2 use weight rows 2 / 0 / 1; image 2 keeps nothing."""
    c = T.c3_case()
    conf, mask, kept = check_cells(c)
    assert kept[2] == 0 and not conf[2].any() and not mask[2].any()
    assert (np.count_nonzero(conf[:2], axis=1) == 3).all() and kept[0] == kept[1] == 560
    assert (mask[0] >> np.uint32(31)).any() and not np.array_equal(conf[0], conf[1])
    s32 = c["scores"][0].astype(np.float32)
    f32_products = (s32 * c["weights"][2][c["labels"][0]].astype(np.float32)).astype(np.float64)
    assert not np.isin(conf[0][conf[0] > 0], f32_products).all()          # a float32 product is another number


@pytest.mark.parametrize("rows,cols,npatch", [(1, 1, 1), (64, 64, 1), (64, 64, 300), (1, 1, 300)])
def test_c4_grid_limits(rows, cols, npatch):
    """C4: the smallest grid and the largest the LDS arrays hold (4096 cells), with one detection per image and with 300."""
    check_cells(T.c4_case(rows, cols, npatch))


def test_c4_too_many_cells_is_refused(lib):
    c = T.c4_case(1, 4097)
    conf, mask, kept = run_cells(c, expect_rc=1)
    assert b"1..4096 cells" in lib[1].tstar_last_error()
    assert (conf == -1.0).all() and (mask == np.uint32(0xFFFFFFFF)).all() and (kept == -1).all()      # nothing launched
