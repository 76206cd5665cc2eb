"""CPU pins of tests/owl_tail_util.py, the float64 restatement the GPU tests of the detector tail (tests/test_gpu_owl_tail.py) compare
the kernels with: it agrees with oracle/owl_ref's class-head, box-head and merge code and with HF's head modules, and its cell step
equals oracle.searcher_ref.image_grid_score and TStarSearcher.imageGridScoreFunction on the border table of scenario C1 -- centres
included where floor(a / b) and numpy's float64 floor_divide give different cells."""
import math
import types

import numpy as np
import pytest
import torch

import owl_tail_util as T
from oracle import owl_ref, searcher_ref
from tstar_amd import weights as W

G = W.with_input_size(W.B32, (64, 96))                      # the GPU tests' scorer: 2 x 3 patches


@pytest.fixture(scope="module")
def tail():
    return T.tail_weights(T.crafted_tail("owlvit"), G), T.query_sets()


def _head_inputs(w, rows, seed):
    """feats, and cls / boxh computed from them with oracle/owl_ref.heads' own float32 statements on small random matrices."""
    import torch.nn.functional as F
    rs = np.random.RandomState(seed)
    feats = T._unit(rs, rows, T.D).astype(np.float32)
    full = dict(w)
    full.update(cls_w=(0.05 * T._unit(rs, T.PROJ, T.D)).astype(np.float32), cls_b=(0.02 * T._unit(rs, T.PROJ)).astype(np.float32))
    for k in ("box0", "box1"):
        full[k + "_w"] = (0.05 * T._unit(rs, T.D, T.D)).astype(np.float32)
        full[k + "_b"] = (0.02 * T._unit(rs, T.D)).astype(np.float32)
    t = torch.from_numpy
    cls = F.linear(t(feats), t(full["cls_w"]), t(full["cls_b"])).numpy()
    b = F.gelu(F.linear(t(feats), t(full["box0_w"]), t(full["box0_b"])))
    boxh = F.gelu(F.linear(b, t(full["box1_w"]), t(full["box1_b"]))).numpy()
    return feats, cls, boxh, full


@pytest.mark.parametrize("slot", [0, 1, 2, 4, 6])
def test_heads_agree_with_oracle(tail, slot):
    """class head + box head: |float64 restatement - oracle/owl_ref.heads| within what float32 needs against float64 (the bound of
    owl_tail_util.bound, measured with the restatement's own float32 twin)."""
    w, sets = tail
    npatch, B = G.npatch, 2
    feats, cls, boxh, full = _head_inputs(w, B * npatch, 50 + slot)
    q_raw, qmask, _ = sets[slot]
    with torch.no_grad():
        lg, bx = owl_ref.heads(torch.from_numpy(feats).view(B, npatch, T.D), torch.from_numpy(q_raw), full, qmask)
    case = dict(feats=feats, cls=cls, boxh=boxh, sets=[slot] * B, H=95, W=200)
    r64, r32 = T.detect64(case, w, sets, npatch, "owlvit"), T.detect_f32(case, w, sets, npatch, "owlvit")
    real = np.concatenate(T.unmasked(case, sets, npatch))
    ref_lg, f32_lg, got_lg = np.concatenate(r64["logits"]), np.concatenate(r32["logits"]), lg.numpy().reshape(B * npatch, -1)
    bl, ml = T.bound(f32_lg, ref_lg, real)
    bb, mb = T.bound(r32["cxcywh"], r64["cxcywh"])
    el, eb = np.abs(got_lg - ref_lg)[real].max(), np.abs(bx.numpy().reshape(-1, 4) - r64["cxcywh"]).max()
    print(f"slot {slot}: logits err {el:.3g} (float32 twin {ml:.3g}, bound {bl:.3g}); boxes err {eb:.3g} (twin {mb:.3g}, bound {bb:.3g})")
    assert el <= bl and eb <= bb
    assert (got_lg[~real] == np.float32(T.F32_MIN)).all() and (ref_lg[~real] == T.F32_MIN).all()
    (_, dense) = owl_ref.post_process(lg, bx, 95, 200)
    assert np.abs(dense[0].reshape(-1) - r64["scores"]).max() <= T.bound(r32["scores"], r64["scores"])[0]
    assert np.abs(dense[2].reshape(-1, 4) - r64["xyxy"]).max() <= T.bound(r32["xyxy"], r64["xyxy"])[0]
    clear = r64["margin"] > 2 * bl
    assert np.array_equal(dense[1].reshape(-1)[clear], r64["labels"][clear])


def test_heads_agree_with_hf_modules(tail):
    """The same against HF's own OwlViTClassPredictionHead / OwlViTBoxPredictionHead."""
    transformers = pytest.importorskip("transformers")
    from transformers.models.owlvit import modeling_owlvit as M
    w, sets = tail
    cfg = transformers.OwlViTConfig()
    torch.manual_seed(3)
    ch, bh = M.OwlViTClassPredictionHead(cfg).eval(), M.OwlViTBoxPredictionHead(cfg).eval()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    with torch.no_grad():
        ch.logit_shift.weight.copy_(t(w["shift_w"]).view(1, -1)); ch.logit_shift.bias.copy_(t(w["shift_b"]))
        ch.logit_scale.weight.copy_(t(w["scale_w"]).view(1, -1)); ch.logit_scale.bias.copy_(t(w["scale_b"]))
        bh.dense2.weight.copy_(t(w["box2_w"])); bh.dense2.bias.copy_(t(w["box2_b"]))
        for lin in (bh.dense0, bh.dense1):
            lin.weight.mul_(T.D ** -0.5)
        npatch, B, slot = G.npatch, 2, 0
        feats = torch.from_numpy(T._unit(np.random.RandomState(60), B, npatch, T.D).astype(np.float32))
        q_raw, qmask, _ = sets[slot]
        lg, _ = ch(feats, t(q_raw)[None].expand(B, -1, -1), torch.from_numpy(qmask.astype(np.int64))[None].expand(B, -1))
        cls = ch.dense0(feats)
        boxh = bh.gelu(bh.dense1(bh.gelu(bh.dense0(feats))))
        boxes = torch.sigmoid(bh(feats) + t(w["box_bias"]))
    case = dict(feats=feats.numpy().reshape(-1, T.D), cls=cls.numpy().reshape(-1, T.PROJ), boxh=boxh.numpy().reshape(-1, T.D), sets=[slot] * B, H=95, W=200)
    r64, r32 = T.detect64(case, w, sets, npatch, "owlvit"), T.detect_f32(case, w, sets, npatch, "owlvit")
    real = np.concatenate(T.unmasked(case, sets, npatch))
    ref_lg, got = np.concatenate(r64["logits"]), lg.numpy().reshape(B * npatch, -1)
    assert np.abs(got - ref_lg)[real].max() <= T.bound(np.concatenate(r32["logits"]), ref_lg, real)[0]
    assert (got[~real] == np.float32(T.F32_MIN)).all()
    assert np.abs(boxes.numpy().reshape(-1, 4) - r64["cxcywh"]).max() <= T.bound(r32["cxcywh"], r64["cxcywh"])[0]


def test_merge_agrees_with_oracle(tail, monkeypatch):
    """merge64 against the post-LayerNorm / class-token merge / detection-LayerNorm lines of oracle/owl_ref.vision_features (itself
    bit-equal to HF, tests/test_oracle_owl.py), reached with the encoder layers replaced by the identity."""
    import torch.nn.functional as F
    w, _ = tail
    rs = np.random.RandomState(70)
    full = dict(w)
    full.update(patch_w=(0.02 * T._unit(rs, W.V_D, 3 * W.PATCH * W.PATCH)).astype(np.float32), pos_emb=(0.5 * T._unit(rs, W.NTOK, W.V_D)).astype(np.float32),
                pre_ln_w=(1 + 0.1 * T._unit(rs, W.V_D)).astype(np.float32), pre_ln_b=(0.1 * T._unit(rs, W.V_D)).astype(np.float32))
    monkeypatch.setattr(owl_ref, "_encoder_layer", lambda x, *a, **k: x)
    B = 1
    px = torch.from_numpy(rs.standard_normal((B, 3, W.IMG, W.IMG)).astype(np.float32))
    t = torch.from_numpy
    with torch.no_grad():
        got = owl_ref.vision_features(px, full).numpy().reshape(-1, W.V_D)
        x = F.conv2d(px, t(full["patch_w"]).view(W.V_D, 3, W.PATCH, W.PATCH), stride=W.PATCH).flatten(2).transpose(1, 2)
        x = torch.cat([t(full["class_emb"]).expand(B, 1, -1), x], dim=1) + t(full["pos_emb"])
        x = F.layer_norm(x, (W.V_D,), t(full["pre_ln_w"]), t(full["pre_ln_b"]), W.LN_EPS).numpy().reshape(-1, W.V_D)
    ref = T.merge64(x, B, W.NTOK, w)
    b, m = T.bound(T.merge_f32(x, B, W.NTOK, w), ref)
    err = np.abs(got - ref).max()
    print(f"merge: err {err:.3g} (float32 twin {m:.3g}, bound {b:.3g})")
    assert err <= b


def test_d1_seed_leaves_clear_margins(tail):
    """D1's labels are compared wherever the float64 top-2 margin exceeds the logit bound; the seed keeps every row of the float32
    CPU evaluation clear of it (at most 5 % may be excluded)."""
    w, sets = tail
    case = T.case_d1(G.npatch)
    r64, r32 = T.detect64(case, w, sets, G.npatch, "owlvit"), T.detect_f32(case, w, sets, G.npatch, "owlvit")
    bl, _ = T.bound(np.concatenate(r32["logits"]), np.concatenate(r64["logits"]))
    clear = r64["margin"] > bl
    assert (~clear).mean() <= 0.05
    assert np.array_equal(r32["labels"][clear], r64["labels"][clear])
    assert len(set(r64["labels"].tolist())) > 1


def test_d6_rows_sit_where_they_should(tail):
    w, sets = tail
    case = T.case_d6(G.npatch, w)
    pre = T.scale_pre64(case["feats"], w)[:5]
    assert np.abs(pre - np.asarray(T.D6_PRE)).max() < 2e-6 and abs(pre[2]) < 2e-6


def test_d7_rows_sit_where_they_should(tail):
    w, _ = tail
    case = T.case_d7(G.npatch, w, 95, 200)
    pre = T.box_pre64(case["boxh"], np.arange(6) % G.npatch, w)
    for r, tg in enumerate(T.D7_TARGETS):
        if tg is not None:
            assert np.abs(pre[r] - np.asarray(tg)).max() < 1e-3
    assert np.abs(w["box_bias"]).max() > 5.0                 # a box_bias that matters: it moves a pre-sigmoid value by more than 5


# --------------------------------------------------------------------------------------------------------- the cell step
def _np_floor_divide(a, b):
    """csrc/common.h np_floor_divide, statement by statement."""
    mod = math.fmod(a, b)
    div = (a - mod) / b
    f = math.floor(div)
    return f + 1.0 if div - f > 0.5 else f


def test_c1_table_holds_centres_where_the_two_floors_differ():
    d = T.c1_differing()
    print(f"{len(d)} centres of the C1 table fall into another cell with floor(a / b): {d[:8]} ...")
    assert (800, 6, 400.0, 2, 3) in d                        # numpy 1.26: cell 2; floor(400.0 / 133.33333333333334): cell 3
    assert {(s, n) for s, n, *_ in d} >= {(800, 6), (800, 15), (800, 24)}     # interior borders that are whole pixels (the last border clamps)
    for size, n in T.C1_AXES:
        for c in T.c1_centres(size, n):
            assert _np_floor_divide(float(c), size / n) == float(np.float64(c) // (size / n)), (size, n, c)
            assert c >= 0


class _Det:
    def __init__(self, xyxy, labels, scores):
        self.xyxy, self.class_id, self.confidence = xyxy, labels, scores


@pytest.mark.parametrize("size,n", T.C1_AXES)
def test_cell_step_equals_oracle_and_host_path(size, n):
    """cell_reduce_ref == oracle.searcher_ref.image_grid_score == TStarSearcher.imageGridScoreFunction on every image of C1."""
    from tstar_amd.interface_searcher import TStarSearcher
    c = T.c1_case(size, n)
    conf, mask, kept = T.cell_reduce_ref(c["scores"], c["labels"], c["xyxy"], c["weights"], None, c["W"], c["H"], c["rows"], c["cols"])
    texts = [[f"c{q}"] for q in range(T.MAXQ)]
    o2w = {f"c{q}": float(c["weights"][0, q]) for q in range(T.MAXQ)}
    B = len(c["scores"])
    assert (kept == 2).all()
    dets = iter([_Det(c["xyxy"][b], c["labels"][b].astype(np.int64), c["scores"][b])] for b in range(B))
    stub = types.SimpleNamespace(heuristic=types.SimpleNamespace(texts=texts, inference_detector=lambda images, use_amp: next(dets)), object2weight=o2w)
    img = np.zeros((c["H"], c["W"], 1), np.uint8)
    host_conf, host_names = TStarSearcher.imageGridScoreFunction(stub, [img] * B, None, (n, n))
    for b in range(B):
        cm, names = searcher_ref.image_grid_score(c["xyxy"][b], c["labels"][b], c["scores"][b], texts, o2w, c["H"], c["W"], n, n)
        want = np.zeros(n * n, np.uint32)
        for cell, ns in enumerate(names):
            for nme in ns:
                want[cell] |= np.uint32(1) << np.uint32(int(nme[1:]))
        assert np.array_equal(cm.reshape(-1), conf[b]) and np.array_equal(want, mask[b]), (size, n, b, c["xyxy"][b])
        assert np.array_equal(host_conf[b].reshape(-1), conf[b]) and host_names[b] == names
