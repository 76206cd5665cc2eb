"""Helpers of tests/test_owl_tail_reference.py (CPU) and tests/test_gpu_owl_tail.py (GPU): the OWL-ViT / OWLv2 detector TAIL --
everything tstar_owl_score runs after the encoder -- restated step by step in numpy float64, the same formulas in float32
torch (the yardstick the kernels' bounds are measured with), crafted head weights, query sets and scenarios.

The float64 statements are written from HF's formulas, as cited in csrc/heads.hip and csrc/rowops.hip:
  * merge     modeling_owlvit.py image_text_embedder: post-LayerNorm, class token times patch tokens, detection LayerNorm
  * class     OwlViTClassPredictionHead.forward after dense0: both sides / (norm + 1e-6), dot, (sim + shift) * (ELU(scale) + 1),
              masked queries = finfo(float32).min
  * box       OwlViTBoxPredictionHead dense2, + box_bias, sigmoid
  * post      image_processing_owlvit.py post_process_object_detection: max / argmax over queries (first maximum), sigmoid,
              centre form -> corner form times the image size (OWLv2: times max(H, W) on both axes)
  * objectness  Owlv2ForObjectDetection.objectness_predictor's dense2, [..., 0]
  * cells     TStarSearcher.imageGridScoreFunction's loop, with the numpy-1.26 promotions made explicit (cell_reduce_ref)
Nothing here is shared with the code under test.
"""
import math

import numpy as np

D, PROJ, MAXQ = 768, 512, 32
F32_MIN = float(np.finfo(np.float32).min)                   # -FLT_MAX
EPS32 = float(np.finfo(np.float32).eps)                     # 2^-23: one float32 ulp of 1.0
THR = np.float32(0.005)


def _unit(rs, *shape):
    """Unit-variance uniform float64 from numpy's frozen legacy stream."""
    return (rs.random_sample(shape) - 0.5) * math.sqrt(12.0)


# ----------------------------------------------------------------------------------------------- crafted weights and queries
def crafted_tail(family="owlvit", seed=5):
    """HF state-dict entries of the tail, to be laid over a synthetic state dict before ``pack_blob``: LayerNorm weights and
    biases that are not 1 / 0, shift / scale heads of a size that puts the scale pre-activation on both ELU branches
    (std 0.55 on unit-variance feats), a dense2 box head whose output competes with box_bias.  OWLv2: the post-LayerNorm bias
    is ZERO (a constant token row then gives an all-zero product with the class token) and the objectness dense2 is set."""
    rs = np.random.RandomState(seed)
    f = np.float32
    vm = family + ".vision_model."
    sd = {
        vm + "embeddings.class_embedding": (0.5 * _unit(rs, D)).astype(f),
        vm + "post_layernorm.weight": (1.0 + 0.2 * _unit(rs, D)).astype(f),
        vm + "post_layernorm.bias": (0.1 * _unit(rs, D)).astype(f),
        "layer_norm.weight": (1.0 + 0.2 * _unit(rs, D)).astype(f),
        "layer_norm.bias": (0.1 * _unit(rs, D)).astype(f),
        "class_head.logit_shift.weight": (0.02 * _unit(rs, 1, D)).astype(f),
        "class_head.logit_shift.bias": np.array([0.1], f),
        "class_head.logit_scale.weight": (0.02 * _unit(rs, 1, D)).astype(f),
        "class_head.logit_scale.bias": np.array([0.2], f),
        "box_head.dense2.weight": (0.05 * _unit(rs, 4, D)).astype(f),
        "box_head.dense2.bias": (0.1 * _unit(rs, 4)).astype(f),
    }
    if family == "owlv2":
        sd[vm + "post_layernorm.bias"] = np.zeros(D, f)
        sd["objectness_head.dense2.weight"] = (0.05 * _unit(rs, 1, D)).astype(f)
        sd["objectness_head.dense2.bias"] = np.array([0.3], f)
    return sd


def tail_weights(crafted, geometry):
    """The crafted entries under the blob's short names, plus the run's box_bias: what the handle holds for the tail."""
    from tstar_amd import weights as W
    vm = geometry.prefix + "vision_model."
    w = dict(class_emb=crafted[vm + "embeddings.class_embedding"], post_ln_w=crafted[vm + "post_layernorm.weight"],
             post_ln_b=crafted[vm + "post_layernorm.bias"], det_ln_w=crafted["layer_norm.weight"], det_ln_b=crafted["layer_norm.bias"],
             shift_w=crafted["class_head.logit_shift.weight"].reshape(D), shift_b=crafted["class_head.logit_shift.bias"],
             scale_w=crafted["class_head.logit_scale.weight"].reshape(D), scale_b=crafted["class_head.logit_scale.bias"],
             box2_w=crafted["box_head.dense2.weight"], box2_b=crafted["box_head.dense2.bias"], box_bias=W.compute_box_bias(geometry))
    if geometry.family == "owlv2":
        w["obj2_w"] = crafted["objectness_head.dense2.weight"].reshape(D)
        w["obj2_b"] = crafted["objectness_head.dense2.bias"]
    return w


def query_sets(seed=6):
    """slot -> (raw query embeddings float32 [Q, 512], mask uint8 [Q], class weights float64 [Q]).  Rows are NOT unit length (the
    q / (|q| + 1e-6) kernel is part of what is tested).
      0: Q = 32; padded (mask 0) queries first, in the middle and last (0, 15, 31); query 7 is the zero vector
      1: Q = 4, all real
      2: Q = 3, the middle one padded          3: Q = 4, ALL padded
      4: Q = 32, all real; row 17 = row 3 and row 31 = row 0 (bit-equal logits)
      5: Q = 1                                  6: Q = 4, the first two padded"""
    rs = np.random.RandomState(seed)

    def q(n):
        return (_unit(rs, n, PROJ) * rs.uniform(0.3, 3.0, (n, 1))).astype(np.float32)

    def wts(n):
        return rs.uniform(0.1, 1.0, n)

    s = {}
    m0 = np.ones(32, np.uint8)
    m0[[0, 15, 31]] = 0
    q0 = q(32)
    q0[7] = 0.0
    s[0] = (q0, m0, wts(32))
    s[1] = (q(4), np.ones(4, np.uint8), wts(4))
    s[2] = (q(3), np.array([1, 0, 1], np.uint8), wts(3))
    s[3] = (q(4), np.zeros(4, np.uint8), wts(4))
    q4 = q(32)
    q4[17], q4[31] = q4[3], q4[0]
    s[4] = (q4, np.ones(32, np.uint8), wts(32))
    s[5] = (q(1), np.ones(1, np.uint8), wts(1))
    s[6] = (q(4), np.array([0, 0, 1, 1], np.uint8), wts(4))
    return s


EMPTY_SLOT = 9                                              # never installed


# ----------------------------------------------------------------------------------------------- float64 statements
def ln64(x, w, b, eps=1e-5):
    x = np.asarray(x, np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def merge64(x, B, ntok, w):
    """x [B * ntok, 768] -> feats [B * (ntok - 1), 768]."""
    e = ln64(np.asarray(x, np.float64).reshape(B, ntok, D), w["post_ln_w"], w["post_ln_b"])
    return ln64(e[:, 1:] * e[:, :1], w["det_ln_w"], w["det_ln_b"]).reshape(B * (ntok - 1), D)


def _elu_plus_one(pre):
    return np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0.0))) + 1.0


def scale_pre64(feats, w):
    return np.asarray(feats, np.float64) @ w["scale_w"].astype(np.float64) + float(w["scale_b"][0])


def shift64(feats, w):
    return np.asarray(feats, np.float64) @ w["shift_w"].astype(np.float64) + float(w["shift_b"][0])


def class_logits64(feats, cls, q_raw, qmask, w):
    """feats [n, 768], cls [n, 512] (dense0's output), raw queries [Q, 512] -> logits [n, Q]."""
    c = np.asarray(cls, np.float64)
    c = c / (np.sqrt((c * c).sum(-1, keepdims=True)) + 1e-6)
    q = np.asarray(q_raw, np.float64)
    q = q / (np.sqrt((q * q).sum(-1, keepdims=True)) + 1e-6)
    lg = (c @ q.T + shift64(feats, w)[:, None]) * _elu_plus_one(scale_pre64(feats, w))[:, None]
    lg[:, np.asarray(qmask) == 0] = F32_MIN
    return lg


def box_pre64(boxh, patch, w):
    return np.asarray(boxh, np.float64) @ w["box2_w"].astype(np.float64).T + w["box2_b"].astype(np.float64) + w["box_bias"].astype(np.float64)[patch]


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def box_scale(family, H, W):
    """(sx, sy): OWL-ViT scales the relative boxes by (W, H), OWLv2 by max(H, W) on both axes."""
    return (float(max(H, W)),) * 2 if family == "owlv2" else (float(W), float(H))


def detect64(case, w, sets, npatch, family):
    """The whole detect_rows step of one case in float64.  -> dict of scores [rows], labels [rows], xyxy / cxcywh [rows, 4],
    logits (list per image, [np, Q of its set]), margin [rows] (top-1 minus top-2 logit; inf for a single query)."""
    rows = case["feats"].shape[0]
    B = rows // npatch
    sx, sy = box_scale(family, case["H"], case["W"])
    patch = np.arange(rows) % npatch
    cxcywh = sigmoid64(box_pre64(case["boxh"], patch, w))
    cx, cy, bw, bh = cxcywh.T
    xyxy = np.stack([(cx - 0.5 * bw) * sx, (cy - 0.5 * bh) * sy, (cx + 0.5 * bw) * sx, (cy + 0.5 * bh) * sy], 1)
    logits, scores, labels, margin = [], np.zeros(rows), np.zeros(rows, np.int64), np.full(rows, np.inf)
    for b in range(B):
        q_raw, qmask, _ = sets[case["sets"][b]]
        r = slice(b * npatch, (b + 1) * npatch)
        lg = class_logits64(case["feats"][r], case["cls"][r], q_raw, qmask, w)
        logits.append(lg)
        labels[r] = lg.argmax(-1)                            # first maximum
        best = lg.max(-1)
        scores[r] = sigmoid64(best)
        if lg.shape[1] > 1:
            top = np.sort(lg, -1)
            margin[r] = top[:, -1] - top[:, -2]
    return dict(scores=scores, labels=labels, xyxy=xyxy, cxcywh=cxcywh, logits=logits, margin=margin)


def row_dot64(h, w):
    return np.asarray(h, np.float64) @ w["obj2_w"].astype(np.float64) + float(w["obj2_b"][0])


# ----------------------------------------------------------------------------------------------- the same in float32 torch
def merge_f32(x, B, ntok, w):
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    e = F.layer_norm(t(x).view(B, ntok, D), (D,), t(w["post_ln_w"]), t(w["post_ln_b"]), 1e-5)
    return F.layer_norm(e[:, 1:] * e[:, :1], (D,), t(w["det_ln_w"]), t(w["det_ln_b"]), 1e-5).reshape(B * (ntok - 1), D).numpy()


def detect_f32(case, w, sets, npatch, family):
    """detect64's quantities through float32 torch ops, written like oracle/owl_ref.heads / post_process."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    rows = case["feats"].shape[0]
    B = rows // npatch
    sx, sy = box_scale(family, case["H"], case["W"])
    feats = t(case["feats"])
    bias = t(w["box_bias"])[torch.arange(rows) % npatch]
    cxcywh = torch.sigmoid(F.linear(t(case["boxh"]), t(w["box2_w"]), t(w["box2_b"])) + bias)
    cx, cy, bw, bh = cxcywh.unbind(-1)
    xyxy = torch.stack([cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh], -1) * torch.tensor([sx, sy, sx, sy])
    shift = F.linear(feats, t(w["shift_w"]).view(1, -1), t(w["shift_b"]))
    scale = F.elu(F.linear(feats, t(w["scale_w"]).view(1, -1), t(w["scale_b"]))) + 1
    c = t(case["cls"])
    c = c / (torch.linalg.norm(c, dim=-1, keepdim=True) + 1e-6)
    logits, scores, labels = [], [], []
    for b in range(B):
        q_raw, qmask, _ = sets[case["sets"][b]]
        q = t(q_raw)
        q = q / (torch.linalg.norm(q, dim=-1, keepdim=True) + 1e-6)
        r = slice(b * npatch, (b + 1) * npatch)
        lg = (c[r] @ q.t() + shift[r]) * scale[r]
        lg = torch.where(torch.from_numpy(np.asarray(qmask)).view(1, -1) == 0, torch.finfo(torch.float32).min, lg)
        v, lab = torch.max(lg, dim=-1)
        logits.append(lg.numpy())
        scores.append(torch.sigmoid(v).numpy())
        labels.append(lab.numpy())
    return dict(scores=np.concatenate(scores), labels=np.concatenate(labels), xyxy=xyxy.numpy(), cxcywh=cxcywh.numpy(), logits=logits)


def row_dot_f32(h, w):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return (torch.nn.functional.linear(t(h), t(w["obj2_w"]).view(1, -1), t(w["obj2_b"]))[:, 0]).numpy()


def bound(f32_value, ref64, where=None):
    """(bound, measured): 4 x the worst error of the float32 evaluation against float64 (the kernels sum in wave-shuffle order,
    torch in its own), plus one float32 ulp of the quantity's largest magnitude: over a few dozen elements the measured figure
    can be zero by luck (a saturated sigmoid is exactly 1.0 in float32 torch and 1 - 4e-44 in float64), and no float32 result can
    be asked to be closer than its own spacing."""
    ref = np.asarray(ref64, np.float64)
    err = np.abs(np.asarray(f32_value, np.float64) - ref)
    if where is not None:
        err, ref = err[where], ref[where]
    measured = float(err.max()) if err.size else 0.0
    return 4.0 * measured + EPS32 * (float(np.abs(ref).max()) if ref.size else 0.0), measured


def unmasked(case, sets, npatch):
    """Per image the boolean [np, Q] of logits that are real numbers (not the padded queries' -FLT_MAX)."""
    return [np.broadcast_to(sets[s][1] != 0, (npatch, len(sets[s][1]))) for s in case["sets"]]


# ----------------------------------------------------------------------------------------------- detect_rows scenarios
def _rows(rs, rows):
    feats = _unit(rs, rows, D).astype(np.float32)                       # unit variance, like a LayerNorm's output
    cls = (_unit(rs, rows, PROJ) * rs.uniform(0.2, 5.0, (rows, 1))).astype(np.float32)
    boxh = (0.6 * _unit(rs, rows, D)).astype(np.float32)
    return feats, cls, boxh


def case_random(npatch, B, slots, seed, H=95, W=200):
    feats, cls, boxh = _rows(np.random.RandomState(seed), B * npatch)
    return dict(feats=feats, cls=cls, boxh=boxh, sets=list(slots), H=H, W=W)


D1_SEED = 21


def case_d1(npatch):
    """D1: B = 3, Q = 4, every query real."""
    return case_random(npatch, 3, [1, 1, 1], D1_SEED)


def case_d2(npatch, sets, slot):
    """D2: slot 0 (Q = 32; padded queries 0, 15, 31; zero query 7) or slot 3 (all padded).  The class rows of the first three
    patches ARE the padded queries 0, 15 and 31: without the mask they would win."""
    c = case_random(npatch, 3, [slot] * 3, 22)
    c["cls"][0], c["cls"][1], c["cls"][2] = sets[0][0][0], sets[0][0][15], sets[0][0][31]
    return c


def case_d3(npatch, sets):
    """D3: slot 4.  Rows 0-5 carry query 3 (= query 17) as their class embedding, rows 6-11 query 0 (= query 31), scaled."""
    c = case_random(npatch, 3, [4] * 3, 23)
    q = sets[4][0]
    for r in range(6):
        c["cls"][r] = q[3] * np.float32(0.5 + r)
        c["cls"][6 + r] = q[0] * np.float32(0.25 * (1 + r))
    return c


def case_d4(npatch):
    """D4: four images scored against slots 2, 0, 2, 5 (Q = 3 / 32 / 3 / 1)."""
    return case_random(npatch, 4, [2, 0, 2, 5], 24)


def case_d5(npatch):
    """D5: slot 6 (the first two queries padded); class rows 1, 4 and the last are all zero."""
    c = case_random(npatch, 3, [6] * 3, 25)
    c["zero_rows"] = [1, 4, 3 * npatch - 1]
    c["cls"][c["zero_rows"]] = 0.0
    return c


D6_PRE = (-20.0, -1e-3, 0.0, 1e-3, 5.0)


def case_d6(npatch, w):
    """D6: one image; row i < 5 is moved along scale_w so that the scale head's pre-activation is D6_PRE[i] (to float32
    rounding of the row: the float64 statement reads the rounded row)."""
    c = case_random(npatch, 1, [1], 26)
    sw = w["scale_w"].astype(np.float64)
    for i, x in enumerate(D6_PRE):
        f = c["feats"][i].astype(np.float64)
        f = f + (x - float(w["scale_b"][0]) - f @ sw) / (sw @ sw) * sw
        c["feats"][i] = f.astype(np.float32)
    return c


D7_TARGETS = ((100.0, 100.0, 100.0, 100.0), (-100.0, -100.0, -100.0, -100.0), (0.0, 0.0, 0.0, 0.0), None,
              (100.0, 100.0, -100.0, -100.0), (0.0, 0.0, 100.0, 100.0))


def case_d7(npatch, w, H, W):
    """D7: six rows whose four pre-sigmoid box values (dense2 + bias + box_bias of the row's patch) are D7_TARGETS; None: the box
    head's input is zero, so the box is sigmoid(dense2 bias + box_bias) alone."""
    rows = len(D7_TARGETS)
    assert rows % npatch == 0
    c = case_random(npatch, rows // npatch, [1] * (rows // npatch), 27, H, W)
    W2 = w["box2_w"].astype(np.float64)
    G = W2 @ W2.T
    for r, tg in enumerate(D7_TARGETS):
        if tg is None:
            c["boxh"][r] = 0.0
            continue
        rest = np.asarray(tg) - w["box2_b"].astype(np.float64) - w["box_bias"].astype(np.float64)[r % npatch]
        c["boxh"][r] = (np.linalg.solve(G, rest) @ W2).astype(np.float32)
    return c


# ----------------------------------------------------------------------------------------------- merge scenarios
def case_m1(B, ntok, seed=31):
    """Random tokens, a distinct class-token row per image."""
    rs = np.random.RandomState(seed)
    return (_unit(rs, B * ntok, D) * rs.uniform(0.5, 2.0, (B * ntok, 1)) + rs.uniform(-1, 1, (B * ntok, 1))).astype(np.float32)


M2_CONSTANTS = (2.0, -0.5, 0.0)                              # sums of 768 of them, and the sum times float32(1 / 768), are exact


def case_m2(ntok, seed=32):
    """One image of ntok >= 6 tokens: patch rows 0-2 constant (M2_CONSTANTS), patch rows 3-4 with mean 1e3 and unit spread."""
    rs = np.random.RandomState(seed)
    x = _unit(rs, ntok, D).astype(np.float32)
    for i, c in enumerate(M2_CONSTANTS):
        x[1 + i] = c
    x[4] = (1e3 + _unit(rs, D)).astype(np.float32)
    x[5] = (-1e3 + _unit(rs, D)).astype(np.float32)
    return x


# ----------------------------------------------------------------------------------------------- the cell step
def cell_reduce_ref(scores, labels, xyxy, weights, image_set, W, H, rows, cols, thr=THR):
    """imageGridScoreFunction's loop over the detections with score > thr of every image, with the promotions of the
    reference's pinned numpy 1.26 written out: float32 add then halve; np.float64(centre) // Python-float cell size (numpy's
    float64 floor_divide); min(., n - 1); float64 product score * weight; max.  -> (conf float64 [B, rows * cols],
    mask uint32 [B, rows * cols]: bit q set where a kept detection of label q fell into the cell, n_kept int32 [B]).
    Box centres are >= 0 (a sigmoid times a positive size); a negative centre would index the map from its end in the
    reference and is outside what the kernel promises."""
    scores = np.asarray(scores, np.float32)
    xyxy = np.asarray(xyxy, np.float32)
    B, npatch = scores.shape
    cw, ch = W / cols, H / rows                              # Python floats
    conf = np.zeros((B, rows * cols), np.float64)
    mask = np.zeros((B, rows * cols), np.uint32)
    kept = np.zeros(B, np.int32)
    for b in range(B):
        wt = np.asarray(weights, np.float64)[0 if image_set is None else image_set[b]]
        for p in np.flatnonzero(scores[b] > np.float32(thr)):
            x0, y0, x1, y1 = xyxy[b, p]
            cx = np.float32(x0 + x1) / np.float32(2)
            cy = np.float32(y0 + y1) / np.float32(2)
            gx = min(int(np.float64(cx) // cw), cols - 1)
            gy = min(int(np.float64(cy) // ch), rows - 1)
            lab = int(labels[b, p])
            cell = gy * cols + gx
            conf[b, cell] = max(conf[b, cell], float(np.float64(scores[b, p]) * wt[lab]))
            mask[b, cell] |= np.uint32(1) << np.uint32(lab)
            kept[b] += 1
    return conf, mask, kept


def naive_cell(c, size, n):
    """floor(double(c) / (size / n)), clamped: what the kernels computed before np_floor_divide."""
    return min(int(math.floor(float(np.float32(c)) / (size / n))), n - 1)


def numpy_cell(c, size, n):
    return min(int(np.float64(np.float32(c)) // (size / n)), n - 1)


C1_AXES = ((800, 3), (800, 6), (800, 7), (800, 15), (800, 24), (600, 7), (427, 4), (960, 7), (1000, 24))


def c1_boxes(size, n):
    """(lo, hi) float32 pairs of one axis of `size` pixels cut into n cells: for every border k * size / n, k = 0 .. n + 1 (the
    last two are the image edge and one cell beyond it: both clamp to the last cell), the float32 nearest to the border and its
    two float32 neighbours as DEGENERATE boxes (lo = hi, so the centre is that very number), and ordinary boxes around the same
    three numbers whose float32 sum rounds (lo = c - 37.3, hi = c + 37.3 in float32, clipped at 0); then (0.1, size - 0.1)."""
    cw = size / n
    out = []
    for k in range(n + 2):
        c0 = np.float32(k * cw)
        for c in (np.nextafter(c0, np.float32(-1)), c0, np.nextafter(c0, np.float32(4 * size))):
            c = np.float32(max(c, 0.0))
            out.append((c, c))
            out.append((np.float32(max(c - np.float32(37.3), 0.0)), np.float32(c + np.float32(37.3))))
    out.append((np.float32(0.1), np.float32(size - 0.1)))
    return np.asarray(out, np.float32)


def c1_centres(size, n):
    b = c1_boxes(size, n)
    return (b[:, 0] + b[:, 1]) / np.float32(2)


def c1_case(size, n):
    """One image per box of c1_boxes, two detections each: detection 0 has the box on the x axis (label 3, y fixed inside cell
    row 0), detection 1 on the y axis (label 17, x fixed inside the last cell column).  W = H = size, rows = cols = n."""
    bx = c1_boxes(size, n)
    B = len(bx)
    rs = np.random.RandomState(size + n)
    scores = rs.uniform(0.01, 0.99, (B, 2)).astype(np.float32)
    labels = np.tile(np.array([3, 17], np.int32), (B, 1))
    xyxy = np.zeros((B, 2, 4), np.float32)
    inside = np.float32(0.25 * size / n)
    xyxy[:, 0, 0], xyxy[:, 0, 2] = bx[:, 0], bx[:, 1]
    xyxy[:, 0, 1] = xyxy[:, 0, 3] = inside
    xyxy[:, 1, 1], xyxy[:, 1, 3] = bx[:, 0], bx[:, 1]
    xyxy[:, 1, 0] = xyxy[:, 1, 2] = np.float32(size) - inside
    weights = np.zeros((1, MAXQ), np.float64)
    weights[0, 3], weights[0, 17] = 0.7, 1.0 / 3.0
    return dict(scores=scores, labels=labels, xyxy=xyxy, weights=weights, image_set=None, W=size, H=size, rows=n, cols=n, thr=THR)


def c1_differing():
    """[(size, n, centre, numpy's cell, floor(a / b)'s cell)] over the whole C1 table, after the clamp."""
    out = []
    for size, n in C1_AXES:
        for c in c1_centres(size, n):
            a, b = numpy_cell(c, size, n), naive_cell(c, size, n)
            if a != b:
                out.append((size, n, float(c), a, b))
    return out


def c2_case():
    """C2: scores at float32(0.005) and its two float32 neighbours (and 0, 1): only those ABOVE the threshold count."""
    t = THR
    scores = np.array([[np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1)), 0.0, 1.0, np.nextafter(t, np.float32(1))]], np.float32)
    labels = np.array([[0, 1, 2, 3, 4, 5]], np.int32)
    xyxy = np.zeros((1, 6, 4), np.float32)
    xyxy[0, :, 0] = xyxy[0, :, 2] = (np.arange(6) + 0.5) * (200.0 / 6)            # detection k in cell k
    xyxy[0, :, 1] = xyxy[0, :, 3] = 10.0
    weights = np.full((1, MAXQ), 0.9, np.float64)
    return dict(scores=scores, labels=labels, xyxy=xyxy, weights=weights, image_set=None, W=200, H=95, rows=1, cols=6, thr=THR)


def c3_case():
    """C3: B = 3, np = 600 (more than two passes of 256 threads), a 3 x 5 grid on 200 x 95.  Image 0: every detection in one of
    three cells, labels 0 .. 31 (label 31 among them), weights 0.7, 1/3 and 1.0 (and others) from weight row 2; image 1: the
    same detections with weight row 0; image 2: nothing above the threshold."""
    rs = np.random.RandomState(41)
    B, npatch, rows, cols, W, H = 3, 600, 3, 5, 200, 95
    scores = rs.uniform(0.006, 0.999, (B, npatch)).astype(np.float32)
    scores[0, rs.choice(npatch, 40, replace=False)] = rs.uniform(0.0, 0.005, 40).astype(np.float32)
    scores[1] = scores[0]
    scores[2] = rs.uniform(0.0, 0.005, npatch).astype(np.float32)
    scores[2, 7] = THR                                        # exactly the threshold: not kept
    labels = rs.randint(0, 32, (B, npatch)).astype(np.int32)
    labels[:, 599] = 31
    labels[1] = labels[0]
    cells = np.array([(0, 0), (1, 3), (2, 4)])[rs.randint(0, 3, npatch)]
    cx = (cells[:, 1] + rs.uniform(0.05, 0.95, npatch)) * (W / cols)
    cy = (cells[:, 0] + rs.uniform(0.05, 0.95, npatch)) * (H / rows)
    half = rs.uniform(0.0, 3.0, (npatch, 2))
    one = np.stack([cx - half[:, 0], cy - half[:, 1], cx + half[:, 0], cy + half[:, 1]], 1).astype(np.float32)
    xyxy = np.broadcast_to(np.maximum(one, 0.0), (B, npatch, 4)).copy()
    weights = rs.uniform(0.05, 1.0, (3, MAXQ))
    weights[2, :3] = (0.7, 1.0 / 3.0, 1.0)
    weights[0, :3] = (1.0, 0.5, 0.1)
    return dict(scores=scores, labels=labels, xyxy=xyxy, weights=weights, image_set=[2, 0, 1], W=W, H=H, rows=rows, cols=cols, thr=THR)


def c4_case(rows, cols, npatch=1, B=2, seed=42):
    """C4: a rows x cols grid on 640 x 360 with np detections per image at seeded places."""
    rs = np.random.RandomState(seed + rows + cols)
    W, H = 640, 360
    scores = rs.uniform(0.1, 0.9, (B, npatch)).astype(np.float32)
    labels = rs.randint(0, 32, (B, npatch)).astype(np.int32)
    c = np.stack([rs.uniform(0, W, (B, npatch)), rs.uniform(0, H, (B, npatch))], -1)
    xyxy = np.concatenate([np.maximum(c - 2.0, 0.0), c + 2.0], -1).astype(np.float32)
    return dict(scores=scores, labels=labels, xyxy=xyxy, weights=rs.uniform(0.05, 1.0, (1, MAXQ)), image_set=None, W=W, H=H,
                rows=rows, cols=cols, thr=THR)
