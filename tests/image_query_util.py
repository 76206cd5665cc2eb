"""Helpers of tests/test_image_query_host.py and tests/test_gpu_image_query.py: a numpy restatement of the query selection of
HF's ``embed_image_query`` (modeling_owlvit.py; modeling_owlv2.py is the same statements), HF's own statements as the witness,
and the crafted (class embeddings, boxes) cases of the selection kernel.

The restatement: corners, IoU / generalized IoU against the unit box, the 0.8 x max threshold and the selected set as plain
float32 elementwise operations (torch's bits: pinned in test_image_query_host.py); the mean embedding, ``mean_sim`` and the
arg-min in float64 (the only part that depends on a summation order)."""
import types

import numpy as np

PROJ = 512
F32 = np.float32
STATUS_IOU, STATUS_GIOU, STATUS_EMPTY = 0, 1, 2


# ----------------------------------------------------------------------------------------------------- the restatement
def iou_unit(boxes):
    """(iou, giou) float32 [np] of cxcywh boxes float32 [np, 4] against the unit box [0, 0, 1, 1]."""
    b = np.ascontiguousarray(boxes, dtype=F32)
    half, zero, one = F32(0.5), F32(0), F32(1)
    x0, y0 = b[:, 0] - half * b[:, 2], b[:, 1] - half * b[:, 3]
    x1, y1 = b[:, 0] + half * b[:, 2], b[:, 1] + half * b[:, 3]
    area = (x1 - x0) * (y1 - y0)
    iw = np.maximum(np.minimum(one, x1) - np.maximum(zero, x0), zero)
    ih = np.maximum(np.minimum(one, y1) - np.maximum(zero, y0), zero)
    inter = iw * ih
    union = (one + area) - inter
    iou = inter / union
    ew = np.maximum(np.maximum(one, x1) - np.minimum(zero, x0), zero)
    eh = np.maximum(np.maximum(one, y1) - np.minimum(zero, y0), zero)
    enc = ew * eh
    giou = iou - (enc - union) / enc
    for v in (area, inter, union, iou, enc, giou):
        assert v.dtype == F32
    return iou, giou


def select(cls, boxes):
    """The selection for one image: cls float32 [np, 512], boxes float32 [np, 4].  Returns a dict: ``values`` (the IoU or GIoU
    vector used), ``used_giou``, ``thr`` (float32), ``selected`` (bool [np]), ``n_selected``, ``status``, ``mean_sim`` (float64
    [np], of every row), ``best`` (-1 when nothing is selected), ``gap`` (float64: the distance from the smallest ``mean_sim``
    among the selected rows to the next DIFFERENT value among them; inf when there is none) and ``scale`` (the largest
    |mean_sim| among the selected rows)."""
    cls = np.ascontiguousarray(cls, dtype=F32)
    iou, giou = iou_unit(boxes)
    used_giou = bool(np.all(iou == 0))
    values = giou if used_giou else iou
    thr = F32(values.max() * F32(0.8))
    selected = values >= thr
    n = int(selected.sum())
    c64 = cls.astype(np.float64)
    mean_sim = (c64 * c64.mean(0)[None, :]).sum(axis=1)           # row by row: identical rows give identical values (a BLAS product need not)
    out = dict(iou=iou, giou=giou, values=values, used_giou=used_giou, thr=thr, selected=selected, n_selected=n, mean_sim=mean_sim,
               best=-1, gap=float("inf"), scale=0.0, status=STATUS_EMPTY)
    if n:
        idx = np.nonzero(selected)[0]
        ms = mean_sim[idx]
        out["best"] = int(idx[np.argmin(ms)])                    # first occurrence: the lowest row on a tie
        rest = ms[ms != ms.min()]
        out["gap"] = float(rest.min() - ms.min()) if rest.size else float("inf")
        out["scale"] = float(np.abs(ms).max())
        out["status"] = STATUS_GIOU if used_giou else STATUS_IOU
    return out


# --------------------------------------------------------------------------------------------------------- HF's statements
def hf_modules():
    from transformers.models.owlv2 import modeling_owlv2
    from transformers.models.owlvit import modeling_owlvit
    return {"owlvit": (modeling_owlvit, modeling_owlvit.OwlViTForObjectDetection),
            "owlv2": (modeling_owlv2, modeling_owlv2.Owlv2ForObjectDetection)}


def hf_statements(module, boxes):
    """(values float32 [np], used_giou, thr float32, selected bool [np]) by HF's own statements of ``embed_image_query`` up to
    the selection, with the module's ``center_to_corners_format`` / ``box_iou`` / ``generalized_box_iou``."""
    import torch
    corners = module.center_to_corners_format(torch.from_numpy(np.ascontiguousarray(boxes, dtype=F32)))
    query_box = torch.tensor([[0, 0, 1, 1]])
    ious, _ = module.box_iou(query_box, corners)
    used_giou = bool(torch.all(ious[0] == 0.0))
    if used_giou:
        ious = module.generalized_box_iou(query_box, corners)
    thr = torch.max(ious) * 0.8
    assert ious.dtype == torch.float32 and thr.dtype == torch.float32
    return ious[0].numpy(), used_giou, thr.numpy()[()], (ious[0] >= thr).numpy()


def hf_embed_image_query(model_class, cls, boxes):
    """HF's own ``embed_image_query`` on crafted tensors (one image): the method runs on a stub whose ``class_predictor`` /
    ``box_predictor`` return them.  Returns (query embedding float32 [512] or None, best index or -1)."""
    import torch
    t_cls = torch.from_numpy(np.ascontiguousarray(cls, dtype=F32))[None]
    t_box = torch.from_numpy(np.ascontiguousarray(boxes, dtype=F32))[None]
    stub = types.SimpleNamespace(class_predictor=lambda feats: (None, t_cls), box_predictor=lambda feats, fmap, interp=False: t_box)
    feats = torch.zeros((1, t_cls.shape[1], 1))
    with torch.no_grad():
        emb, idx, pred = model_class.embed_image_query(stub, feats, feats, False)
    assert pred is t_box
    if emb is None:
        return None, -1
    return emb[0, 0].numpy(), int(idx[0, 0])


# ------------------------------------------------------------------------------------------------------- crafted cases
CASE_NP = (1, 12, 63, 64, 65, 576, 3600)            # wave edges at 63 / 64 / 65; 3600 is the largest patch grid


def _small_boxes(rs, n):
    """Boxes of 5 .. 20 % of the image, well inside it: IoU with the unit box at most 0.04."""
    return np.concatenate([rs.uniform(0.2, 0.8, (n, 2)), rs.uniform(0.05, 0.2, (n, 2))], axis=1).astype(F32)


def _embeddings(rs, n):
    """Class embeddings with a common component: cls[i] = 4 u + 0.25 noise_i, |u| = 1.  mean_sim is then about 16 for every
    row, with a spread of about 1 (4 u . 0.25 noise_i)."""
    u = rs.standard_normal(PROJ)
    u /= np.linalg.norm(u)
    return (4.0 * u[None, :] + 0.25 * rs.standard_normal((n, PROJ))).astype(F32)


def plant_minimum(cls, row):
    """Make ``row`` the unique ``mean_sim`` minimum by a wide margin: half of the mean embedding is taken off it.  With the
    embeddings of ``_embeddings`` every other row stays near (1 - 0.5 / np) 16 while this one drops to about half of that."""
    cls[row] = (cls[row].astype(np.float64) - 0.5 * cls.astype(np.float64).mean(0)).astype(F32)


STRADDLE_TOP = (0.5, 0.5, 1.0, 0.998046875)       # IoU 1 - 2 / 1024 exactly; found by search: its threshold is hit exactly (below)


def _straddle(n):
    """Row 0 the box with the largest IoU, then full-width boxes centred at y = 0.47 whose heights step through consecutive
    float32 values around the threshold float32(IoU_max * 0.8): their IoUs land on the threshold itself and one ulp on either side
    of it (with a centred unit box as row 0 only odd distances occur: float32(0.8) is not reached)."""
    b = np.empty((n, 4), F32)
    b[0] = STRADDLE_TOP
    h = F32(iou_unit(b[:1])[0][0] * F32(0.8))
    for _ in range((n - 1) // 2):
        h = np.nextafter(h, F32(0))
    for i in range(1, n):
        b[i] = (0.5, 0.47, 1.0, h)
        h = np.nextafter(h, F32(2))
    return b


def make_case(kind, np_, rs, plant=None):
    """(cls float32 [np, 512], boxes float32 [np, 4], expected dict) of one image of a numbered case.  ``plant``: the row that
    gets the planted ``mean_sim`` minimum (among the rows the case selects; default: the middle one)."""
    cls = _embeddings(rs, np_)
    exp = {}
    if kind == 1:                                   # one unit box among small ones
        boxes = _small_boxes(rs, np_)
        r = np_ // 3 if plant is None else plant
        boxes[r] = (0.5, 0.5, 1.0, 1.0)
        exp = dict(status=STATUS_IOU, n_selected=1, best=r, thr=F32(0.8))
    elif kind == 2:                                 # identical maximal IoU 0.5 from (1, 1/2) and (1/2, 1); (1/2, 1/2), (1/4, x) below
        shapes = np.array([(1.0, 0.5), (0.5, 1.0), (0.5, 0.5), (0.25, 1.0), (1.0, 0.25), (0.25, 0.25)], F32)
        pick = np.arange(np_) % len(shapes)
        boxes = np.concatenate([np.full((np_, 2), 0.5, F32), shapes[pick]], axis=1)
        sel = np.nonzero(pick < 2)[0]
        r = int(sel[len(sel) // 2]) if plant is None else plant
        plant_minimum(cls, r)
        exp = dict(status=STATUS_IOU, n_selected=len(sel), best=r, thr=F32(0.4))
    elif kind == 3:                                 # straddling the threshold within one ulp
        boxes = _small_boxes(rs, np_)
        k = min(np_, 41)
        boxes[:k] = _straddle(k)
        iou, _ = iou_unit(boxes)
        thr = F32(F32(1.0 - 2.0 / 1024.0) * F32(0.8))
        lo, hi = np.nextafter(thr, F32(0)), np.nextafter(thr, F32(2))
        assert (iou == thr).any() and (iou == lo).any() and (iou == hi).any(), "the straddle must hit thr and both neighbours"
        sel = np.nonzero(iou >= thr)[0]
        r = int(sel[len(sel) // 2]) if plant is None else plant
        plant_minimum(cls, r)
        exp = dict(status=STATUS_IOU, n_selected=len(sel), best=r, thr=thr)
    elif kind in (4, 5, 6):                         # zero-area boxes: every IoU is 0, the GIoU fallback runs
        boxes = np.concatenate([rs.uniform(0.3, 0.7, (np_, 2)), rs.uniform(0.0, 0.5, (np_, 2))], axis=1).astype(F32)
        boxes[np.arange(np_) % 3 == 0, 2] = 0       # zero width, zero height, or both: inside the unit square, GIoU exactly 0
        boxes[np.arange(np_) % 3 != 0, 3] = 0
        outside = np.zeros(np_, bool)
        if kind == 5:                               # every second row: zero height reaching over the right edge, GIoU < 0
            outside[1::2] = True
        if kind == 6:
            outside[:] = True
        boxes[outside] = (0.9, 0.5, 0.5, 0.0)
        boxes[outside, 2] += rs.uniform(0, 0.5, int(outside.sum())).astype(F32)
        sel = np.nonzero(~outside)[0]
        if kind == 6:
            exp = dict(status=STATUS_EMPTY, n_selected=0, best=-1)
        else:
            r = int(sel[len(sel) // 2]) if plant is None else plant
            if len(sel) > 1:
                plant_minimum(cls, r)
            exp = dict(status=STATUS_GIOU, n_selected=len(sel), best=r, thr=F32(0))
    elif kind == 7:                                 # all boxes identical: every row selected, the planted row decides
        boxes = np.empty((np_, 4), F32)
        boxes[:] = (0.45, 0.55, 0.6, 0.7)
        r = np_ // 2 if plant is None else plant
        if np_ > 1:
            plant_minimum(cls, r)
        exp = dict(status=STATUS_IOU, n_selected=np_, best=r)
    elif kind == 8:                                 # two selected rows with identical embeddings: the lower index
        boxes = np.empty((np_, 4), F32)
        boxes[:] = (0.5, 0.5, 0.9, 0.9)
        r = np_ // 4 if plant is None else plant
        r2 = np_ - 1 if r != np_ - 1 else np_ - 2
        lo, hi = min(r, r2), max(r, r2)
        plant_minimum(cls, lo)
        cls[hi] = cls[lo]
        exp = dict(status=STATUS_IOU, n_selected=np_, best=lo, twin=hi)
    else:
        raise ValueError(kind)
    return cls, np.ascontiguousarray(boxes, dtype=F32), exp


def case_list(np_):
    """[(label, kind, plant)] of every numbered case that np rows can hold (a single row holds neither several boxes nor a tie)."""
    out = [("1 unit box", 1, None)]
    if np_ >= 2:
        out.append(("2 identical maxima", 2, None))
    if np_ >= 12:
        out.append(("3 threshold straddle", 3, None))
    out.append(("4 GIoU fallback", 4, None))
    if np_ >= 2:
        out.append(("5 GIoU negative rows", 5, None))
    out.append(("6 empty selection", 6, None))
    for r in sorted({0, 63, 64, np_ - 1}):
        if r < np_:
            out.append((f"7 identical boxes, minimum at {r}", 7, r))
    if np_ >= 2:
        out.append(("8 identical embeddings", 8, None))
    return out


def build_cases(np_, seed=0):
    """[(label, cls, boxes, expected)] of ``case_list(np_)`` from numpy's frozen legacy stream."""
    out = []
    for i, (label, kind, plant) in enumerate(case_list(np_)):
        rs = np.random.RandomState(1000 * np_ + 10 * i + seed)
        cls, boxes, exp = make_case(kind, np_, rs, plant)
        out.append((label, cls, boxes, exp))
    return out


EPS32 = float(np.finfo(np.float32).eps)


def mean_sim_bound(cls, selected):
    """The error bound on ``mean_sim`` by tests/owl_tail_util.bound's rule: 4 x the error of float32 torch (``torch.mean`` then
    the einsum of ``embed_image_query``) against float64 over the selected rows, plus one float32 ulp of the largest magnitude."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(cls, dtype=F32))
    ms32 = torch.einsum("d,id->i", torch.mean(t, axis=0), t).numpy().astype(np.float64)[selected]
    c64 = cls.astype(np.float64)
    ms64 = (c64 * c64.mean(0)[None, :]).sum(axis=1)[selected]
    if not ms64.size:
        return 0.0
    return 4.0 * float(np.abs(ms32 - ms64).max()) + EPS32 * float(np.abs(ms64).max())


# --------------------------------------------------------------------------------------- end to end: HF on the CPU as the witness
# (family, patch, input size): B/32 at 35 patches, B/16 and OWLv2 B/16 at 24
GEOMETRIES = {"b32": ("owlvit", 32, (160, 224)), "b16": ("owlvit", 16, (64, 96)), "v2": ("owlv2", 16, (64, 96))}
CKPT_SEED = {"b32": 0, "b16": 0, "v2": 0}


def example_images(seed, n, H, W):
    """uint8 [n, H, W, 3]: coloured blocks of 16 px with a little noise, from numpy's frozen legacy stream."""
    rs = np.random.RandomState(seed)
    blocks = rs.randint(0, 256, (n, -(-H // 16), -(-W // 16), 3))
    img = np.kron(blocks, np.ones((1, 16, 16, 1), dtype=np.int64))[:, :H, :W]
    return np.clip(img + rs.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)


def query_and_target_images():
    """(two example images 120 x 168, two target images 95 x 200)."""
    return example_images(41, 2, 120, 168), example_images(42, 2, 95, 200)


def make_checkpoint(geometry, dirpath):
    """HF's model at its own init with the heads shrunk (tests/owl_input_size_util.py / tests/owlv2_util.py), saved to ``dirpath``."""
    family, patch, _ = GEOMETRIES[geometry]
    if family == "owlv2":
        import owlv2_util
        return owlv2_util.make_checkpoint_dir(dirpath, seed=CKPT_SEED[geometry])
    import owl_input_size_util
    return owl_input_size_util.make_checkpoint_dir(dirpath, patch, seed=CKPT_SEED[geometry])


def hf_pixels(geometry, images):
    """float32 [n, 3, h, w]: HF's own image processor of the family at the geometry's input size."""
    family, _, size = GEOMETRIES[geometry]
    if family == "owlv2":
        import owlv2_util as P
    else:
        import owl_input_size_util as P
    return np.stack([P.hf_pixels(img, size) for img in images])


def hf_image_guided(geometry, model, query_images, target_images):
    """HF's ``image_guided_detection(pixel_values, query_pixel_values, interpolate_pos_encoding=True)`` (target image b against
    example image b) and ``embed_image_query`` on the CPU, with what the margin assertions need: per example image the IoU (GIoU)
    vector, threshold and selected set by HF's statements on HF's ``query_pred_boxes`` and float32 ``mean_sim`` by HF's
    statements on HF's class embeddings."""
    import torch
    family = GEOMETRIES[geometry][0]
    module, _ = hf_modules()[family]
    qpx, tpx = torch.from_numpy(hf_pixels(geometry, query_images)), torch.from_numpy(hf_pixels(geometry, target_images))
    with torch.no_grad():
        out = model.image_guided_detection(pixel_values=tpx, query_pixel_values=qpx, interpolate_pos_encoding=True)
        fmap = model.image_embedder(pixel_values=qpx, interpolate_pos_encoding=True)[0]
        feats = fmap.reshape(fmap.shape[0], -1, fmap.shape[-1])
        embeds, indices, qboxes = model.embed_image_query(feats, fmap, True)
        _, class_embeds = model.class_predictor(feats)
    assert embeds is not None and embeds.shape[0] == len(query_images), "HF produced no query for an example image"
    assert torch.equal(qboxes, out.query_pred_boxes)
    per_image = []
    for i in range(len(query_images)):
        values, used_giou, thr, selected = hf_statements(module, qboxes[i].numpy())
        ce = class_embeds[i]
        mean_sim = torch.einsum("d,id->i", torch.mean(ce, axis=0), ce[torch.from_numpy(selected)]).numpy()
        per_image.append(dict(values=values, used_giou=used_giou, thr=thr, selected=selected, mean_sim=mean_sim, best=int(indices[i, 0]),
                              boxes=qboxes[i].numpy(), class_embeds=ce.numpy()))
    q = embeds[:, 0]
    qn = (q / (torch.linalg.norm(q, dim=-1, keepdim=True) + 1e-6)).numpy()
    return dict(per_image=per_image, embeds=q.numpy(), qn=qn, probs=torch.sigmoid(out.logits[..., 0]).numpy(),
                target_boxes=out.target_pred_boxes.numpy())


def assert_hf_margins(ref):
    """HF's own margins, asserted before anything is compared: every patch's IoU at least 1e-3 (relative) away from the
    threshold, and where several rows are selected the two smallest ``mean_sim`` at least 1e-3 of the largest |mean_sim|
    apart.  Returns (smallest threshold margin, smallest gap ratio or inf)."""
    margin, gap = float("inf"), float("inf")
    for i, p in enumerate(ref["per_image"]):
        thr = float(p["thr"])
        assert thr > 0, (i, thr)
        m = float(np.abs(p["values"].astype(np.float64) - thr).min() / thr)
        assert m >= 1e-3, (i, m)
        margin = min(margin, m)
        ms = np.sort(p["mean_sim"].astype(np.float64))
        if ms.size > 1:
            g = float((ms[1] - ms[0]) / np.abs(ms).max())
            assert g >= 1e-3, (i, g)
            gap = min(gap, g)
    return margin, gap


def device_image_guided(h, geometry, ref):
    """The device's side of ``hf_image_guided`` through an ``OWLInterface`` of the geometry: the example images embedded in one
    call, each embedding installed in a slot of its own by hand, target b scored against example b.  Returns what the test
    asserts on: the selection's outcome, whether the query boxes are ``score(...).boxes_cxcywh[best]`` of the same image bit for
    bit, and the largest deviations from HF (normalised embedding, sigmoid(logit), target boxes in pixels)."""
    import torch
    family = GEOMETRIES[geometry][0]
    q_imgs, t_imgs = query_and_target_images()
    dq, dt = torch.from_numpy(q_imgs).cuda(), torch.from_numpy(t_imgs).cuda()
    r = h.scorer.embed_image_queries(dq)
    n = len(q_imgs)
    for b in range(n):
        h.scorer.set_query_embeds(r.embeds[b:b + 1], [1], [1.0], slot=1 + b)
    slots = [1 + b for b in range(n)]
    same = h.scorer.score(dq, 1, 1, want_logits=True, image_sets=slots)
    res = h.scorer.score(dt, 1, 1, want_logits=True, image_sets=slots)
    torch.cuda.synchronize()
    cx = same.boxes_cxcywh.cpu().numpy()
    box_bits = all(r.best[b] >= 0 and np.array_equal(r.boxes_cxcywh[b].view(np.uint32), cx[b, r.best[b]].view(np.uint32)) for b in range(n))
    e64 = r.embeds.astype(np.float64)
    qn = e64 / (np.linalg.norm(e64, axis=1, keepdims=True) + 1e-6)
    probs = torch.sigmoid(res.logits[..., 0]).cpu().numpy()
    H_, W_ = t_imgs.shape[1:3]
    sx, sy = (max(H_, W_), max(H_, W_)) if family == "owlv2" else (W_, H_)          # OWLv2 boxes are relative to the padded square
    tb, half = ref["target_boxes"].astype(F32), F32(0.5)
    want = np.stack([(tb[..., 0] - half * tb[..., 2]) * F32(sx), (tb[..., 1] - half * tb[..., 3]) * F32(sy),
                     (tb[..., 0] + half * tb[..., 2]) * F32(sx), (tb[..., 1] + half * tb[..., 3]) * F32(sy)], axis=-1)
    return dict(result=r, query_boxes_are_the_scorers_bits=box_bits, emb_err=float(np.abs(qn - ref["qn"]).max()),
                prob_err=float(np.abs(probs - ref["probs"]).max()), box_err=float(np.abs(res.boxes.cpu().numpy() - want).max()))


def reference_for(geometry, model, wkey, cache):
    """``hf_image_guided`` of the geometry, once per weights (``wkey`` "f32", or "bf16": HF on ``round_weights_to_bf16`` weights)."""
    if (geometry, wkey) not in cache:
        import copy
        import torch
        from tstar_amd import weights as W
        if wkey == "bf16":
            sd = W.round_weights_to_bf16({k: v.numpy() for k, v in model.state_dict().items()})
            model = copy.deepcopy(model)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        q, t = query_and_target_images()
        cache[(geometry, wkey)] = hf_image_guided(geometry, model, q, t)
    return cache[(geometry, wkey)]


E2E_CASES = [(g, m) for g in GEOMETRIES for m in ("f32", "f32x3")] + [("b16", "bf16")]
