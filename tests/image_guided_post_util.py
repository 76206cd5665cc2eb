"""Helpers of tests/test_image_guided_post_host.py and tests/test_gpu_image_guided_post.py: a numpy restatement of HF's
``post_process_image_guided_detection`` (float32, statement by statement), HF's own method as the witness, the crafted
(logits, boxes) cases of the post-process kernel, the general-box form of the query selection of tests/image_query_util.py, and
the end-to-end one-shot references (HF on the CPU).

Every case has distinct non-zero scores where it has scores at all: torch's ``argsort`` leaves the order of equal scores open, so
only then is HF alone unambiguous.  ``assert_unambiguous`` checks it."""
import types

import numpy as np

import image_query_util as U

F32 = np.float32
NP_LIST = (1, 2, 63, 64, 65, 255, 256, 257, 576, 3600)
SIZES3 = ((285, 600), (1520, 3200), (333, 111))         # (height, width) of up to three images


# ------------------------------------------------------------------------------------------- the post-process, restated
def corners(boxes):
    b = np.ascontiguousarray(boxes, dtype=F32)
    half = F32(0.5)
    return np.stack([b[:, 0] - half * b[:, 2], b[:, 1] - half * b[:, 3], b[:, 0] + half * b[:, 2], b[:, 1] + half * b[:, 3]], axis=1)


def iou_row(c, i):
    """HF's ``box_iou(c[i:i + 1], c)[0][0]``: float32 [np]."""
    area = (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
    wh = np.maximum(np.minimum(c[i, 2:], c[:, 2:]) - np.maximum(c[i, :2], c[:, :2]), F32(0))
    inter = wh[:, 0] * wh[:, 1]
    union = area[i] + area - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / union
    assert iou.dtype == F32
    return iou


def post_process(scores, boxes, threshold, nms_threshold, scale_xy=None, deciding=None):
    """One image: scores float32 [np], boxes cxcywh float32 [np, 4] -> dict(alphas, boxes, keep, n_kept, dropped).  ``deciding``:
    a list that receives every IoU a live candidate compared with the threshold against a box that was still live."""
    s = np.array(scores, dtype=F32)
    n = s.size
    c = corners(boxes)
    if nms_threshold < 1.0:
        for i in np.lexsort((np.arange(n), -s)):                 # score descending, lowest index first
            if not s[i]:
                continue
            iou = iou_row(c, i)
            iou[i] = F32(-1)
            if deciding is not None:
                live = s != 0
                live[i] = False
                deciding.extend(iou[live].tolist())
            s[iou > F32(nms_threshold)] = 0
    sx, sy = (F32(1), F32(1)) if scale_xy is None else (F32(scale_xy[0]), F32(scale_xy[1]))
    scaled = c * np.array([sx, sy, sx, sy], dtype=F32)
    alphas = np.zeros(n, F32)
    dropped = not s.any()
    if not dropped:
        s[s < F32(threshold)] = 0
        m = s.max() + F32(1e-6)
        alphas = np.clip((s - m * F32(0.1)) / (m * F32(0.9)), F32(0), F32(1))
    assert scaled.dtype == F32 and alphas.dtype == F32
    keep = alphas > 0
    return dict(alphas=alphas, boxes=scaled, keep=keep, n_kept=int(keep.sum()), dropped=dropped, nms_scores=s)


def scale_of(target_sizes, family="owlvit"):
    """float32 [B, 2] (sx, sy) of (height, width) sizes as the family's HF processor scales boxes; None stays None."""
    if target_sizes is None:
        return None
    return np.array([(max(h, w), max(h, w)) if family == "owlv2" else (w, h) for h, w in target_sizes], dtype=F32)


# ------------------------------------------------------------------------------------------------------- HF's own method
def scores_of(logits):
    """What HF's post-process starts from: sigmoid(max logit over the queries), by torch."""
    import torch
    return torch.sigmoid(torch.max(torch.from_numpy(np.ascontiguousarray(logits, dtype=F32)), dim=-1).values).numpy()


def hf_processor_class(family="owlvit"):
    if family == "owlv2":
        from transformers.models.owlv2.image_processing_pil_owlv2 import Owlv2ImageProcessorPil
        return Owlv2ImageProcessorPil
    from transformers.models.owlvit.image_processing_pil_owlvit import OwlViTImageProcessorPil
    return OwlViTImageProcessorPil


def hf_post_process(logits, boxes, threshold, nms_threshold, target_sizes, family="owlvit"):
    """HF's ``post_process_image_guided_detection`` on logits float32 [B, np, Q] / target_pred_boxes float32 [B, np, 4]: a list of
    B (scores float32 [k], boxes float32 [k, 4]).  HF leaves an image without a non-zero score out of its list; NMS never zeroes
    the best live candidate, so these are exactly the images whose scores are all 0: an empty entry is put back for each."""
    import torch
    out = types.SimpleNamespace(logits=torch.from_numpy(np.array(logits, dtype=F32)), target_pred_boxes=torch.from_numpy(np.array(boxes, dtype=F32)))
    ts = None if target_sizes is None else torch.tensor([list(t) for t in target_sizes])
    res = hf_processor_class(family).post_process_image_guided_detection(None, out, threshold=threshold, nms_threshold=nms_threshold,
                                                                         target_sizes=ts)
    dropped = [not sc.any() for sc in scores_of(logits)]
    assert len(res) == len(dropped) - sum(dropped)
    it = iter(res)
    full = []
    for d in dropped:
        if d:
            full.append((np.zeros(0, F32), np.zeros((0, 4), F32)))
        else:
            r = next(it)
            assert r["labels"] is None and r["scores"].dtype == torch.float32 and r["boxes"].dtype == torch.float32
            full.append((r["scores"].numpy(), r["boxes"].numpy()))
    return full


# ---------------------------------------------------------------------------------------------------------- crafted cases
NMS = F32(0.3)
_BUILT = {}


def _logits(rs, n, top=0):
    """Distinct logits: a permutation of n evenly spaced values in [-4, 4]; the first ``top`` rows get 5.0, 4.9, ... instead."""
    v = np.linspace(-4.0, 4.0, n) if n > 1 else np.array([0.7])
    v = rs.permutation(v)
    v[:top] = 5.0 - 0.1 * np.arange(top)
    return v.astype(F32)


def _away(rs, n):
    """Small boxes in the lower part of the image (y above 0.62), clear of what the chain / straddle kinds plant above it."""
    return np.concatenate([rs.uniform(0.1, 0.9, (n, 1)), rs.uniform(0.7, 0.9, (n, 1)), rs.uniform(0.02, 0.15, (n, 2))], axis=1).astype(F32)


def _straddle_pairs():
    if "straddle" not in _BUILT:
        _BUILT["straddle"] = _find_straddle_pairs()
    return _BUILT["straddle"]


def _find_straddle_pairs():
    """Three nested pairs (same centre and width, heights H and h) whose IoU is float32(0.3) exactly, one ulp below and one ulp
    above: found by a search over consecutive float32 heights, in the restatement's arithmetic."""
    thr = NMS
    targets = (thr, np.nextafter(thr, F32(0)), np.nextafter(thr, F32(1)))
    out = []
    for cx, want in zip((0.15, 0.5, 0.85), targets):
        found = None
        H = F32(0.5)
        for _ in range(64):                                       # the larger height, a float32 at a time
            big = np.array([cx, 0.3, 0.2, H], F32)
            h = F32(F32(0.5) * thr)
            for _ in range(256):
                h = np.nextafter(h, F32(0))
            smalls = np.empty((512, 4), F32)
            for k in range(512):                                  # the smaller height, 256 float32 values to either side
                smalls[k] = (cx, 0.3, 0.2, h)
                h = np.nextafter(h, F32(1))
            hit = np.nonzero(iou_row(corners(np.concatenate([big[None], smalls])), 0)[1:] == want)[0]
            if hit.size:
                found = smalls[hit[0]].copy()
                break
            H = np.nextafter(H, F32(0))
        assert found is not None, "no pair of heights gives the wanted IoU"
        out.append((big, found))
    return out


def make_image(kind, n, rs):
    """(logits float32 [n], boxes float32 [n, 4], expected {row: kept?}) of one image."""
    exp = {}
    if kind == "random":
        logits = _logits(rs, n)
        boxes = np.concatenate([rs.uniform(0.1, 0.9, (n, 2)), rs.uniform(0.02, 0.3, (n, 2))], axis=1).astype(F32)
    elif kind == "disjoint":                        # a grid of boxes that do not touch: every candidate stays live
        logits = _logits(rs, n)
        g = int(np.ceil(np.sqrt(n)))
        k = np.arange(n)
        boxes = np.stack([(k % g + 0.5) / g, (k // g + 0.5) / g, np.full(n, 0.5 / g), np.full(n, 0.5 / g)], axis=1).astype(F32)
    elif kind == "clusters":                        # near-duplicates around a few centres
        logits = _logits(rs, n)
        nc = max(1, n // 8)
        centres = np.concatenate([rs.uniform(0.2, 0.8, (nc, 2)), rs.uniform(0.1, 0.3, (nc, 2))], axis=1)
        boxes = (centres[rs.randint(0, nc, n)] + 1e-3 * rs.standard_normal((n, 4))).astype(F32)
    elif kind == "chain":                           # A suppresses B, so B must not suppress C (needs n >= 3)
        logits = _logits(rs, n, top=3)
        boxes = _away(rs, n)
        boxes[0], boxes[1], boxes[2] = (0.3, 0.25, 0.4, 0.3), (0.45, 0.25, 0.4, 0.3), (0.6, 0.25, 0.4, 0.3)
        exp = {0: True, 1: False, 2: True}
    elif kind == "straddle":                        # IoU == nms_threshold, one ulp below, one ulp above (needs n >= 6)
        logits = _logits(rs, n, top=6)
        boxes = _away(rs, n)
        for k, (big, small) in enumerate(_straddle_pairs()):
            boxes[k], boxes[3 + k] = big, small
        exp = {0: True, 1: True, 2: True, 3: True, 4: True, 5: False}
    elif kind == "degenerate":                      # zero-area boxes (identical ones: 0 / 0), inverted boxes, ordinary ones
        logits = _logits(rs, n)
        boxes = np.concatenate([rs.uniform(0.2, 0.8, (n, 2)), rs.uniform(0.05, 0.4, (n, 2))], axis=1).astype(F32)
        k = np.arange(n)
        boxes[k % 5 == 0, 2] = 0
        boxes[k % 5 == 1, 3] = 0
        boxes[k % 5 == 2] = (0.5, 0.5, 0.0, 0.0)
        boxes[k % 5 == 3, 2] *= -1
    elif kind == "allzero":                         # sigmoid(-200) is 0 in float32: HF drops the image
        logits = np.full(n, -200.0, F32)
        boxes = np.concatenate([rs.uniform(0.1, 0.9, (n, 2)), rs.uniform(0.02, 0.3, (n, 2))], axis=1).astype(F32)
    else:
        raise ValueError(kind)
    return logits, np.ascontiguousarray(boxes, dtype=F32), exp


def _case_specs():
    """[(np, kinds of the B images, threshold, nms_threshold, target sizes or None)]"""
    specs = []
    for n in NP_LIST:
        specs.append((n, ("random",), 0.0, 0.3, None))
        specs.append((n, ("clusters", "random", "allzero"), 0.0, 0.3, SIZES3))
        specs.append((n, ("degenerate",), 0.0, 0.3, SIZES3[:1]))
        if n >= 6:
            specs.append((n, ("chain", "degenerate", "straddle"), 0.0, 0.3, None))
            specs.append((n, ("straddle",), 0.0, 0.3, SIZES3[1:2]))
            specs.append((n, ("chain",), 0.0, 0.3, None))
    for n in (65, 576):
        for nms in (0.0, 1.0):
            specs.append((n, ("clusters", "degenerate", "random"), 0.0, nms, SIZES3 if nms else None))
            specs.append((n, ("random",), 0.0, nms, None if nms else SIZES3[:1]))
        specs.append((n, ("random",), 2.0, 0.3, None))                     # a threshold above every score
        specs.append((n, ("clusters", "random", "chain"), 0.5, 0.3, SIZES3))
        specs.append((n, ("allzero",), 0.0, 0.3, None))
    specs.append((257, ("disjoint",), 0.0, 0.3, None))
    specs.append((3600, ("disjoint",), 0.0, 0.3, SIZES3[:1]))
    specs.append((3600, ("clusters", "degenerate", "chain"), 0.2, 0.3, SIZES3))
    return specs


def build_cases():
    """[dict(label, np, B, logits [B, np, 2], boxes [B, np, 4], threshold, nms, sizes, expected [per image {row: kept?}])] from
    numpy's frozen legacy stream; built once."""
    if "cases" not in _BUILT:
        cases = []
        for ci, (n, kinds, thr, nms, sizes) in enumerate(_case_specs()):
            imgs = [make_image(kind, n, np.random.RandomState(7000 + 10 * ci + b)) for b, kind in enumerate(kinds)]
            top = np.stack([im[0] for im in imgs])
            logits = np.stack([top - F32(1.0), top], axis=-1)           # two queries: the max is the second column
            cases.append(dict(label=f"np={n} {'+'.join(kinds)} thr={thr} nms={nms} sizes={'yes' if sizes else 'none'}", np=n, B=len(kinds),
                              logits=np.ascontiguousarray(logits, dtype=F32), boxes=np.stack([im[1] for im in imgs]), threshold=thr, nms=nms,
                              sizes=sizes, expected=[im[2] for im in imgs], kinds=kinds))
        _BUILT["cases"] = cases
    return _BUILT["cases"]


def assert_unambiguous(case):
    """Distinct non-zero scores in every image that has scores at all: then HF's order, and so its result, is determined."""
    for b, s in enumerate(scores_of(case["logits"])):
        if case["kinds"][b] == "allzero":
            assert not s.any(), (case["label"], b)
        else:
            assert s.all() and np.unique(s).size == s.size, (case["label"], b)


def restated(case):
    """``post_process`` of every image of a case (cached), with the case's planted expectations asserted."""
    if "restated" not in case:
        scores, scale = scores_of(case["logits"]), scale_of(case["sizes"])
        out = []
        for b in range(case["B"]):
            r = post_process(scores[b], case["boxes"][b], case["threshold"], case["nms"], None if scale is None else scale[b])
            if case["nms"] == 0.3 and case["threshold"] == 0.0:
                for row, kept in case["expected"][b].items():
                    assert bool(r["keep"][row]) == kept, (case["label"], b, row)
            out.append(r)
        case["restated"] = out
    return case["restated"]


def host_entry(scores, boxes, threshold, nms, scale):
    """``tstar_image_guided_postprocess_host`` -> (alphas [B, np], boxes [B, np, 4], keep u8 [B, np], n_kept [B])."""
    from tstar_amd import _lib
    lib = _lib.load()
    scores, boxes = np.ascontiguousarray(scores, dtype=F32), np.ascontiguousarray(boxes, dtype=F32)
    B, n = scores.shape
    alphas, xyxy = np.full((B, n), F32(-77.25)), np.full((B, n, 4), F32(-77.25))
    keep, n_kept = np.full((B, n), 9, np.uint8), np.full(B, -12345, np.int32)
    rc = lib.tstar_image_guided_postprocess_host(scores.ctypes.data, boxes.ctypes.data, B, n, float(threshold), float(nms),
                                                 None if scale is None else np.ascontiguousarray(scale, dtype=F32).ctypes.data,
                                                 alphas.ctypes.data, xyxy.ctypes.data, keep.ctypes.data, n_kept.ctypes.data)
    _lib.check(rc, "tstar_image_guided_postprocess_host")
    return alphas, xyxy, keep, n_kept


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, dtype=F32).view(np.uint32), np.ascontiguousarray(b, dtype=F32).view(np.uint32))


# --------------------------------------------------------------------------- the query selection against a general query box
UNIT = np.array([0, 0, 1, 1], F32)


def iou_box(boxes, qbox):
    """(iou, giou) float32 [np] of cxcywh boxes against the query box (x0, y0, x1, y1): ``image_query_util.iou_unit`` with HF's
    ``box_iou`` / ``generalized_box_iou`` in their general form."""
    c = corners(boxes)
    q = np.ascontiguousarray(qbox, dtype=F32)
    x0, y0, x1, y1 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    zero = F32(0)
    area_q = (q[2] - q[0]) * (q[3] - q[1])
    area = (x1 - x0) * (y1 - y0)
    iw = np.maximum(np.minimum(q[2], x1) - np.maximum(q[0], x0), zero)
    ih = np.maximum(np.minimum(q[3], y1) - np.maximum(q[1], y0), zero)
    inter = iw * ih
    union = (area_q + area) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / union
        ew = np.maximum(np.maximum(q[2], x1) - np.minimum(q[0], x0), zero)
        eh = np.maximum(np.maximum(q[3], y1) - np.minimum(q[1], y0), zero)
        enc = ew * eh
        giou = iou - (enc - union) / enc
    for v in (area_q, area, inter, union, iou, enc, giou):
        assert v.dtype == F32
    return iou, giou


def select_box(cls, boxes, qbox):
    """``image_query_util.select`` against a general query box (the same fields)."""
    cls = np.ascontiguousarray(cls, dtype=F32)
    iou, giou = iou_box(boxes, qbox)
    used_giou = bool(np.all(iou == 0))
    values = giou if used_giou else iou
    thr = F32(values.max() * F32(0.8))
    selected = values >= thr
    n = int(selected.sum())
    c64 = cls.astype(np.float64)
    mean_sim = (c64 * c64.mean(0)[None, :]).sum(axis=1)
    out = dict(iou=iou, giou=giou, values=values, used_giou=used_giou, thr=thr, selected=selected, n_selected=n, mean_sim=mean_sim,
               best=-1, gap=float("inf"), scale=0.0, status=U.STATUS_EMPTY)
    if n:
        idx = np.nonzero(selected)[0]
        ms = mean_sim[idx]
        out["best"] = int(idx[np.argmin(ms)])
        rest = ms[ms != ms.min()]
        out["gap"] = float(rest.min() - ms.min()) if rest.size else float("inf")
        out["scale"] = float(np.abs(ms).max())
        out["status"] = U.STATUS_GIOU if used_giou else U.STATUS_IOU
    return out


def hf_statements_box(module, boxes, qbox):
    """``image_query_util.hf_statements`` with HF's ``box_iou`` / ``generalized_box_iou`` given another query box."""
    import torch
    c = module.center_to_corners_format(torch.from_numpy(np.ascontiguousarray(boxes, dtype=F32)))
    q = torch.from_numpy(np.ascontiguousarray(qbox, dtype=F32))[None]
    ious, _ = module.box_iou(q, c)
    used_giou = bool(torch.all(ious[0] == 0.0))
    if used_giou:
        ious = module.generalized_box_iou(q, c)
    thr = torch.max(ious) * 0.8
    return ious[0].numpy(), used_giou, thr.numpy()[()], (ious[0] >= thr).numpy()


HALF = np.array([0, 0, 0.5, 0.5], F32)                      # every crafted case of image_query_util scaled by 1/2: the same bits
OFF = np.array([0.55, 0.1, 0.8, 0.4], F32)                  # a small off-centre box
BOX_NP = (1, 63, 64, 65, 576, 3600)


def box_cases(np_):
    """[(label, cls, boxes, qbox, restatement's result)]: the crafted cases of ``image_query_util`` against the unit box and,
    scaled by 1/2 (a power of two: every IoU keeps its bits, so the exact-threshold straddle moves with them), against
    [0, 0, 0.5, 0.5]; and against a small off-centre box: a planted match, the GIoU fallback (zero-area predictions inside the
    box, none overlapping it) and a negative largest GIoU (status 2)."""
    key = ("box", np_)
    if key in _BUILT:
        return _BUILT[key]
    out = []
    for label, cls, boxes, exp in U.build_cases(np_):
        ru = U.select(cls, boxes)
        for q, bx, tag in ((UNIT, boxes, "unit"), (HALF, (boxes * F32(0.5)).astype(F32), "half")):
            r = select_box(cls, bx, q)
            assert (r["status"], r["n_selected"], r["best"]) == (ru["status"], ru["n_selected"], ru["best"]), (np_, label, tag)
            assert same_bits(r["values"], ru["values"]) and r["thr"] == ru["thr"], (np_, label, tag)
            out.append((f"{label} / {tag}", cls, bx, q, r))
    rs = np.random.RandomState(4242 + np_)
    # a planted match: row r is the query box itself, row r2 a slightly smaller one (both selected when np >= 2)
    cls, boxes = U._embeddings(rs, np_), U._small_boxes(rs, np_)
    boxes[:, :2] = rs.uniform(0.1, 0.4, (np_, 2)).astype(F32) * np.array([1, 2], F32) + np.array([0, 0.2], F32)        # mostly clear of OFF
    qc = np.array([(OFF[0] + OFF[2]) / 2, (OFF[1] + OFF[3]) / 2, OFF[2] - OFF[0], OFF[3] - OFF[1]], F32)
    r0 = np_ // 3
    boxes[r0] = qc
    if np_ >= 2:
        r2 = (r0 + 1) % np_
        boxes[r2] = qc * np.array([1, 1, 0.95, 0.97], F32)
        U.plant_minimum(cls, r2)
    r = select_box(cls, boxes, OFF)
    assert r["status"] == U.STATUS_IOU and r["n_selected"] == min(np_, 2) and r["best"] == (r2 if np_ >= 2 else r0), (np_, r["n_selected"])
    out.append(("off-centre match", cls, boxes, OFF, r))
    # the GIoU fallback: zero-width boxes, every third inside the query box (GIoU exactly 0), the others outside (negative)
    cls = U._embeddings(rs, np_)
    boxes = np.concatenate([rs.uniform(0.05, 0.45, (np_, 2)), np.zeros((np_, 1)), rs.uniform(0.0, 0.1, (np_, 1))], axis=1).astype(F32)
    inside = np.arange(np_) % 3 == 0
    boxes[inside, 0] = rs.uniform(0.6, 0.75, int(inside.sum())).astype(F32)
    boxes[inside, 1] = rs.uniform(0.2, 0.3, int(inside.sum())).astype(F32)
    sel = np.nonzero(inside)[0]
    if len(sel) > 1:
        U.plant_minimum(cls, int(sel[len(sel) // 2]))
    r = select_box(cls, boxes, OFF)
    assert r["status"] == U.STATUS_GIOU and r["n_selected"] == len(sel) and r["best"] == int(sel[len(sel) // 2]) and r["thr"] == 0, (np_, r["n_selected"])
    out.append(("off-centre GIoU fallback", cls, boxes, OFF, r))
    # nothing overlaps and every prediction has an area: the largest GIoU is negative, nothing is selected
    cls = U._embeddings(rs, np_)
    boxes = np.concatenate([rs.uniform(0.1, 0.4, (np_, 1)), rs.uniform(0.5, 0.9, (np_, 1)), rs.uniform(0.05, 0.15, (np_, 2))], axis=1).astype(F32)
    r = select_box(cls, boxes, OFF)
    assert r["status"] == U.STATUS_EMPTY and r["used_giou"] and r["values"].max() < 0, np_
    out.append(("off-centre negative GIoU", cls, boxes, OFF, r))
    for label, cls, boxes, q, r in out:
        if r["n_selected"] > 1:                    # the planted gap: 64 x the error bound on mean_sim, as the unit-box tests require
            assert r["gap"] >= 64 * U.mean_sim_bound(cls, r["selected"]), (np_, label)
    _BUILT[key] = out
    return out


# ------------------------------------------------------------------------------------------- end to end: HF as the witness
SCORE_BOUND, BOX_BOUND = 1e-3, 1e-2             # the project's bounds on sigmoid(logit) and on boxes in pixels
E2E_QBOX_PX = (100, 60, 168, 120)               # a region of the 120 x 168 example, (x0, y0, x1, y1) in pixels
# (family, patch, input size): few patches, so that HF's scores can lie more than twice the score bound apart from each other --
# with the 35 patches of image_query_util's B/32 geometry no image does (the chance is about exp(-n^2 gap / spread)).  OWLv2: the
# smallest square the device shrinks a 3200-pixel image to (at 32 x 32 the filter window of one output pixel does not fit in LDS)
E2E_GEOMETRIES = {"b32": ("owlvit", 32, (96, 128)), "v2": ("owlv2", 16, (64, 64))}


def e2e_checkpoint(geometry, dirpath):
    return U.make_checkpoint("v2" if geometry == "v2" else "b32", dirpath)


def e2e_pixels(geometry, images):
    family, _, size = E2E_GEOMETRIES[geometry]
    if family == "owlv2":
        import owlv2_util as P
    else:
        import owl_input_size_util as P
    return np.stack([P.hf_pixels(img, size) for img in images])


def grid_image(seed=5, cell=(380, 800)):
    """uint8: a 4 x 4 grid of frames of ``cell`` pixels (what a searcher's image grid looks like); 1520 x 3200 by default."""
    ch, cw = cell
    cells = U.example_images(seed, 16, ch, cw)
    return np.ascontiguousarray(cells.reshape(4, 4, ch, cw, 3).transpose(0, 2, 1, 3, 4).reshape(4 * ch, 4 * cw, 3))


def e2e_images(seed=0):
    """(example image 120 x 168, [target 285 x 600, 1520 x 3200 grid image])"""
    return U.example_images(41 + 100 * seed, 1, 120, 168)[0], [U.example_images(43 + 100 * seed, 1, 285, 600)[0], grid_image(5 + 100 * seed)]


def relative_box(px, H, W):
    return np.array([F32(px[0]) / F32(W), F32(px[1]) / F32(H), F32(px[2]) / F32(W), F32(px[3]) / F32(H)], F32)


def hf_one_shot(geometry, model, example, targets, qbox_px=None, threshold=0.0, nms_threshold=0.3):
    """HF's one-shot pipeline on the CPU: ``image_guided_detection`` (every target against the one example) and
    ``post_process_image_guided_detection`` with the targets' own sizes.  With ``qbox_px`` the query is chosen by ``select_box``
    on HF's own class embeddings / boxes of the example and goes through HF's ``class_predictor`` / ``box_predictor``.  Returns
    dict(probs [B, np], boxes cxcywh [B, np, 4], hf [(scores, boxes)] per image, sizes)."""
    import torch
    family = E2E_GEOMETRIES[geometry][0]
    sizes = [t.shape[:2] for t in targets]
    tpx = torch.from_numpy(e2e_pixels(geometry, targets))
    qpx = torch.from_numpy(e2e_pixels(geometry, [example] * len(targets)))
    with torch.no_grad():
        if qbox_px is None:
            out = model.image_guided_detection(pixel_values=tpx, query_pixel_values=qpx, interpolate_pos_encoding=True)
            logits, tboxes = out.logits, out.target_pred_boxes
        else:
            qmap = model.image_embedder(pixel_values=qpx[:1], interpolate_pos_encoding=True)[0]
            qfeats = qmap.reshape(1, -1, qmap.shape[-1])
            _, qcls = model.class_predictor(qfeats)
            qboxes = model.box_predictor(qfeats, qmap, True)
            sel = select_box(qcls[0].numpy(), qboxes[0].numpy(), relative_box(qbox_px, *example.shape[:2]))
            whole = select_box(qcls[0].numpy(), qboxes[0].numpy(), UNIT)
            assert sel["best"] != whole["best"], "the query box selects the whole image's patch: the case would show nothing"
            assert sel["status"] == U.STATUS_IOU and float(np.abs(sel["values"].astype(np.float64) - float(sel["thr"])).min()) >= 1e-3 * float(sel["thr"])
            ms = np.sort(sel["mean_sim"][sel["selected"]])
            assert ms.size == 1 or (ms[1] - ms[0]) >= 1e-3 * np.abs(ms).max(), "the example's two best rows are too close to call"
            query = qcls[0, sel["best"]][None, None, :].expand(len(targets), 1, -1)
            fmap = model.image_embedder(pixel_values=tpx, interpolate_pos_encoding=True)[0]
            feats = fmap.reshape(fmap.shape[0], -1, fmap.shape[-1])
            logits, _ = model.class_predictor(image_feats=feats, query_embeds=query)
            tboxes = model.box_predictor(feats, fmap, True)
    logits, tboxes = logits.numpy(), tboxes.numpy()
    hf = hf_post_process(logits, tboxes, threshold, nms_threshold, sizes, family)
    return dict(probs=scores_of(logits), boxes=tboxes, hf=hf, sizes=sizes, family=family, geometry=geometry, threshold=threshold, nms=nms_threshold)


def padding_patches(geometry, H, W):
    """bool [np]: the patches that see nothing but padding.  OWLv2's processor pads an H x W image to a max(H, W) square (grey, at
    the bottom / right) before resizing; OWL-ViT's does not pad."""
    family, patch, (ih, iw) = E2E_GEOMETRIES[geometry]
    gh, gw = ih // patch, iw // patch
    if family != "owlv2":
        return np.zeros(gh * gw, bool)
    S = max(H, W)
    rows, cols = np.arange(gh) * S >= H * gh, np.arange(gw) * S >= W * gw        # a row starting at or below the image's last line
    return (rows[:, None] | cols[None, :]).reshape(-1)


def assert_one_shot_preconditions(ref):
    """On HF's side, before anything of the device is compared: the restatement reproduces HF's result bit for bit (so its keep
    mask is HF's); every IoU that decided a suppression is at least 1e-3 away from the NMS threshold; neighbouring scores in the
    order differ by more than twice the score bound; HF itself suppresses something and keeps fewer patches than there are (a
    configuration in which NMS does nothing would show nothing).

    One kind of pair cannot meet the score condition.  OWLv2's processor pads the wide targets to a square, so the lower half of
    the patch grid sees the same grey pixels; such patches differ by their position embeddings alone and their scores lie 1e-5 to
    1e-4 apart at every seed and every input size that holds two of them (measured: the closest pair of all 40 seeds tried at
    64 x 64 was a padding pair).  For pairs of two padding patches the condition is therefore replaced by what it stands for:
    the kept set must not depend on their order -- HF's post-process on HF's boxes gives the same kept patches under 64 seeded
    perturbations of ALL scores by up to the score bound.  Every other neighbouring pair must meet the condition as stated.
    Returns (kept patches per image, smallest IoU margin, smallest gap outside padding pairs)."""
    scale = scale_of(ref["sizes"], ref["family"])
    kept, margin, gap = [], float("inf"), float("inf")
    ref["n_suppressed"], ref["padding_pairs"] = 0, 0
    for b in range(len(ref["sizes"])):
        deciding = []
        r = post_process(ref["probs"][b], ref["boxes"][b], ref["threshold"], ref["nms"], scale[b], deciding)
        assert same_bits(r["alphas"][r["keep"]], ref["hf"][b][0]) and same_bits(r["boxes"][r["keep"]], ref["hf"][b][1]), b
        ref["n_suppressed"] += int((r["nms_scores"] == 0).sum())
        if deciding:
            margin = min(margin, float(np.abs(np.asarray(deciding, dtype=np.float64) - ref["nms"]).min()))
        pad = padding_patches(ref["geometry"], *ref["sizes"][b])
        order = np.argsort(ref["probs"][b], kind="stable")
        d = np.diff(ref["probs"][b][order].astype(np.float64))
        both_pad = pad[order[:-1]] & pad[order[1:]]
        close = d <= 2 * SCORE_BOUND
        assert not (close & ~both_pad).any(), (b, float(d[~both_pad].min()))
        if (~both_pad).any():
            gap = min(gap, float(d[~both_pad].min()))
        if (close & both_pad).any():
            ref["padding_pairs"] += int((close & both_pad).sum())
            rs = np.random.RandomState(1234 + b)
            for _ in range(64):
                noisy = (ref["probs"][b].astype(np.float64) + rs.uniform(-SCORE_BOUND, SCORE_BOUND, pad.size)).astype(F32)
                rn = post_process(noisy, ref["boxes"][b], ref["threshold"], ref["nms"], scale[b])
                assert np.array_equal(rn["keep"], r["keep"]), (b, "the kept set depends on the order of two padding patches")
        kept.append(dict(patches=np.nonzero(r["keep"])[0], alphas=r["alphas"][r["keep"]], boxes=r["boxes"][r["keep"]],
                         m=float(ref["probs"][b].max()) + 1e-6))
    assert margin >= 1e-3, margin
    assert ref["n_suppressed"] > 0, "HF suppresses nothing in this configuration: the case shows nothing of the NMS"
    assert sum(len(k["patches"]) for k in kept) < sum(p.size for p in ref["probs"]), "HF keeps every patch"
    return kept, margin, gap


def alpha_bound(m):
    """|alpha - HF's| when every score is within SCORE_BOUND of HF's: alpha = (s - 0.1 m) / (0.9 m), so to first order
    (|ds| + 0.1 |dm|) / (0.9 m) with |ds|, |dm| <= SCORE_BOUND."""
    return (SCORE_BOUND + 0.1 * SCORE_BOUND) / (0.9 * m)
