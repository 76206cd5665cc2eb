"""The YOLO-World post-process (head_decode_kernel, sort_nms_kernel, det_cells_kernel of csrc/yolo.hip) on crafted head
outputs, path by path, through tstar_yolo_postprocess -- the tail of tstar_yolo_detect on caller-supplied tensors.

The text features are standard basis vectors, so a class logit is placed by one embedding entry; one-hot (or equal-weight)
DFL logits decode to exact integers.  Every selection check is teacher-forced: the GPU's own dense scores / boxes go
through the literal statement of mmyolo's predict_by_feat tail + the wrapper (tests/yolo_post_util.py, no shortcut) and
through oracle.yolo_ref.select, and scores, labels, boxes, n_kept, the padding and the cell outputs must be BIT-equal.
No near-tie allowance exists.  Each scenario also asserts, from the read-back data, that it reaches the path it is named for.
"""
import numpy as np
import pytest
import torch

import yolo_post_util as U

pytestmark = pytest.mark.gpu

SLOT_Q = {0: 4, 1: 32, 2: 1}                                        # query sets installed by the fixture
SLOT_W = {0: list(U.CELL_WEIGHTS), 1: [1.0 / (k + 3) for k in range(32)], 2: [0.3]}


@pytest.fixture(scope="module")
def env():
    from tstar_amd import yolo_world as Y
    from tstar_amd.yolo import YoloDetector
    sd = Y.synthetic_state_dict(2, "s")
    det = YoloDetector(sd, "s", max_batch=2)                         # batches of 3 run as 2 + 1: list bases and output offsets of a chunk
    for slot, q in SLOT_Q.items():
        det.set_text_feats(U.basis_text(q), SLOT_W[slot], slot=slot)
    yield dict(det=det, params=U.level_params(sd))
    det.close()


def upload(sc, params):
    e = [torch.from_numpy(x).cuda() for x in U.embeds_from_logits(sc["logits"], params)]
    d = [torch.from_numpy(x).cuda() for x in U.dfl_levels(sc["dfl"])]
    return e, d


def run(env, sc, dev, slots, thr=None, max_dets=None, grid=None, dense=True):
    B = sc["logits"].shape[0]
    rows, cols = grid or sc["grid"]
    r = env["det"].postprocess(dev[0], dev[1], B, sc["H"], sc["W"], rows, cols, score_threshold=sc["thr"] if thr is None else thr,
                               max_dets=max_dets or sc["max_dets"], image_sets=slots, want_dense=dense)
    torch.cuda.synchronize()
    out = dict(scores=r.scores.cpu().numpy(), labels=r.labels.cpu().numpy(), boxes=r.boxes.cpu().numpy(), n_kept=r.n_kept.cpu().numpy(),
               cell_conf=r.cell_conf.cpu().numpy(), cell_mask=r.cell_mask.cpu().numpy().astype(np.uint32))
    if dense:
        out["dense_scores"], out["dense_boxes"] = r.dense_scores.cpu().numpy(), r.dense_boxes.cpu().numpy()
    return out


def same_outputs(x, y):
    return all(np.array_equal(x[k], y[k]) for k in ("scores", "labels", "boxes", "n_kept", "cell_conf", "cell_mask"))


def check_image(out, b, dsc, dbx, H, W, thr, max_dets, grid, slot):
    """Teacher-forced: image b of ``out`` against the literal statement and the oracle selection on (dsc, dbx)."""
    from oracle import yolo_ref as R, searcher_ref as S
    lit = U.literal_select(dsc, dbx, (H, W), wrapper_thr=thr, max_dets=max_dets)
    sel = R.select(dsc, dbx, (H, W), wrapper_thr=thr, max_dets=max_dets)
    assert U.same_selection(lit, sel), "the literal statement and oracle.yolo_ref.select disagree"
    n = int(out["n_kept"][b])
    assert n == len(lit["scores"]), (b, n, len(lit["scores"]))
    assert np.array_equal(out["scores"][b, :n], lit["scores"])
    assert np.array_equal(out["labels"][b, :n], lit["labels"])
    assert np.array_equal(out["boxes"][b, :n], lit["xyxy"])
    assert (out["labels"][b, n:] == -1).all() and (out["scores"][b, n:] == 0).all() and (out["boxes"][b, n:] == 0).all()
    rows, cols = grid
    q = SLOT_Q[slot]
    texts = [[f"c{k}"] for k in range(q)]
    cm, names = S.image_grid_score(lit["xyxy"], lit["labels"], lit["scores"], texts, {f"c{k}": SLOT_W[slot][k] for k in range(q)}, H, W, rows, cols)
    assert np.array_equal(out["cell_conf"][b].reshape(rows, cols), cm)
    want = np.zeros(rows * cols, np.uint32)
    for cell, ns in enumerate(names):
        for nme in ns:
            want[cell] |= np.uint32(1) << np.uint32(int(nme[1:]))
    assert np.array_equal(out["cell_mask"][b], want)
    return lit


def check(out, sc, slots, thr=None, max_dets=None, grid=None):
    thr = sc["thr"] if thr is None else thr
    return [check_image(out, b, out["dense_scores"][b], out["dense_boxes"][b], sc["H"], sc["W"], thr, max_dets or sc["max_dets"],
                        grid or sc["grid"], slots[b]) for b in range(len(slots))]


def full_ranks(dsc):
    """(anchor, class, score) of every candidate in the published order (stable descending sort), before any cut."""
    a, k = np.nonzero(dsc > np.float32(0.001))
    v = dsc[a, k]
    o = np.argsort(-v, kind="stable")
    return a[o], k[o], v[o]


def report(name, lits, thr):
    for b, lit in enumerate(lits):
        print(f"reach {name} image {b}: {U.reach(lit, thr)}")


# ----------------------------------------------------------------------------- decode and scores
@pytest.mark.parametrize("H,W,Q", [(640, 640, 4), (380, 800, 32), (285, 600, 1), (360, 640, 4), (800, 380, 32), (320, 320, 1)])
def test_decode_and_scores_against_float64(env, H, W, Q):
    """head_decode_kernel against the float64 statement (yolo_post_util.decode_f64) on every anchor of a batch of two: DFL rows
    that are one-hot with four different bins (a side / bin transposition moves the box), all-zero (uniform), N(0, 3) and
    uniform in +-60 (the max subtraction); the first and last anchor of every level of every image are one-hot; class logits
    from -100 (expf overflows, score exactly 0) to +30 (saturated), and N(0, 3).
    Bound: 4 x the worst error of the oracle's float32 torch statement of the same quantity against float64, plus one float32
    ulp of the quantity's largest magnitude, and in any case the bounds of the full-forward tests (scores 1e-4, boxes
    0.05 * max(1, max(H, W) / 640) px).
    Measured on an MI355X, worst over the batch (HIP / the float32 statement; the test prints them per image):
      640x640 Q=4:  scores 8.8e-08 / 1.1e-07, boxes 9.6e-05 / 9.3e-05 px (one-hot rows exact)
      380x800 Q=32: scores 9.0e-08 / 1.0e-07, boxes 1.6e-04 / 1.6e-04 px
      285x600 Q=1:  scores 8.6e-08 / 1.0e-07, boxes 1.2e-04 / 1.2e-04 px
      360x640 Q=4:  scores 8.9e-08 / 1.0e-07, boxes 8.5e-05 / 1.0e-04 px
      800x380 Q=32: scores 9.2e-08 / 1.1e-07, boxes 1.3e-04 / 1.3e-04 px
      320x320 Q=1:  scores 8.8e-08 / 1.0e-07, boxes 4.2e-05 / 5.8e-05 px
    (the box figures are the float32 spacing of coordinates between 512 and 2048, 6e-5 .. 1.2e-4, in both)."""
    rs = np.random.RandomState(100 + H + Q)
    B = 2
    params = env["params"]
    lg = np.where(rs.rand(B, U.A, Q) < 0.5, rs.uniform(-100.0, 30.0, (B, U.A, Q)), 3.0 * rs.standard_normal((B, U.A, Q)))
    kind = rs.randint(0, 4, (B, U.A))
    bins = np.stack([rs.permutation(16)[:4] for _ in range(B * U.A)]).reshape(B, U.A, 4)        # four different bins
    dfl = U.onehot_dfl(bins)
    dfl[kind == 1] = 0.0
    dfl[kind == 2] = (3.0 * rs.standard_normal((int((kind == 2).sum()), 64))).astype(np.float32)
    dfl[kind == 3] = rs.uniform(-60.0, 60.0, (int((kind == 3).sum()), 64)).astype(np.float32)
    ends = [U.BASE[l] for l in range(3)] + [U.BASE[l] + U.SIZES[l] ** 2 - 1 for l in range(3)]
    dfl[:, ends] = U.onehot_dfl(np.broadcast_to(np.array([1, 5, 9, 14]), (B, 6, 4)))
    kind[:, ends] = 0
    sc = dict(logits=lg, dfl=dfl, H=H, W=W, thr=0.12, max_dets=100, grid=(4, 4))
    slot = {4: 0, 32: 1, 1: 2}[Q]
    dev = upload(sc, params)
    out = run(env, sc, dev, [slot] * B)
    e_all, d_all = U.embeds_from_logits(lg, params), U.dfl_levels(dfl)
    box_cap = 0.05 * max(1.0, max(H, W) / 640)
    for b in range(B):
        e = [x.reshape(B, -1, x.shape[1])[b] for x in e_all]
        d = [x.reshape(B, -1, 64)[b] for x in d_all]
        s64, b64 = U.decode_f64(e, d, params, H, W, Q)
        s32, b32 = U.decode_f32(e, d, params, H, W, Q)
        for what, hip, f32, f64, cap in (("score", out["dense_scores"][b], s32, s64, 1e-4), ("box", out["dense_boxes"][b], b32, b64, box_cap)):
            eh, e32 = float(np.abs(hip - f64).max()), float(np.abs(f32 - f64).max())
            bound = 4.0 * e32 + float(np.spacing(np.float32(np.abs(f64).max())))
            print(f"decode {H}x{W} Q={Q} image {b} {what}: HIP {eh:.3e}  float32 statement {e32:.3e}  bound {min(bound, cap):.3e}")
            assert eh <= bound and eh <= cap, (what, b, eh, e32, bound, cap)
        if (H, W) == (640, 640):                                        # ratio 1, no padding: one-hot rows decode to exact integers
            hot = kind[b] == 0
            assert np.array_equal(out["dense_boxes"][b][hot].astype(np.float64), b64[hot])
        lo = lg[b] < -95.0
        assert lo.any() and (out["dense_scores"][b][lo] == 0).all()      # expf overflow: exactly 0
        assert (out["dense_scores"][b][lg[b] > 25.0] == 1).all()         # saturated
    if Q <= 4:                                                          # and the selection on these free-form boxes, teacher-forced
        check(out, sc, [slot] * B)


# ----------------------------------------------------------------------------- selection scenarios
def test_few_candidates_and_empty_images(env):
    """Scenario 1, the real-checkpoint regime: no cut, LDS sort of a short list; an image with no candidate at all between two
    others in one batch (which also spans two chunks), and one whose candidates all stay below the wrapper threshold."""
    sc = U.scenario_few()
    dev = upload(sc, env["params"])
    out = run(env, sc, dev, [0, 0, 0])
    lits = check(out, sc, [0, 0, 0])
    report("few", lits, sc["thr"])
    r = [U.reach(l, sc["thr"]) for l in lits]
    assert 1000 < r[0]["candidates"] <= 5000 and 0 < r[0]["above"] and out["n_kept"][0] > 0
    assert r[1]["candidates"] == 0 and out["n_kept"][1] == 0 and not out["cell_conf"][1].any() and not out["cell_mask"][1].any()
    assert r[2]["candidates"] > 100 and r[2]["above"] == 0 and out["n_kept"][2] == 0
    for thr, md in ((0.0005, 300), (0.12, 7)):
        o2 = run(env, sc, dev, [0, 0, 0], thr=thr, max_dets=md)
        l2 = check(o2, sc, [0, 0, 0], thr=thr, max_dets=md)
        assert len(l2[2]["scores"]) > 0 or thr > 0.01


def test_the_nms_pre_cut_decides(env):
    """Scenario 2 (see yolo_post_util.scenario_cut) and scenario 8 on it: three runs, bit-equal."""
    from oracle import yolo_ref as R
    sc = U.scenario_cut()
    dev = upload(sc, env["params"])
    out = run(env, sc, dev, [0, 0])
    lits = check(out, sc, [0, 0])
    report("cut", lits, sc["thr"])
    for b, lit in enumerate(lits):
        dsc, dbx = out["dense_scores"][b], out["dense_boxes"][b]
        a, k, v = full_ranks(dsc)
        big = U.CUT_BIG[b]
        assert len(v) == (33600, 33597)[b] and lit["n_sorted"] == 30000
        assert dbx.max() == U.CUT_MAX[b] == dbx[big].max() and np.flatnonzero(a == big).min() >= 30000     # the largest coordinate is cut away
        assert dbx[np.unique(a[:30000])].max() == 667 and lit["off_unit"] == 668.0
        want = [(U.CUT_P, 0), (U.CUT_PIN, 0)] if b == 0 else [(U.CUT_P, 0), (U.CUT_P2, 2), (U.CUT_Q2, 3), (U.CUT_PIN, 0)]
        assert [(int(x), int(c)) for x, c in zip(lit["anchors"], lit["labels"])] == want
        nocut = R.select(dsc, dbx, (640, 640), max_dets=300, nms_pre=10 ** 9)
        assert (U.CUT_Q, 1) in [(int(x), int(c)) for x, c in zip(nocut["anchors"], nocut["labels"])]
    # image 1: bit-equal scores straddle rank 30000; the last kept candidate alone holds the kept maximum, the first cut one the overall maximum
    assert v[29999] == v[30000] and np.count_nonzero(v == v[30000]) == 1993 and v[29002] > v[29003] and v[30995] > v[30996]
    assert (a[29999], k[29999]) == (U.CUT_LAST, 3) and (a[30000], k[30000]) == (U.CUT_BIG[1], 0)
    assert dbx[np.unique(a[:29999])].max() == 664 and dbx[np.unique(a[:30001])].max() == 732
    for _ in range(2):
        assert same_outputs(out, run(env, sc, dev, [0, 0], dense=False))


def test_global_sort_fallback(env):
    """Scenario 3 (see yolo_post_util.scenario_fallback) with Q = 32 and scenario 8 on it: three runs, bit-equal."""
    sc = U.scenario_fallback()
    dev = upload(sc, env["params"])
    out = run(env, sc, dev, [1, 1, 1])
    lits = check(out, sc, [1, 1, 1])
    report("fallback", lits, sc["thr"])
    r = [U.reach(l, sc["thr"]) for l in lits]
    above_all = [int(np.count_nonzero(out["dense_scores"][b] > np.float32(sc["thr"]))) for b in range(3)]
    print("fallback: candidates above the wrapper threshold before the cut:", above_all)
    assert r[0]["candidates"] == 268800 and above_all[0] > 30000 and r[0]["above"] == 30000          # cut and fallback combine
    assert r[1]["candidates"] == 80000 and 16384 < above_all[1] < 30000 and r[1]["examined"] == above_all[1] and r[1]["survivors"] < 300
    assert r[2]["candidates"] == 24999 and 16384 < above_all[2] and r[2]["examined"] == above_all[2] and r[2]["survivors"] < 300
    assert out["n_kept"][0] == 300 and int(out["labels"][0].max()) == 31
    for _ in range(2):
        assert same_outputs(out, run(env, sc, dev, [1, 1, 1], dense=False))


def test_long_greedy_pass(env):
    """Scenario 4 (see yolo_post_util.scenario_greedy): thousands of candidates examined, 300 survivors out of 400, and the three
    kinds of suppression the one-wave pass must get right."""
    sc = U.scenario_greedy()
    dev = upload(sc, env["params"])
    out = run(env, sc, dev, [0, 0])
    lits = check(out, sc, [0, 0])
    report("greedy", lits, sc["thr"])
    for b, lit in enumerate(lits):
        r = U.reach(lit, sc["thr"])
        assert r["survivors"] == 300 and r["survivors_available"] == 400 and 2000 < r["examined"] < r["above"] <= 16384, r
        assert out["n_kept"][b] == 300
        ex = r["examined"]
        lo, hi, kr = lit["sup_lo"][:ex], lit["sup_hi"][:ex], lit["keep_ranks"]
        for first in (64, 128, 256):                                  # suppressed ONLY by a survivor of a later stride of the lane loop
            assert np.count_nonzero(lo >= first) > 0
        one = np.flatnonzero((lo >= 0) & (lo == hi))
        fetch_c, fetch_s = one // 64, kr[lo[one]] // 64
        assert np.count_nonzero(fetch_c == fetch_s) > 100            # ... by a survivor accepted earlier in the same 64-candidate fetch
        assert np.count_nonzero(fetch_c - fetch_s >= 20) > 10        # ... by a survivor from a much earlier fetch
    o2 = run(env, sc, dev, [0, 0], max_dets=100)                     # inference()'s default
    check(o2, sc, [0, 0], max_dets=100)


def test_ties_and_thresholds(env):
    """Scenario 5 (see yolo_post_util.scenario_ties)."""
    sc = U.scenario_ties()
    dev = upload(sc, env["params"])
    out = run(env, sc, dev, [0, 0])
    lits = check(out, sc, [0, 0])
    report("ties", lits, sc["thr"])
    dsc, dbx = out["dense_scores"], out["dense_boxes"]
    tie = dsc[0, U.anchor(0, 0, 4), 0]
    assert np.count_nonzero(dsc[0] == tie) == 400 and np.count_nonzero(dsc[0] > tie) == 20
    assert out["n_kept"][0] == 300 and out["scores"][0, 20] == tie and out["scores"][0, 299] == tie and out["scores"][0, 19] > tie
    # image 1: exact IoUs from integer boxes
    kept = {(int(a), int(c)) for a, c in zip(lits[1]["anchors"], lits[1]["labels"])}
    f = np.float32
    for suffix in "02":
        (aa, c), (ab, _), (ac, _) = (U.TIE_IOU[n + suffix] for n in "ABC")
        A_, B_, C_ = dbx[1, aa], dbx[1, ab], dbx[1, ac]
        assert A_.tolist() == [4, 68 + 160 * (suffix == "2"), 84, 100 + 160 * (suffix == "2")]
        area = lambda q: (q[2] - q[0]) * (q[3] - q[1])
        inter = lambda p, q: max(min(p[2], q[2]) - max(p[0], q[0]), f(0)) * max(min(p[3], q[3]) - max(p[1], q[1]), f(0))
        assert inter(A_, B_) / (area(A_) + area(B_) - inter(A_, B_)) == f(0.7)
        assert inter(A_, C_) / (area(A_) + area(C_) - inter(A_, C_)) == f(0.8)
        assert (aa, c) in kept and (ab, c) in kept and (ac, c) not in kept
    assert lits[1]["off_unit"] == 657.0
    for n in ("Z0", "Z1"):
        an, c = U.TIE_IOU[n]
        assert dbx[1, an, 0] == dbx[1, an, 2] and (an, c) in kept
    # the wrapper's knobs on the same input
    o = run(env, sc, dev, [0, 0], max_dets=50)
    check(o, sc, [0, 0], max_dets=50)
    assert o["n_kept"][0] == 50 and o["scores"][0, 49] == tie
    o = run(env, sc, dev, [0, 0], thr=float(tie))                     # strictly greater
    check(o, sc, [0, 0], thr=float(tie))
    assert o["n_kept"][0] == 20
    o = run(env, sc, dev, [0, 0], thr=float(out["scores"][1, 3]))
    check(o, sc, [0, 0], thr=float(out["scores"][1, 3]))
    assert o["n_kept"][1] == np.count_nonzero(out["scores"][1] > out["scores"][1, 3])
    o = run(env, sc, dev, [0, 0], thr=0.0005)                         # below score_thr: 0.001 still decides who is a candidate
    l5 = check(o, sc, [0, 0], thr=0.0005)
    for b in range(2):
        assert np.count_nonzero((dsc[b] > 0.0005) & (dsc[b] <= 0.001)) == 50 and l5[b]["scores"].min() > 0.001
        assert o["n_kept"][b] == 300 or b == 1
    assert o["n_kept"][1] > out["n_kept"][1]


def test_classes_and_mixed_query_sets(env):
    """Scenario 6: Q = 32, 4 and 1 in one batch.  Dense outputs need one Q per call, so each image's dense scores come from a
    call with its own set for the whole batch; the mixed call must then equal the literal statement on them."""
    sc = U.scenario_classes()
    dev = upload(sc, env["params"])
    slots = [1, 0, 2]
    mixed = run(env, sc, dev, slots, dense=False)
    lits = []
    for b, slot in enumerate(slots):
        uni = run(env, sc, dev, [slot] * 3)
        lits.append(check_image(mixed, b, uni["dense_scores"][b], uni["dense_boxes"][b], sc["H"], sc["W"], sc["thr"], sc["max_dets"], sc["grid"], slot))
        assert uni["dense_scores"].shape[2] == SLOT_Q[slot]
        assert same_outputs({k: v[b] for k, v in uni.items()}, {k: v[b] for k, v in mixed.items()})
    report("classes", lits, sc["thr"])
    hot = U.anchor(1, 7, 7)
    assert sorted(lits[0]["labels"][lits[0]["anchors"] == hot].tolist()) == list(range(32)) and lits[0]["labels"][0] == 31
    assert sorted(lits[1]["labels"][lits[1]["anchors"] == hot].tolist()) == list(range(4)) and lits[1]["labels"].max() == 3
    assert len(lits[2]["labels"]) > 0 and lits[2]["labels"].max() == 0
    assert int(mixed["cell_mask"][0].max()) >= 1 << 31


def test_cells(env):
    """Scenario 7 (see yolo_post_util.scenario_cells): 1 x 1, 4 x 4 and 16 x 16 grids over 300 detections, non-dyadic weights; then
    the scenario's grids of non-representable cells, (3, 7) and (14, 12): on the second the centre (160, 180) lies on a border of
    both axes, where the cell is numpy 1.26's float64 floor_divide (row 6, column 2), not floor(c / cell) (row 7, column 3)."""
    sc = U.scenario_cells()
    dev = upload(sc, env["params"])
    assert U.cell_index_forms(160.0, 640, 12) == (2, 3) and U.cell_index_forms(180.0, 360, 14) == (6, 7)      # the case cannot go dead
    for grid in ((1, 1), (4, 4), (16, 16)) + sc["border_grids"]:
        out = run(env, sc, dev, [0, 0], grid=grid)
        lits = check(out, sc, [0, 0], grid=grid)
        for b, lit in enumerate(lits):
            assert out["n_kept"][b] == 300
            raw = out["dense_boxes"][b][lit["anchors"]]
            assert (raw[:, 3] < 0).any() and (raw[:, 1] > 360).any() and raw.min() < -200 and raw.max() > 800   # outside before the clamp
            cx, cy = (lit["xyxy"][:, 0] + lit["xyxy"][:, 2]) / 2, (lit["xyxy"][:, 1] + lit["xyxy"][:, 3]) / 2
            assert ((cx == 160) & (cy == 180)).any()                   # on a border of the 4 x 4 and the 16 x 16 grid
            assert len(np.unique(out["cell_conf"][b])) > (0 if grid == (1, 1) else 3)
    report("cells", lits, sc["thr"])
