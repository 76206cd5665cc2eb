"""Image-guided (one-shot) detection end to end, on the device:

* the post-process kernel through ``tstar_image_guided_postprocess`` against the host entry (which
  tests/test_image_guided_post_host.py pins to HF bit for bit), word for word on every crafted case;
* the selection kernel with a query box through ``tstar_image_query_select_box`` against the numpy restatement;
* ``OWLInterface.detect_image_guided`` on HF-initialised checkpoints against HF's ``image_guided_detection`` +
  ``post_process_image_guided_detection`` on the CPU;
* the surface: the searcher's query sets are untouched, ``set_query_images`` with a box."""
import numpy as np
import pytest
import torch

import image_guided_post_util as G
import image_query_util as U

pytestmark = pytest.mark.gpu

POISON_F, POISON_I, POISON_B = np.float32(-77.25), np.int32(-12345), 0xA5
CASES = G.build_cases()


# ------------------------------------------------------------------------------------------------------------ the kernel
def _post(scores, boxes, threshold, nms, scale):
    """``tstar_image_guided_postprocess`` on [B, np] scores / [B, np, 4] boxes with 64 rows of NaN behind the last image; every
    output has room for one image more, filled with poison, which must come back untouched."""
    from tstar_amd import _lib
    lib = _lib.load()
    B, n = scores.shape
    d_s = torch.full((B * n + 64,), float("nan"), device="cuda")
    d_b = torch.full((B * n + 64, 4), float("nan"), device="cuda")
    d_s[:B * n] = torch.from_numpy(scores.reshape(-1)).cuda()
    d_b[:B * n] = torch.from_numpy(boxes.reshape(-1, 4)).cuda()
    a = torch.full(((B + 1) * n,), float(POISON_F), device="cuda")
    x = torch.full(((B + 1) * n, 4), float(POISON_F), device="cuda")
    k = torch.full(((B + 1) * n,), POISON_B, dtype=torch.uint8, device="cuda")
    cnt = torch.full((B + 1,), int(POISON_I), dtype=torch.int32, device="cuda")
    rc = lib.tstar_image_guided_postprocess(d_s.data_ptr(), d_b.data_ptr(), B, n, float(threshold), float(nms),
                                            None if scale is None else np.ascontiguousarray(scale, dtype=np.float32).ctypes.data,
                                            a.data_ptr(), x.data_ptr(), k.data_ptr(), cnt.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "tstar_image_guided_postprocess")
    torch.cuda.synchronize()
    a, x, k, cnt = a.cpu().numpy(), x.cpu().numpy(), k.cpu().numpy(), cnt.cpu().numpy()
    assert (a[B * n:] == POISON_F).all() and (x[B * n:] == POISON_F).all() and (k[B * n:] == POISON_B).all() and cnt[B] == POISON_I
    assert torch.isnan(d_s[B * n:]).all() and torch.isnan(d_b[B * n:]).all()
    return a[:B * n].reshape(B, n), x[:B * n].reshape(B, n, 4), k[:B * n].reshape(B, n), cnt[:B]


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_kernel_is_the_host_entry_word_for_word(case):
    """Every crafted case of the host test (np = 3600 at B = 3 included): alphas, scaled boxes, keep mask and kept count of the
    kernel are the host entry's words -- the host entry tests every pair as HF does, the kernel only the candidates behind the
    live one, so this also checks the symmetry argument of csrc/image_guided_post.hip.  Poison behind every output and the NaN
    rows behind the last image stay as they were."""
    scores, scale = G.scores_of(case["logits"]), G.scale_of(case["sizes"])
    want = G.host_entry(scores, case["boxes"], case["threshold"], case["nms"], scale)
    got = _post(scores, case["boxes"], case["threshold"], case["nms"], scale)
    assert np.array_equal(got[3], want[3]), (got[3], want[3])
    assert np.array_equal(got[2], want[2])
    assert G.same_bits(got[0], want[0]) and G.same_bits(got[1], want[1])
    for b, r in enumerate(G.restated(case)):                    # and the restatement's kept set, which is HF's
        assert np.array_equal(got[2][b].astype(bool), r["keep"]), b


def test_kernel_refuses_bad_arguments_and_launches_nothing():
    from tstar_amd import _lib
    lib = _lib.load()
    s, b = torch.full((3601,), 0.5, device="cuda"), torch.full((3601, 4), 0.25, device="cuda")
    a, x = torch.full((3601,), float(POISON_F), device="cuda"), torch.full((3601, 4), float(POISON_F), device="cuda")
    k, cnt = torch.full((3601,), POISON_B, dtype=torch.uint8, device="cuda"), torch.full((1,), int(POISON_I), dtype=torch.int32, device="cuda")

    def call(sp=s.data_ptr(), B=1, n=4, ap=a.data_ptr(), kp=k.data_ptr()):
        return lib.tstar_image_guided_postprocess(sp, b.data_ptr(), B, n, 0.0, 0.3, None, ap, x.data_ptr(), kp, cnt.data_ptr(), _lib.stream_ptr())

    for kw in (dict(n=3601), dict(n=0), dict(B=0), dict(B=65536), dict(sp=None), dict(ap=None), dict(kp=None)):
        assert call(**kw) == 1, kw
        assert lib.tstar_last_error()
    torch.cuda.synchronize()
    assert (a == float(POISON_F)).all() and (x == float(POISON_F)).all() and (k == POISON_B).all() and int(cnt[0]) == int(POISON_I)
    assert call() == 0
    torch.cuda.synchronize()
    assert int(cnt[0]) == 1 and k[:4].tolist() == [1, 0, 0, 0]             # four identical boxes and scores: the lowest index survives


# ------------------------------------------------------------------------------------------------------------ query boxes
SENTINEL_F, SENTINEL_I = np.float32(-77.25), np.int32(-12345)


def _select_box(cls_list, boxes_list, qboxes, np_, entry="box"):
    """``tstar_image_query_select_box`` (or, ``entry="plain"``, ``tstar_image_query_select``) laid out as tests/test_gpu_image_query.py
    does: NaN rows behind the last image, and behind the last query box; one sentinel entry behind every host output."""
    from tstar_amd import _lib
    lib = _lib.load()
    n = len(cls_list)
    cls = torch.full((n * np_ + 64, U.PROJ), float("nan"), device="cuda")
    boxes = torch.full((n * np_ + 64, 4), float("nan"), device="cuda")
    cls[:n * np_] = torch.from_numpy(np.concatenate(cls_list)).cuda()
    boxes[:n * np_] = torch.from_numpy(np.concatenate(boxes_list)).cuda()
    emb, box = np.full((n + 1, U.PROJ), SENTINEL_F, np.float32), np.full((n + 1, 4), SENTINEL_F, np.float32)
    best, nsel, status = (np.full(n + 1, SENTINEL_I, np.int32) for _ in range(3))
    tail = (emb.ctypes.data, best.ctypes.data, box.ctypes.data, nsel.ctypes.data, status.ctypes.data, _lib.stream_ptr())
    if entry == "plain":
        rc = lib.tstar_image_query_select(cls.data_ptr(), boxes.data_ptr(), n, np_, *tail)
    else:
        dq = None
        if qboxes is not None:
            dq = torch.full((n + 1, 4), float("nan"), device="cuda")
            dq[:n] = torch.from_numpy(np.stack(qboxes)).cuda()
        rc = lib.tstar_image_query_select_box(cls.data_ptr(), boxes.data_ptr(), None if dq is None else dq.data_ptr(), n, np_, *tail)
    _lib.check(rc, "tstar_image_query_select_box")
    assert np.all(emb[n] == SENTINEL_F) and np.all(box[n] == SENTINEL_F) and best[n] == nsel[n] == status[n] == SENTINEL_I
    return emb[:n], best[:n], box[:n], nsel[:n], status[:n]


@pytest.mark.parametrize("np_", G.BOX_NP)
def test_selection_kernel_with_query_boxes(np_):
    """The crafted cases of tests/image_query_util.py against the unit box and, scaled by 1/2 with the exact-threshold straddle
    among them, against [0, 0, 0.5, 0.5]; a small off-centre box with a planted match, with the GIoU fallback and with a negative
    largest GIoU (status 2): selected count, best index, embedding and box bits and status are the restatement's, three images
    with three different boxes per call.  With unit boxes, and with no boxes, the outputs are ``tstar_image_query_select``'s bits."""
    cases = G.box_cases(np_)
    for k in range(0, len(cases), 3):
        call = [cases[(k + j) % len(cases)] for j in range(3)]
        emb, best, box, nsel, status = _select_box([c[1] for c in call], [c[2] for c in call], [c[3] for c in call], np_)
        for j, (label, cls, boxes, q, r) in enumerate(call):
            where = (np_, label)
            assert status[j] == r["status"] and nsel[j] == r["n_selected"] and best[j] == r["best"], (where, status[j], nsel[j], best[j])
            if r["best"] < 0:
                assert not emb[j].view(np.uint32).any() and not box[j].view(np.uint32).any(), where
            else:
                assert np.array_equal(emb[j].view(np.uint32), cls[r["best"]].view(np.uint32)), where
                assert np.array_equal(box[j].view(np.uint32), boxes[r["best"]].view(np.uint32)), where
    unit = [c for c in cases if np.array_equal(c[3], G.UNIT)]
    cls_l, box_l = [c[1] for c in unit], [c[2] for c in unit]
    plain = _select_box(cls_l, box_l, None, np_, entry="plain")
    for qb in ([G.UNIT] * len(unit), None):
        got = _select_box(cls_l, box_l, qb, np_)
        for a, b in zip(got, plain):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# -------------------------------------------------------------------------------------------------- end to end against HF
# seeds of the images at which HF's own preconditions hold (found on the CPU; asserted below, on HF's side, before anything else)
E2E_SEED = {("b32", False): 0, ("v2", False): 33, ("b32", True): 20}


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    out = {}
    for g in ("b32", "v2"):
        d = str(tmp_path_factory.mktemp(f"image_guided_post_{g}"))
        out[g] = (d, G.e2e_checkpoint(g, d))
    return out


_REF = {}


def _reference(g, model, qbox):
    key = (g, qbox)
    if key not in _REF:
        example, targets = G.e2e_images(E2E_SEED[(g, qbox is not None)])
        ref = G.hf_one_shot(g, model, example, targets, qbox)
        ref["kept"], ref["margin"], ref["gap"] = G.assert_one_shot_preconditions(ref)
        _REF[key] = ref
    return _REF[key]


@pytest.mark.parametrize("g,mode,qbox", [("b32", "f32", None), ("b32", "f32x3", None), ("v2", "f32", None), ("v2", "f32x3", None),
                                         ("b32", "f32", G.E2E_QBOX_PX), ("b32", "f32x3", G.E2E_QBOX_PX)])
def test_detect_image_guided_matches_hf(ckpts, g, mode, qbox):
    """One example image, two target images (285 x 600 and a 1520 x 3200 grid image) through an HF-initialised checkpoint (B/32 at
    96 x 128, OWLv2 at 64 x 64):
    ``detect_image_guided`` against HF's ``image_guided_detection`` + ``post_process_image_guided_detection(threshold=0.0,
    nms_threshold=0.3, target_sizes)``; with a query box, against HF's forward and the general-box selection of the util.  HF's
    side first (``assert_one_shot_preconditions``): every IoU that decides a suppression at least 1e-3 from 0.3, neighbouring scores
    more than 2e-3 apart (pairs of OWLv2 padding patches, which never are: the kept set does not depend on their order), HF
    suppresses something and keeps fewer patches than there are.  Then the
    same kept patches, alphas within (|ds| + 0.1 |dm|) / (0.9 m) for |ds|, |dm| <= 1e-3 (the project's score bound carried through
    the alpha formula), boxes within 1e-2 px.  Observed values are printed."""
    from tstar_amd.interface_heuristic import OWLInterface
    family, patch, size = G.E2E_GEOMETRIES[g]
    d, model = ckpts[g]
    ref = _reference(g, model, qbox)
    h = OWLInterface(model_name_or_path=d, max_batch=2, weights_dtype=mode, input_size=size)
    assert h.family == family
    h.reparameterize_object_list(["couch"], ["tv"])
    example, targets = G.e2e_images(E2E_SEED[(g, qbox is not None)])
    res = h.detect_image_guided(targets, example, query_boxes=qbox)
    assert len(res) == len(targets)
    worst_a, worst_b = 0.0, 0.0
    for b, (r, k) in enumerate(zip(res, ref["kept"])):
        assert r["labels"] is None and r["scores"].dtype == np.float32 and r["boxes"].dtype == np.float32
        assert np.array_equal(r["patches"], k["patches"]), (b, r["patches"], k["patches"])
        assert len(r["detections"]) == len(k["patches"]) and np.array_equal(r["detections"].xyxy, r["boxes"])
        da = float(np.abs(r["scores"].astype(np.float64) - k["alphas"]).max())
        db = float(np.abs(r["boxes"].astype(np.float64) - k["boxes"]).max())
        worst_a, worst_b = max(worst_a, da / G.alpha_bound(k["m"])), max(worst_b, db)
        print(f"{g} {mode} box={qbox} image {b}: kept {len(k['patches'])} of {ref['probs'].shape[1]}, max |alpha - HF| = {da:.2e} "
              f"(bound {G.alpha_bound(k['m']):.2e}), max |box - HF| = {db:.2e} px")
        assert da <= G.alpha_bound(k["m"]), (b, da, G.alpha_bound(k["m"]))
        assert db < G.BOX_BOUND, (b, db)
    print(f"{g} {mode} box={qbox}: HF's IoU margin to 0.3 = {ref['margin']:.2e}, smallest score gap = {ref['gap']:.2e}, HF suppresses "
          f"{ref['n_suppressed']} patches; padding pairs closer than 2e-3: {ref['padding_pairs']}")
    del h


# ------------------------------------------------------------------------------------------------------------ the surface
SIZE = (160, 224)                                     # B/32: 35 patches


@pytest.fixture(scope="module")
def heur():
    from tstar_amd.interface_heuristic import OWLInterface
    return OWLInterface(synthetic_seed=0, max_batch=16, input_size=SIZE)


def _searcher(h, store, seed):
    from tstar_amd.interface_searcher import TStarSearcher
    return TStarSearcher(store, h, ["mug"], ["tv"], search_nframes=4, image_grid_shape=(3, 3), search_budget=0.4, confidence_threshold=0.6,
                         rng=np.random.RandomState(seed), keep_visual_history=False)


def test_searcher_untouched_by_detect_image_guided(heur):
    """The registry's query sets are what they were after ``detect_image_guided`` -- ``texts``, the slots the scorer holds and their
    embeddings -- also when the distinct examples outnumber the free slots and go through in groups; a search after the call
    gives the keyframes of a search before it; per-image queries give what one call per image gives."""
    from tstar_amd.video import synthetic_video
    h = heur
    h.clear_query_images()
    store = synthetic_video(160, seed=31)
    fr0, ts0 = _searcher(h, store, 70).search()
    h.reparameterize_object_list(["couch", "mug"], ["tv"])
    for slot in range(3, 62):                                   # 59 more slots held: 0 and 3..61; free are 1, 2, 62, 63
        h.install_queries(slot, ["dog"], ["lamp"])
    texts = [list(t) for t in h.texts]
    held = sorted(set(h.scorer.Qs) | set(h.scorer._pending))
    assert len(held) == 60
    before = {sl: h.scorer.get_query_embeds(sl) for sl in held}
    examples = U.example_images(17, 6, 120, 168)
    targets = [U.example_images(18 + b, 1, 95, 200)[0] for b in range(6)]
    res = h.detect_image_guided(targets, list(examples))          # six distinct examples, four free slots
    assert h.texts == texts and sorted(set(h.scorer.Qs) | set(h.scorer._pending)) == held
    for sl in held:
        assert np.array_equal(h.scorer.get_query_embeds(sl).view(np.uint32), before[sl].view(np.uint32)), sl
    for b in range(6):
        one = h.detect_image_guided([targets[b]], examples[b])[0]
        assert np.array_equal(one["patches"], res[b]["patches"]) and G.same_bits(one["scores"], res[b]["scores"]), b
        assert G.same_bits(one["boxes"], res[b]["boxes"]) and len(res[b]["patches"]) >= 1, b
    fr1, ts1 = _searcher(h, store, 70).search()
    assert ts1 == ts0 and np.array_equal(fr1, fr0)
    with pytest.raises(ValueError, match="query image 1"):
        h.detect_image_guided(targets[:2], [examples[0], np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError, match="outside"):
        h.detect_image_guided(targets[:1], examples[0], query_boxes=(0, 0, 169, 10))


def test_status_2_raises_naming_the_index(heur, monkeypatch):
    """An example from which no query can be formed (status 2 of the selection: an empty selection, as a query box gives that no
    prediction overlaps) raises ValueError naming the index of the FIRST image that uses it, and the registry is untouched."""
    from tstar_amd.owl import ImageQueryResult
    h = heur
    examples = U.example_images(17, 3, 120, 168)
    targets = [U.example_images(18 + b, 1, 95, 200)[0] for b in range(3)]
    held = dict(h.scorer.Qs)

    def stub(images, query_boxes=None):
        n = images.shape[0]
        assert n == 2 and query_boxes is None                                    # the distinct examples, embedded once each
        return ImageQueryResult(embeds=np.ones((n, 512), np.float32), best=np.array([3, -1], np.int32), boxes_cxcywh=np.zeros((n, 4), np.float32),
                                n_selected=np.array([2, 0], np.int32), status=np.array([0, 2], np.int32))

    monkeypatch.setattr(h.scorer, "embed_image_queries", stub)
    ex0, ex1 = examples[0], examples[1]
    with pytest.raises(ValueError, match="query image 1:"):
        h.detect_image_guided(targets, [ex0, ex1, ex1])
    with pytest.raises(ValueError, match="query image 2:"):
        h.detect_image_guided(targets, [ex0, ex0, ex1])
    assert dict(h.scorer.Qs) == held


def test_detect_image_guided_is_score_plus_the_kernel(heur):
    """What ``detect_image_guided`` returns is the post-process kernel on ``score(..., want_logits=True)`` of a hand-installed
    one-query slot: the host entry on those scores and boxes gives the same rows, bit for bit."""
    h = heur
    example = U.example_images(17, 1, 120, 168)[0]
    targets = [U.example_images(18 + b, 1, 95, 200)[0] for b in range(3)]
    res = h.detect_image_guided(targets, example, threshold=0.2, nms_threshold=0.5)
    r = h.scorer.embed_image_queries(torch.from_numpy(example[None]).cuda())
    h.scorer.set_query_embeds(r.embeds[:1], [1], [1.0], slot=40)
    try:
        sc = h.scorer.score(torch.from_numpy(np.stack(targets)).cuda(), 1, 1, want_logits=True, image_sets=[40] * 3)
        torch.cuda.synchronize()
        scores, cx = sc.scores.cpu().numpy(), sc.boxes_cxcywh.cpu().numpy()
        a, x, k, n = G.host_entry(scores, cx, 0.2, 0.5, np.array([[200, 95]] * 3, np.float32))
    finally:
        h.scorer.Qs.pop(40, None)
    for b in range(3):
        m = k[b].astype(bool)
        assert np.array_equal(res[b]["patches"], np.nonzero(m)[0]) and G.same_bits(res[b]["scores"], a[b][m]) and G.same_bits(res[b]["boxes"], x[b][m]), b


def test_set_query_images_with_a_box(heur):
    """``set_query_images({"mug": (img, box)})`` then ``reparameterize_object_list`` installs the embedding that
    ``embed_image_queries(img, query_boxes=...)`` returns for the relative box; ``query_image_info`` carries the box; a bad box
    raises ValueError naming the object and registers nothing."""
    h = heur
    h.clear_query_images()
    img = U.example_images(41, 1, 120, 168)[0]
    box_px = (20, 10, 150, 110)
    rel = G.relative_box(box_px, 120, 168)
    r = h.scorer.embed_image_queries(torch.from_numpy(img[None]).cuda(), query_boxes=rel[None])
    whole = h.scorer.embed_image_queries(torch.from_numpy(img[None]).cuda())
    assert r.status[0] != 2
    h.set_query_images({"mug": (img, box_px), "cup": img})
    info = h.query_image_info["mug"]
    assert np.array_equal(info["query_box"], rel) and info["best_index"] == int(r.best[0]) and h.query_image_info["cup"]["query_box"] is None
    assert np.array_equal(h._query_images["mug"].view(np.uint32), r.embeds[0].view(np.uint32))
    assert np.array_equal(h._query_images["cup"].view(np.uint32), whole.embeds[0].view(np.uint32))
    h.reparameterize_object_list(["couch", " mug "], ["tv"])
    assert np.array_equal(h.scorer.get_query_embeds(0)[1].view(np.uint32), r.embeds[0].view(np.uint32))
    for bad in ((40, 24, 40, 104), (136, 24, 40, 104), (0, 0, 169, 10)):
        with pytest.raises(ValueError, match="'vase'"):
            h.set_query_images({"vase": (img, bad)})
    assert "vase" not in h._query_images and "vase" not in h.query_image_info
    h.clear_query_images()
