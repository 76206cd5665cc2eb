"""tstar_owl_score_cells / ``score_batch(..., boxes=False)``: the 1 x 1 forward without the box head.

With one grid cell the boxes reach no output but themselves (every kept detection falls in cell 0), so the entry skips the box
head's two GELU GEMMs, the box tail of detect_rows and both box stores.  The class head's launches are the same, hence:

* every other output holds the bits of the full entry, in each weights mode, on both workspace lanes, across a full and a partial
  forward chunk, and on a B/16 and an OWLv2 handle at their smallest input;
* a grid of more than one cell is refused before anything is launched;
* a search without a visual history (which takes the entry for its verification frames) equals the search with one (which does
  not), alone and as a lock-step group;
* asking such a result for boxes raises the documented error.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODES = ("f32", "f32x3", "bf16", "bf16_exact")


def _token_ids(names):
    """Hand-made CLIP-style ids (no vocabulary needed): [BOS, toks.., EOS, 0 pad]."""
    ids = np.zeros((len(names), 16), dtype=np.int64)
    am = np.zeros((len(names), 16), dtype=np.int64)
    for i, n in enumerate(names):
        toks = [49406] + [1000 + (sum(map(ord, w)) * 31 + len(w)) % 40000 for w in n.split()] + [49407]
        ids[i, :len(toks)] = toks
        am[i, :len(toks)] = 1
    return ids, am


def _scorer(mode, family="owlvit", patch=None, size=None, max_batch=2):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    g = W.with_input_size(W.geometry_for_family(family, patch), size)
    sd = W.synthetic_state_dict(0, "both", geometry=g)
    sc = OwlScorer(W.pack_blob(sd, W.vision_spec(g), g), W.pack_blob(sd, W.text_spec(g)), max_batch=max_batch, weights_mode=mode,
                   patch_size=patch, input_size=size, family=family)
    ids, am = _token_ids(["couch", "tv", "chair", ""])
    sc.set_queries(ids, am, [1.0, 0.7, 0.5, 0.5])
    return sc


def _images(B, H, W, seed):
    rs = np.random.RandomState(seed)
    low = rs.randint(0, 256, (B, H // 8 + 1, W // 8 + 1, 3)).astype(np.float32)
    img = np.repeat(np.repeat(low, 8, axis=1), 8, axis=2)[:, :H, :W] + rs.randint(-20, 20, (B, H, W, 3))
    return torch.from_numpy(np.clip(img, 0, 255).astype(np.uint8)).cuda()


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32).cpu().numpy()


def _assert_same_bits(full, cells, fields, what):
    for f in fields:
        a, b = getattr(full, f), getattr(cells, f)
        assert a is not None and b is not None, (what, f)
        assert np.array_equal(_bits(a), _bits(b)), f"{what}: {f} differs from the full entry"
    assert cells.boxes is None and cells.boxes_cxcywh is None


def _both_lanes(sc, imgs, what, objectness=False, must_keep=True):
    fields = ["scores", "labels", "cell_conf", "cell_mask", "n_kept", "logits"] + (["objectness"] if objectness else [])
    for lane in (0, 1):
        full = sc.score(imgs, 1, 1, want_logits=True, lane=lane, objectness=objectness)
        cells = sc.score(imgs, 1, 1, want_logits=True, lane=lane, objectness=objectness, boxes=False)
        torch.cuda.synchronize()
        assert not must_keep or int(full.n_kept.sum()) > 0, "the case must keep detections, or cell_conf / cell_mask check nothing"
        _assert_same_bits(full, cells, fields, f"{what} lane {lane}")


@pytest.mark.parametrize("mode", MODES)
def test_equal_bits_in_every_weights_mode(mode):
    """B = 3 verification-size images with max_batch = 2: a full forward chunk and a partial one, on both lanes."""
    sc = _scorer(mode)
    try:
        _both_lanes(sc, _images(3, 285, 600, seed=0), mode)
    finally:
        sc.close()


@pytest.mark.parametrize("family,patch", [("owlvit", 16), ("owlv2", None)])
def test_equal_bits_b16_and_owlv2_at_the_smallest_input(family, patch):
    sc = _scorer("f32x3", family, patch, (16, 16))
    try:
        assert sc.num_patches == 1
        _both_lanes(sc, _images(3, 40, 56, seed=0), f"{family}/16", objectness=family == "owlv2", must_keep=False)
    finally:
        sc.close()


def test_a_larger_grid_is_refused_and_nothing_is_launched():
    from tstar_amd import _lib
    lib = _lib.load()
    sc = _scorer("f32")
    try:
        imgs = _images(1, 190, 400, seed=1)
        npatch = sc.num_patches

        def filled(shape, dtype):
            return torch.full(shape, -12345, dtype=dtype, device="cuda")
        scores, labels = filled((1, npatch), torch.float32), filled((1, npatch), torch.int32)
        conf, mask, kept = filled((1, 4), torch.float64), filled((1, 4), torch.int32), filled((1,), torch.int32)
        for rows, cols in ((2, 2), (1, 2), (4, 1)):
            rc = lib.tstar_owl_score_cells(sc._h, 0, imgs.data_ptr(), 1, 190, 400, rows, cols, None, scores.data_ptr(), labels.data_ptr(),
                                           conf.data_ptr(), mask.data_ptr(), kept.data_ptr(), None, None, _lib.stream_ptr())
            assert rc == 1 and b"1x1 grid" in lib.tstar_last_error(), (rc, lib.tstar_last_error())
        torch.cuda.synchronize()
        for t in (scores, labels, conf, mask, kept):
            assert bool((t == -12345).all()), "a refused call wrote an output"
        with pytest.raises(ValueError, match="1x1 grid"):
            sc.score(imgs, 2, 2, boxes=False)
        # the null checks of the new entry; the full entry still asks for its boxes
        rc = lib.tstar_owl_score_cells(sc._h, 0, imgs.data_ptr(), 1, 190, 400, 1, 1, None, None, labels.data_ptr(), conf.data_ptr(), mask.data_ptr(),
                                       kept.data_ptr(), None, None, _lib.stream_ptr())
        assert rc == 1 and b"null argument" in lib.tstar_last_error()
        rc = lib.tstar_owl_score_lane_obj(sc._h, 0, imgs.data_ptr(), 1, 190, 400, 1, 1, None, scores.data_ptr(), labels.data_ptr(), None, conf.data_ptr(),
                                          mask.data_ptr(), kept.data_ptr(), None, None, None, _lib.stream_ptr())
        assert rc == 1 and b"null argument" in lib.tstar_last_error()
    finally:
        sc.close()


class _ScoreSpy:
    """Counts the forwards of an OWLInterface's scorer by (grid cells, boxes) WITHOUT replacing ``score_batch`` (a wrapper there keeps
    getting boxes: tstar_amd.interface_searcher.verify_score_kwargs)."""

    def __init__(self, h):
        self.seen = []
        orig = h.scorer.score

        def score(images, rows, cols, *a, **kw):
            self.seen.append((rows * cols, bool(kw.get("boxes", True))))
            return orig(images, rows, cols, *a, **kw)
        h.scorer.score = score

    def verify_boxes(self):
        return {b for cells, b in self.seen if cells == 1}

    def grid_boxes(self):
        return {b for cells, b in self.seen if cells > 1}


@pytest.fixture(scope="module")
def x3_interface():
    from tstar_amd.interface_heuristic import OWLInterface
    return OWLInterface(synthetic_seed=0, max_batch=32, weights_dtype="f32x3")


def _search_record(s, frames, ts):
    return dict(frames=frames, ts=list(ts), sd=np.array(s.score_distribution), P=list(s.P_history[-1]), frames_scored=s.frames_scored,
                detector_calls=s.detector_calls)


def _assert_same_search(a, b):
    assert a["ts"] == b["ts"] and np.array_equal(a["frames"], b["frames"])
    assert np.array_equal(a["sd"], b["sd"]) and a["P"] == b["P"]
    assert (a["frames_scored"], a["detector_calls"]) == (b["frames_scored"], b["detector_calls"])


def test_search_without_visual_history_equals_the_search_with_one(x3_interface):
    """The small f32x3 search of tests/test_gpu_searcher.py (N = 900, g = 6): keep_visual_history=False scores its verification
    frames without boxes, True with them; everything the search returns and counts is equal."""
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    h = x3_interface
    N, g, K, seed = 900, 6, 6, 11
    store = synthetic_video(N, seed=6)
    runs = {}
    for keep in (False, True):
        spy = _ScoreSpy(h)
        try:
            s = TStarSearcher(store, h, ["couch"], ["tv", "chair"], search_nframes=K, image_grid_shape=(g, g), search_budget=0.3,
                              confidence_threshold=0.6, rng=np.random.RandomState(seed), keep_visual_history=keep)
            frames, ts = s.search()
        finally:
            del h.scorer.score
        assert spy.verify_boxes() == {keep} and spy.grid_boxes() == {True}, spy.seen
        runs[keep] = _search_record(s, frames, ts)
        if keep:
            assert len(s.detect_bbox_iters) > 0
    _assert_same_search(runs[False], runs[True])


def test_lockstep_group_without_visual_history_equals_the_group_with_one(x3_interface):
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.lockstep import search_lockstep_groups
    from tstar_amd.video import synthetic_video
    h = x3_interface
    N, g, K = 900, 6, 6
    stores = [synthetic_video(N, seed=6), synthetic_video(N, seed=7)]
    questions = [(["couch"], ["tv", "chair"]), (["dog", "lamp"], ["road"])]
    runs = {}
    for keep in (False, True):
        spy = _ScoreSpy(h)
        try:
            group = [TStarSearcher(stores[i], h, list(questions[i][0]), list(questions[i][1]), search_nframes=K, image_grid_shape=(g, g),
                                   search_budget=0.3, confidence_threshold=0.6, rng=np.random.RandomState(11 + i), keep_visual_history=keep)
                     for i in range(2)]
            res = search_lockstep_groups([group])[0]
        finally:
            del h.scorer.score
        assert spy.verify_boxes() == {keep} and spy.grid_boxes() == {True}, spy.seen
        runs[keep] = [_search_record(s, fr, ts) for s, (fr, ts) in zip(group, res)]
    for a, b in zip(runs[False], runs[True]):
        _assert_same_search(a, b)


def test_boxes_of_a_result_without_boxes_raise(x3_interface):
    from tstar_amd.interface_heuristic import NO_BOXES_ERROR
    h = x3_interface
    h.reparameterize_object_list(["couch"], ["tv"])
    imgs = _images(2, 285, 600, seed=2)
    r = h.score_batch(imgs, 1, 1, boxes=False)
    assert r.boxes is None and r.cell_conf.shape == (2, 1)
    with pytest.raises(ValueError, match="boxes=False") as e:
        h.annotated_batch(imgs, r)
    assert NO_BOXES_ERROR in str(e.value)
    with pytest.raises(ValueError, match="boxes=False"):
        h._detections_from(r, 0)
    imgs_after = imgs.clone()
    full = h.score_batch(imgs, 1, 1)                                   # the default is unchanged: boxes, drawable
    painted, dets = h.annotated_batch(imgs_after, full)
    assert painted.shape == (2, 285, 600, 3) and len(dets) == 2 and full.boxes.shape == (2, h.scorer.num_patches, 4)
