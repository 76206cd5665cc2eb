"""Image-guided (one-shot) queries on the HIP detector path.

* the selection kernel through ``tstar_image_query_select`` on the crafted cases of tests/image_query_util.py (np at the wave
  edges and at the largest grid, n = 1, 2, 5, NaN behind the last image, sentinels behind the outputs) against the numpy
  restatement that tests/test_image_query_host.py pins to HF's statements;
* HF-initialised B/32, B/16 and OWLv2 B/16 checkpoints through ``OWLInterface`` against HF's own
  ``image_guided_detection`` / ``embed_image_query`` on the CPU;
* the Python surface on synthetic weights: mixed text / image query sets, the three ways of installing them, searches.

tools/measure_image_query.py records the same deviations, with timings, in profiles/image_query_measure.md."""
import numpy as np
import pytest
import torch

import image_query_util as U

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_I = np.float32(-77.25), np.int32(-12345)


# ------------------------------------------------------------------------------------------------------------ the kernel
def _select(cls_list, boxes_list, np_):
    """``tstar_image_query_select`` on the images of the lists, laid out as one [n * np] block with 64 rows of NaN behind the last
    image; the host outputs have one entry more than n, filled with a sentinel."""
    from tstar_amd import _lib
    lib = _lib.load()
    n = len(cls_list)
    cls = torch.full((n * np_ + 64, U.PROJ), float("nan"), device="cuda")
    boxes = torch.full((n * np_ + 64, 4), float("nan"), device="cuda")
    cls[:n * np_] = torch.from_numpy(np.concatenate(cls_list)).cuda()
    boxes[:n * np_] = torch.from_numpy(np.concatenate(boxes_list)).cuda()
    emb = np.full((n + 1, U.PROJ), SENTINEL_F, np.float32)
    box = np.full((n + 1, 4), SENTINEL_F, np.float32)
    best, nsel, status = (np.full(n + 1, SENTINEL_I, np.int32) for _ in range(3))
    rc = lib.tstar_image_query_select(cls.data_ptr(), boxes.data_ptr(), n, np_, emb.ctypes.data, best.ctypes.data, box.ctypes.data,
                                      nsel.ctypes.data, status.ctypes.data, _lib.stream_ptr())
    _lib.check(rc, "tstar_image_query_select")
    assert np.all(emb[n] == SENTINEL_F) and np.all(box[n] == SENTINEL_F)
    assert best[n] == nsel[n] == status[n] == SENTINEL_I
    return emb[:n], best[:n], box[:n], nsel[:n], status[:n]


_CASES = {}


def _cases(np_):
    """[(label, cls, boxes, restatement's result)] of one np, built and evaluated once for the three n."""
    if np_ not in _CASES:
        built = []
        for label, cls, boxes, exp in U.build_cases(np_):
            r = U.select(cls, boxes)
            assert (r["status"], r["n_selected"], r["best"]) == (exp["status"], exp["n_selected"], exp["best"]), (np_, label)
            if r["n_selected"] > 1:            # the planted gap: 64 x the error bound on mean_sim (owl_tail_util.bound's rule)
                b = U.mean_sim_bound(cls, r["selected"])
                assert r["gap"] >= 64 * b, (np_, label, r["gap"], b)
            built.append((label, cls, boxes, r))
        _CASES[np_] = built
    return _CASES[np_]


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("np_", U.CASE_NP)
def test_selection_kernel_on_crafted_cases(np_, n):
    """Every numbered case that np rows can hold, n images per call (the case list in calls of n, wrapping round: the images of
    one call are different cases, or the same boxes with the minimum planted elsewhere).  Exact: status, selected count, best
    index (every case plants its minimum with a gap of at least 64 x the error bound), the box and the embedding row's bits."""
    cases = _cases(np_)
    calls = [[(k + j) % len(cases) for j in range(n)] for k in range(0, len(cases), n)]
    for call in calls:
        assert n > len(cases) or len(set(call)) == n
        emb, best, box, nsel, status = _select([cases[i][1] for i in call], [cases[i][2] for i in call], np_)
        for j, i in enumerate(call):
            label, cls, boxes, r = cases[i]
            where = (np_, n, label)
            assert status[j] == r["status"], where
            assert nsel[j] == r["n_selected"], where
            assert best[j] == r["best"], where
            if r["best"] < 0:
                assert not emb[j].view(np.uint32).any() and not box[j].view(np.uint32).any(), where
            else:
                assert np.array_equal(emb[j].view(np.uint32), cls[r["best"]].view(np.uint32)), where
                assert np.array_equal(box[j].view(np.uint32), boxes[r["best"]].view(np.uint32)), where


def test_selection_refuses_bad_arguments():
    from tstar_amd import _lib
    lib = _lib.load()
    cls, boxes = torch.zeros((4, U.PROJ), device="cuda"), torch.zeros((4, 4), device="cuda")
    emb, box = np.full((1, U.PROJ), SENTINEL_F, np.float32), np.full((1, 4), SENTINEL_F, np.float32)
    ints = [np.full(1, SENTINEL_I, np.int32) for _ in range(3)]

    def call(c=cls.data_ptr(), b=boxes.data_ptr(), n=1, np_=4, e=emb.ctypes.data):
        return lib.tstar_image_query_select(c, b, n, np_, e, ints[0].ctypes.data, box.ctypes.data, ints[1].ctypes.data, ints[2].ctypes.data,
                                            _lib.stream_ptr())

    for kw in (dict(c=None), dict(b=None), dict(e=None), dict(n=0), dict(np_=0), dict(np_=3601), dict(c=cls.data_ptr() + 4)):
        assert call(**kw) == 1, kw
        assert lib.tstar_last_error()
    assert np.all(emb == SENTINEL_F) and np.all(box == SENTINEL_F) and all(v[0] == SENTINEL_I for v in ints)
    assert call() == 0


# -------------------------------------------------------------------------------------------------- end to end against HF
@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    out = {}
    for g in U.GEOMETRIES:
        d = str(tmp_path_factory.mktemp(f"image_query_{g}"))
        out[g] = (d, U.make_checkpoint(g, d))
    return out


_REF = {}


@pytest.mark.parametrize("g,mode", U.E2E_CASES)
def test_checkpoint_image_guided_matches_hf(ckpts, g, mode):
    """Two example images and two target images (target b against example b) through an HF-initialised checkpoint, against HF's
    ``image_guided_detection(..., interpolate_pos_encoding=True)`` on pixels from HF's own processor.  HF's own margins are
    asserted first (threshold margin >= 1e-3 relative for every patch, mean_sim gap >= 1e-3 of the largest |mean_sim|); then: the
    best index equals HF's, the query box is ``score(...).boxes_cxcywh[best]`` of the same image bit for bit, the normalised
    embedding within 1e-5, sigmoid(logit) of the image query within 1e-3, target boxes within 1e-2 px (bf16: against HF on the
    rounded weights, same bounds, as tests/test_gpu_owl_input_size.py).  The observed maxima are printed
    (tools/measure_image_query.py writes them to profiles/image_query_measure.md)."""
    from tstar_amd.interface_heuristic import OWLInterface
    family, patch, size = U.GEOMETRIES[g]
    d, model = ckpts[g]
    ref = U.reference_for(g, model, "bf16" if mode == "bf16" else "f32", _REF)
    margin, gap = U.assert_hf_margins(ref)
    assert 0.05 < ref["probs"].min() and ref["probs"].max() < 0.95                 # not a saturated comparison
    h = OWLInterface(model_name_or_path=d, max_batch=2, weights_dtype=mode, input_size=size)
    assert h.family == family and h.scorer.num_patches == (size[0] // patch) * (size[1] // patch)
    dev = U.device_image_guided(h, g, ref)
    r = dev["result"]
    print(f"{g} {size[0]}x{size[1]} {mode}: HF threshold margin {margin:.2e}, mean_sim gap {gap:.2e}; max |qn - HF| = {dev['emb_err']:.2e}, "
          f"max |sigmoid(logit) - HF| = {dev['prob_err']:.2e}, max |box - HF| = {dev['box_err']:.2e} px")
    for b, p in enumerate(ref["per_image"]):
        assert r.status[b] == (1 if p["used_giou"] else 0) and r.n_selected[b] == int(p["selected"].sum()), b
        assert r.best[b] == p["best"], (b, r.best[b], p["best"])
    assert dev["query_boxes_are_the_scorers_bits"]
    assert dev["emb_err"] < 1e-5, dev["emb_err"]
    assert dev["prob_err"] < 1e-3, dev["prob_err"]
    assert dev["box_err"] < 1e-2, dev["box_err"]
    del h


# ---------------------------------------------------------------------------------------------------------- the surface
SIZE = (160, 224)                                     # B/32: 35 patches


@pytest.fixture(scope="module")
def heur():
    from tstar_amd.interface_heuristic import OWLInterface
    return OWLInterface(synthetic_seed=0, max_batch=16, input_size=SIZE)


def _logits(h, imgs, slot=0):
    r = h.scorer.score(imgs, 1, 1, want_logits=True, image_sets=[slot] * imgs.shape[0])
    torch.cuda.synchronize()
    return r.logits.cpu().numpy()


def test_mixed_set_and_the_three_installs(heur):
    """Two text names, one image-backed name and the blank: the text columns' logits and raw rows are the all-text install's
    bits, the image column is a manual ``set_query_embeds`` install of the returned embedding, and the lazily installed slot 0,
    ``install_queries`` and ``install_queries_many`` give identical slots; ``clear_query_images`` restores the text bits."""
    h = heur
    h.clear_query_images()
    example, targets = U.query_and_target_images()
    imgs = torch.from_numpy(targets).cuda()
    h.reparameterize_object_list(["couch", " mug "], ["tv"])
    assert h.texts == [["couch"], ["mug"], ["tv"], [" "]]
    text_raw, text_logits = h.scorer.get_query_embeds(0), _logits(h, imgs)
    h.set_query_images({" mug ": example[0]})
    assert list(h.query_image_info) == ["mug"]
    info = h.query_image_info["mug"]
    r = h.scorer.embed_image_queries(torch.from_numpy(example[:1]).cuda())
    assert info["best_index"] == int(r.best[0]) and info["n_selected"] == int(r.n_selected[0]) and np.array_equal(info["box_cxcywh"], r.boxes_cxcywh[0])
    assert info["giou_fallback"] == bool(r.status[0] == 1) and 0 <= info["best_index"] < h.scorer.num_patches
    # the logits of slot 0 installed before the registry changed are still the text ones: registering installs nothing
    assert np.array_equal(_logits(h, imgs), text_logits)
    h.reparameterize_object_list(["couch", " mug "], ["tv"])
    assert h.texts == [["couch"], ["mug"], ["tv"], [" "]] and 0 in h.scorer._pending               # still lazy
    mixed_logits, mixed_raw = _logits(h, imgs), h.scorer.get_query_embeds(0)
    for col in (0, 2, 3):
        assert np.array_equal(mixed_logits[..., col].view(np.uint32), text_logits[..., col].view(np.uint32)), col
        assert np.array_equal(mixed_raw[col].view(np.uint32), text_raw[col].view(np.uint32)), col
    assert np.array_equal(mixed_raw[1].view(np.uint32), r.embeds[0].view(np.uint32))
    assert not np.array_equal(mixed_logits[..., 1], text_logits[..., 1])
    manual = text_raw.copy()
    manual[1] = r.embeds[0]
    h.scorer.set_query_embeds(manual, (h._ids[:, 0] > 0).astype(np.uint8), [1.0, 1.0, 0.5, 0.5], slot=9)
    assert np.array_equal(_logits(h, imgs, 9).view(np.uint32), mixed_logits.view(np.uint32))
    assert h.install_queries(3, ["couch", " mug "], ["tv"]) == h.texts
    assert h.install_queries_many([(4, ["couch", " mug "], ["tv"], None), (5, ["mug"], [], None)]) == [h.texts, [["mug"], [" "]]]
    for slot in (3, 4):
        assert np.array_equal(h.scorer.get_query_embeds(slot).view(np.uint32), mixed_raw.view(np.uint32)), slot
        assert np.array_equal(_logits(h, imgs, slot).view(np.uint32), mixed_logits.view(np.uint32)), slot
    assert np.array_equal(h.scorer.get_query_embeds(5)[0].view(np.uint32), r.embeds[0].view(np.uint32))
    h.clear_query_images()
    h.reparameterize_object_list(["couch", " mug "], ["tv"])
    assert np.array_equal(_logits(h, imgs).view(np.uint32), text_logits.view(np.uint32))
    assert np.array_equal(h.scorer.get_query_embeds(0).view(np.uint32), text_raw.view(np.uint32))
    h.install_queries(3, ["couch", " mug "], ["tv"])
    assert np.array_equal(_logits(h, imgs, 3).view(np.uint32), text_logits.view(np.uint32))


def test_embed_image_queries_chunks_paths_and_owlv2(tmp_path):
    """n = 5 through a max_batch 2 handle (chunks of 2, 2, 1) equals one image at a time, on an OWL-ViT B/32 handle in f32 and on
    an OWLv2 handle in f32x3; installed queries are untouched; an image FILE registers like its array."""
    from PIL import Image
    from tstar_amd.interface_heuristic import OWLInterface
    imgs = U.example_images(7, 5, 90, 130)
    for kw in (dict(input_size=SIZE), dict(family="owlv2", input_size=(64, 96), weights_dtype="f32x3")):
        h = OWLInterface(synthetic_seed=0, max_batch=2, **kw)
        h.reparameterize_object_list(["couch"], ["tv"])
        before = h.scorer.get_query_embeds(0)
        d = torch.from_numpy(imgs).cuda()
        r = h.scorer.embed_image_queries(d)
        assert np.array_equal(h.scorer.get_query_embeds(0), before)
        for b in range(5):
            one = h.scorer.embed_image_queries(d[b:b + 1])
            for f in ("embeds", "best", "boxes_cxcywh", "n_selected", "status"):
                assert np.array_equal(getattr(one, f)[0], getattr(r, f)[b]), (kw, b, f)
        assert (r.status != 2).all() and (r.best >= 0).all() and (r.best < h.scorer.num_patches).all()
        path = str(tmp_path / "example.png")
        Image.fromarray(imgs[3]).save(path)
        h.set_query_images({"a": path, "b": imgs[3], "c": U.example_images(8, 1, 64, 64)[0]})
        assert np.array_equal(h._query_images["a"], r.embeds[3]) and np.array_equal(h._query_images["b"], r.embeds[3])
        assert set(h.query_image_info) == {"a", "b", "c"}
        del h


def test_empty_selection_raises_naming_the_object(heur, monkeypatch):
    from tstar_amd.owl import ImageQueryResult
    h = heur
    h.clear_query_images()

    def stub(images):
        n = images.shape[0]
        return ImageQueryResult(embeds=np.zeros((n, 512), np.float32), best=np.array([3, -1][:n], np.int32), boxes_cxcywh=np.zeros((n, 4), np.float32),
                                n_selected=np.array([2, 0][:n], np.int32), status=np.array([0, 2][:n], np.int32))

    monkeypatch.setattr(h.scorer, "embed_image_queries", stub)
    img = U.example_images(1, 1, 64, 64)[0]
    with pytest.raises(ValueError, match="'the mug'"):
        h.set_query_images({"fine": img, "the mug": img})
    assert h._query_images == {} and h.query_image_info == {}                   # nothing is registered by a refused call
    with pytest.raises(ValueError):
        h.set_query_images({"x": np.zeros((4, 4), np.uint8)})


def _searcher(h, store, targets, cues, k, seed):
    from tstar_amd.interface_searcher import TStarSearcher
    return TStarSearcher(store, h, list(targets), list(cues), search_nframes=k, image_grid_shape=(3, 3), search_budget=0.4,
                         confidence_threshold=0.6, rng=np.random.RandomState(seed), keep_visual_history=False)


def test_search_with_an_image_backed_target(heur):
    """An unchanged ``TStarSearcher`` with an image-backed target: the same keyframes solo, in a lock-step group of three items
    (two of them image-backed) and with the embedding installed by hand in slot 0."""
    from tstar_amd.lockstep import search_lockstep
    from tstar_amd.video import synthetic_video
    h = heur
    h.clear_query_images()
    example, _ = U.query_and_target_images()
    h.set_query_images({"mug": example[0], "this person": example[1]})
    stores = [synthetic_video(160, seed=31), synthetic_video(120, seed=32), synthetic_video(200, seed=33)]
    items = [(["mug"], ["tv"], 4), (["dog", "lamp"], [], 3), (["this person"], ["chair", "mug"], 5)]

    def make(i):
        t, c, k = items[i]
        return _searcher(h, stores[i], t, c, k, 70 + i)

    solo = []
    for i in range(3):
        s = make(i)
        fr, ts = s.search()
        solo.append((fr, ts, np.asarray(s.score_distribution)))
    group = [make(i) for i in range(3)]
    res = search_lockstep(group)
    for i in range(3):
        assert res[i][1] == solo[i][1] and np.array_equal(res[i][0], solo[i][0]), i
        assert np.array_equal(np.asarray(group[i].score_distribution), solo[i][2]), i
    emb = h._query_images["mug"].copy()
    h.clear_query_images()
    text = make(0)
    fr_t, ts_t = text.search()
    print("text-only search of item 0:", ts_t, "image-backed:", solo[0][1])
    s = make(0)
    raw = h.scorer.get_query_embeds(0)
    raw[0] = emb
    h.scorer.set_query_embeds(raw, (h._ids[:, 0] > 0).astype(np.uint8), h._class_weight, slot=0)
    fr, ts = s.search()
    assert ts == solo[0][1] and np.array_equal(fr, solo[0][0])
    assert np.array_equal(np.asarray(s.score_distribution), solo[0][2])
    assert not np.array_equal(np.asarray(text.score_distribution), solo[0][2])            # the example image is not the text "mug"
