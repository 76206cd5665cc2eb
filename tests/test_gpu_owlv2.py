"""OWLv2 B/16 on the HIP detector path.

* pre-processing (both kernel forms) against HF's own ``Owlv2ImageProcessorPil``, bit for bit, B = 2 with different images;
* an HF-initialised OWLv2 checkpoint through ``OWLInterface(model_name_or_path=dir)`` against HF's CPU forward and HF's own
  post-processing, at three small input sizes in all four weight modes and at the default 960 x 960 in f32 / f32x3;
* chunking, lanes and ``objectness=True`` change no bit; searches on a synthetic OWLv2 heuristic at (320, 320);
* refusals, and OWL-ViT B/16 at (960, 960) keeps the bits recorded before this feature (tests/golden/owlvit_b16_960_crc.txt)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import owlv2_util as U

pytestmark = pytest.mark.gpu

_SD = {}


def _vision_sd():
    from tstar_amd import weights as W
    if "v" not in _SD:
        _SD["v"] = W.synthetic_state_dict(0, "vision", geometry=W.OWLV2_B16)
    return _SD["v"]


def _both_sd():
    from tstar_amd import weights as W
    if "b" not in _SD:
        _SD["b"] = dict(_vision_sd(), **W.synthetic_state_dict(0, "text", geometry=W.OWLV2_B16))
    return _SD["b"]


def _vision_scorer(size, max_batch=2):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    g = W.with_input_size(W.OWLV2_B16, size)
    return OwlScorer(W.pack_blob(_vision_sd(), W.vision_spec(g), g), None, max_batch=max_batch, input_size=size, family="owlv2")


def _plan_form(H, Wd, size):
    from tstar_amd import _lib
    p = (C.c_int * 10)()
    _lib.check(_lib.load().tstar_owlv2_preprocess_plan(H, Wd, size[0], size[1], p))
    return p[0]


# ------------------------------------------------------------------------------------------------------------ pre-processing
# (source, target, form): an upscale with H > W (mirror at the first output pixels); a mild shrink; both axes filtered at odd
# extents (windows crossing the image edge and the square's edge); one identity axis; the two production shapes
PRE_CASES = [((37, 23), (64, 64), 0), ((95, 200), (96, 64), 1), ((97, 301), (64, 96), 1), ((600, 600), (480, 960), 1),
             ((285, 600), (960, 960), 0), ((1520, 3200), (960, 960), 1)]


def _check_preprocess(s, imgs, size):
    gh, gw = size[0] // 16, size[1] // 16
    B = imgs.shape[0]
    u8, pat = s.debug_preprocess(torch.from_numpy(imgs).cuda())
    torch.cuda.synchronize()
    assert u8 is None and pat.shape == (B * gh * gw, 768)
    pat = pat.cpu().numpy().reshape(B, gh * gw, 768)
    for b in range(B):
        want = U.im2col(U.hf_pixels(imgs[b], size))
        bad = int((pat[b].view(np.uint32) != want.view(np.uint32)).sum())
        assert bad == 0, (b, bad, float(np.abs(pat[b] - want).max()))


@pytest.mark.parametrize("src,size,form", PRE_CASES)
def test_preprocess_is_hfs_processor_bit_for_bit(src, size, form):
    H, Wd = src
    rs = np.random.RandomState(H * 7 + Wd + size[0])
    imgs = rs.randint(0, 256, (2, H, Wd, 3)).astype(np.uint8)
    imgs[1] = imgs[1] // 2 + 20                        # other clip bounds than image 0: (20 .. 147) against (0 .. 255)
    imgs[1, -1, :, :] = 255                            # an all-255 last row and column next to the zero border
    imgs[1, :, -1, :] = 255
    assert _plan_form(H, Wd, size) == form
    s = _vision_scorer(size)
    assert s.num_patches == (size[0] // 16) * (size[1] // 16) and s.preprocess_form() == -1
    _check_preprocess(s, imgs, size)
    assert s.preprocess_form() == form
    s.close()


@pytest.mark.parametrize("src,size", [((37, 23), (64, 64)), ((95, 200), (96, 64)), ((131, 131), (64, 96)), ((40, 40), (64, 64))])
def test_preprocess_clip_bounds_per_image(src, size):
    """A constant-255 image beside a dark one (maximum 90) and, for the square sources, a bright one whose minimum is not 0:
    each image is clipped to its OWN bounds, in both forms."""
    H, Wd = src
    rs = np.random.RandomState(H + Wd)
    imgs = np.empty((3, H, Wd, 3), np.uint8)
    imgs[0] = 255
    imgs[1] = rs.randint(0, 91, (H, Wd, 3))
    imgs[2] = rs.randint(100, 256, (H, Wd, 3))
    s = _vision_scorer(size, max_batch=3)
    _check_preprocess(s, imgs, size)
    s.close()


# --------------------------------------------------------------------------------------------------------- checkpoint parity
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from transformers import CLIPTokenizer
    d = str(tmp_path_factory.mktemp("owlv2_b16_ckpt"))
    m = U.make_checkpoint_dir(d, seed=2)
    return d, m, CLIPTokenizer.from_pretrained(d, local_files_only=True)


def _test_images():
    from oracle import resize_ref as R
    from tstar_amd.video import synthetic_frames_numpy
    return [R.cv_bilinear_resize(synthetic_frames_numpy([7 + k], 40, 360, 640, seed=5)[0], W_, H_)
            for k, (H_, W_) in enumerate([(285, 600), (400, 190)])]


_REF = {}
PARITY = [((64, 96), m) for m in ("f32", "f32x3", "bf16", "bf16_exact")] + [((160, 160), m) for m in ("f32", "f32x3", "bf16", "bf16_exact")] + \
         [((320, 480), m) for m in ("f32", "f32x3", "bf16", "bf16_exact")] + [(None, "f32"), (None, "f32x3")]


@pytest.mark.parametrize("size,mode", PARITY)
def test_checkpoint_matches_hf(ckpt, size, mode):
    """tests/test_gpu_owl_input_size.py::test_checkpoint_matches_hf_at_input_size for OWLv2, with its bounds: text embeds 1e-5,
    dense and kept scores 1e-3, boxes 1e-2 px against HF's ``post_process_object_detection(target_sizes=[(H, W)])`` (boxes scaled
    by max(H, W): a (W, H) scale fails on the 285 x 600 frame), unsaturated reference; ``objectness_logits`` within 2e-4 in f32 /
    f32x3 (the project's logits bound) and 1e-3 in the bf16 modes.  T = 25, 101, 601 and, at the default size, 3601
    (one image).  The bf16 modes compare against HF on ``round_weights_to_bf16`` weights."""
    from tstar_amd import weights as W
    from tstar_amd.interface_heuristic import OWLInterface
    d, m, tok = ckpt
    h = OWLInterface(model_name_or_path=d, max_batch=2, weights_dtype=mode, input_size=size)
    run = size or (960, 960)
    np_ = (run[0] // 16) * (run[1] // 16)
    assert h.geometry == W.with_input_size(W.OWLV2_B16, size) and h.family == "owlv2" and h.scorer.num_patches == np_
    h.reparameterize_object_list(["couch"], ["tv", "remote control"])
    names = [t[0] for t in h.texts]
    ref_model = m
    if mode in ("bf16", "bf16_exact"):
        ref_model = _REF.get("bf16_model")
        if ref_model is None:
            sd = W.round_weights_to_bf16({k: v.numpy() for k, v in m.state_dict().items()})
            ref_model = copy.deepcopy(m)
            ref_model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            _REF["bf16_model"] = ref_model
    wkey = "bf16" if mode.startswith("bf16") else "f32"
    obj_bound = 1e-3 if wkey == "bf16" else 2e-4
    for k, img in enumerate(_test_images()[:1 if size is None else 2]):
        H_, W_ = img.shape[:2]
        key = (wkey, run, k)
        if key not in _REF:
            _REF[key] = U.hf_detect_at(ref_model, tok, img, names, run)
        ref = _REF[key]
        if k == 0:
            assert np.abs(h.scorer.get_query_embeds() - ref["text_embeds"]).max() < 1e-5
        det = h.inference_detector([img])[0]
        r = h.scorer.score(torch.from_numpy(img).cuda().unsqueeze(0), 1, 1, objectness=True)
        dense = r.scores[0].cpu().numpy()
        err = float(np.abs(dense - ref["dense_scores"]).max())
        assert 0.05 < ref["dense_scores"].min() and ref["dense_scores"].max() < 0.95       # not a saturated comparison
        assert len(det) == len(ref["scores"]) == np_                      # threshold 0.005: every patch kept, patch order
        kept_err = float(np.abs(det.confidence - ref["scores"]).max())
        box_err = float(np.abs(det.xyxy - ref["xyxy"]).max())
        wh = ref["xyxy"][:, 2:] - ref["xyxy"][:, :2]
        assert wh.min() > 1.0 and wh.max() < max(H_, W_)                # real boxes, not saturated sigmoids
        obj = r.objectness[0].cpu().numpy()
        obj_err = float(np.abs(obj - ref["objectness"]).max())
        print(f"OWLv2 at {run[0]}x{run[1]} {mode} {H_}x{W_}: max |score - HF| = {err:.2e}, max |box - HF| = {box_err:.2e} px, "
              f"max |objectness - HF| = {obj_err:.2e} (|objectness| up to {np.abs(ref['objectness']).max():.2f})")
        assert err < 1e-3 and kept_err < 1e-3, (err, kept_err)
        assert box_err < 1e-2, box_err
        assert np.abs(ref["objectness"]).max() < 50 and ref["objectness"].std() > 1e-3      # O(1) logits that vary
        assert obj_err < obj_bound, obj_err
    del h


# --------------------------------------------------------------------------------------------- chunking, lanes, objectness
def _queries():
    from tstar_amd.tokenizer import encode_queries
    ids, am = encode_queries([["couch"], ["tv"], ["chair"], [" "]], "google/owlv2-base-patch16", allow_standin=True)
    return ids, am, [1.0, 0.5, 0.5, 0.5]


def _synthetic(max_batch, mode="f32", size=None):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    g = W.with_input_size(W.OWLV2_B16, size)
    sd = _both_sd()
    s = OwlScorer(W.pack_blob(sd, W.vision_spec(g), g), W.pack_blob(sd, W.text_spec(g)), max_batch=max_batch, weights_mode=mode,
                  input_size=size, family="owlv2")
    s.set_queries(*_queries())
    return s


FIELDS = ("scores", "labels", "boxes", "cell_conf", "cell_mask", "n_kept")


def _fields(r, b):
    return {f: getattr(r, f)[b].cpu().numpy() for f in FIELDS}


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_chunking_lanes_and_objectness_are_bit_identical(mode):
    """(160, 160), T = 101: B = 5 through a max_batch 2 handle (chunks of 2, 2, 1; the filtered form on 190 x 400 frames) gives
    the bits of one image at a time; lane 1 gives lane 0's bits, alone and while lane 0 runs on another stream; asking for the
    objectness logits changes no other output and gives the same logits in a batch and alone."""
    rs = np.random.RandomState(11)
    imgs = torch.from_numpy(rs.randint(0, 256, (5, 190, 400, 3)).astype(np.uint8)).cuda()
    s = _synthetic(2, mode, (160, 160))
    assert s.num_patches == 100
    batch = s.score(imgs, 2, 3)
    torch.cuda.synchronize()
    with_obj = s.score(imgs, 2, 3, objectness=True, want_logits=True)
    lane1 = s.score(imgs, 2, 3, lane=1)
    torch.cuda.synchronize()
    assert batch.objectness is None and with_obj.objectness.shape == (5, 100)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        both1 = s.score(imgs, 2, 3, lane=1)
    both0 = s.score(imgs, 2, 3, lane=0)
    torch.cuda.synchronize()
    for b in range(5):
        r = s.score(imgs[b:b + 1], 2, 3, objectness=True)
        torch.cuda.synchronize()
        one = _fields(r, 0)
        for name, got in (("batch", batch), ("objectness", with_obj), ("lane 1", lane1), ("lane 1 beside lane 0", both1),
                          ("lane 0 beside lane 1", both0)):
            g = _fields(got, b)
            for f in one:
                assert np.array_equal(g[f], one[f]), (mode, name, b, f)
        assert torch.equal(with_obj.objectness[b], r.objectness[0]), (mode, b)
    assert int(batch.n_kept[0]) > 0 and torch.isfinite(with_obj.objectness).all()
    s.close()


# -------------------------------------------------------------------------------------------------------------------- search
def _heuristic(**kw):
    from tstar_amd.interface_heuristic import OWLInterface
    return OWLInterface(model_name_or_path="google/owlv2-base-patch16-ensemble", synthetic_seed=0, input_size=(320, 320), **kw)


def test_search_teacher_forced_and_painter_at_owlv2():
    """tests/test_gpu_owl_input_size.py::test_search_teacher_forced_and_painter_at_448x768 on a synthetic OWLv2 heuristic at
    (320, 320): 400 detections per image, a 160-frame video, a 4 x 4 grid."""
    from oracle import searcher_ref as S
    from oracle.replay import Recorder, replay_through_oracle
    from tstar_amd import _lib
    from tstar_amd.interface_heuristic import Detections, draw_boxes
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    N, g, K, seed = 160, 4, 4, 2025
    h = _heuristic(max_batch=16)
    assert h.family == "owlv2" and h.geometry.npatch == 400 and _lib.load().tstar_owl_num_patches(h.scorer._h) == 400
    rec = Recorder(h)
    s = TStarSearcher(synthetic_video(N, seed=3), h, ["couch"], ["tv", "chair"], search_nframes=K, image_grid_shape=(g, g),
                      search_budget=0.5, confidence_threshold=0.6, rng=np.random.RandomState(seed), keep_visual_history=True)
    frames, ts = s.search()
    assert len(ts) == K
    ref, ts_ref = replay_through_oracle(rec.calls, h.texts, ["couch"], ["tv", "chair"], N, g, K, 0.5, 0.6, seed)
    assert ts_ref == [float(t) for t in ts]
    for i in range(s.iterations):
        assert np.array_equal(np.asarray(s.Score_history[i]), ref.Score_history[i])
        assert np.array_equal(np.asarray(s.non_visiting_history[i]), ref.unvisited_history[i])
        assert np.array_equal(np.asarray(s.P_history[i]), ref.P_history[i])
    first = rec.calls[0]
    assert first["rows"] == g and first["scores"].shape == (1, 400)
    texts = [list(t) for t in h.texts]
    o2w = {"couch": 1.0, "tv": 0.5, "chair": 0.5}
    keep = first["scores"][0] > np.float32(0.005)
    Hg, Wg = first["images"][0].shape[:2]
    cm, _ = S.image_grid_score(first["boxes"][0][keep], first["labels"][0][keep], first["scores"][0][keep], texts, o2w, Hg, Wg, g, g)
    assert np.array_equal(first["conf"][0].reshape(g, g), cm)
    det = Detections(xyxy=first["boxes"][0][keep], confidence=first["scores"][0][keep], class_id=first["labels"][0][keep].astype(np.int64))
    host = draw_boxes(first["images"][0].copy(), det)
    assert len(s.detect_bbox_iters[0][0]) == int(keep.sum())
    assert np.array_equal(s.detect_annotot_iters[0][0], host)
    assert not np.array_equal(host, first["images"][0])


def _make_searcher(h, store, targets, cues, k, seed, thr=0.6):
    from tstar_amd.interface_searcher import TStarSearcher
    return TStarSearcher(store, h, list(targets), list(cues), search_nframes=k, image_grid_shape=(4, 4), search_budget=0.5,
                         confidence_threshold=thr, rng=np.random.RandomState(seed), keep_visual_history=False)


def test_solo_and_lockstep_searches_at_owlv2(monkeypatch):
    """The statements of test_solo_search_equals_the_sequential_loop_at_448x768 and
    test_lockstep_group_of_three_equals_solo_at_448x768 on one synthetic OWLv2 heuristic (f32x3, 160-frame videos, 4 x 4)."""
    from tstar_amd.lockstep import search_lockstep
    from tstar_amd.video import synthetic_video
    h = _heuristic(max_batch=16, weights_dtype="f32x3")
    stores = [synthetic_video(160, seed=31), synthetic_video(160, seed=32), synthetic_video(160, seed=33)]
    items = [(["couch"], ["tv"], 4), (["dog", "lamp"], [], 3), (["tv"], ["chair", "couch"], 4)]

    def make(i, thr=0.6):
        t, c, k = items[i]
        return _make_searcher(h, stores[i], t, c, k, 70 + i, thr)

    for thr in (0.05, 0.6):
        res = []
        for sequential in (False, True):
            if sequential:
                monkeypatch.setenv("TSTAR_SOLO_SEQUENTIAL", "1")
            else:
                monkeypatch.delenv("TSTAR_SOLO_SEQUENTIAL", raising=False)
            s = make(0, thr)
            frames, ts = s.search()
            res.append((frames, ts, np.asarray(s.score_distribution), s.iterations, s.frames_scored,
                        [np.asarray(x) for x in s.Score_history], [np.asarray(x) for x in s.P_history]))
        a, b = res
        assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[3:5] == b[3:5]
        assert len(a[5]) == len(b[5]) and all(np.array_equal(x, y) for x, y in zip(a[5], b[5]))
        assert all(np.array_equal(x, y) for x, y in zip(a[6], b[6]))
    monkeypatch.delenv("TSTAR_SOLO_SEQUENTIAL", raising=False)
    solo = []
    for i in range(3):
        s = make(i)
        fr, ts = s.search()
        solo.append((fr, ts, s.score_distribution))
    group = [make(i) for i in range(3)]
    res = search_lockstep(group)
    for i in range(3):
        assert res[i][1] == solo[i][1] and np.array_equal(res[i][0], solo[i][0])
        assert np.array_equal(group[i].score_distribution, solo[i][2])


# ------------------------------------------------------------------------------------------------- refusals, no regression
def test_refusals(monkeypatch):
    from tstar_amd import _lib
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.owl import OwlScorer
    monkeypatch.delenv("TSTAR_OWL_FAMILY", raising=False)
    monkeypatch.delenv("TSTAR_SYNTHETIC_SEED", raising=False)
    img = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (1, 64, 96, 3)).astype(np.uint8)).cuda()
    vit = OwlScorer.synthetic(0, max_batch=1, patch_size=16, input_size=(64, 96))
    vit.set_queries(*_queries())
    with pytest.raises(ValueError, match="objectness"):
        vit.score(img, 1, 1, objectness=True)
    r = vit.score(img, 1, 1)
    obj = torch.zeros((1, vit.num_patches), device="cuda")
    lib = _lib.load()
    rc = lib.tstar_owl_score_lane_obj(vit._h, 0, img.data_ptr(), 1, 64, 96, 1, 1, None, r.scores.data_ptr(), r.labels.data_ptr(), r.boxes.data_ptr(),
                                      r.cell_conf.data_ptr(), r.cell_mask.data_ptr(), r.n_kept.data_ptr(), None, None, obj.data_ptr(),
                                      _lib.stream_ptr())
    assert rc == 1 and b"OWLv2" in lib.tstar_last_error()
    vit.close()
    s = _synthetic(1, "f32", (64, 96))
    u8 = torch.zeros((1, 64, 96, 3), dtype=torch.uint8, device="cuda")
    pat = torch.zeros((24, 768), device="cuda")
    rc = lib.tstar_owl_debug_preprocess(s._h, img.data_ptr(), 1, 64, 96, u8.data_ptr(), pat.data_ptr(), _lib.stream_ptr())
    assert rc == 1 and b"u8" in lib.tstar_last_error()
    huge = torch.zeros((1, 8, 4320, 3), dtype=torch.uint8, device="cuda")      # 4320 -> 64: the window of one pixel does not fit LDS
    with pytest.raises(_lib.TStarHipError, match="LDS"):
        s.score(huge, 1, 1)
    s.close()
    with pytest.raises(ValueError, match="owlv2"):
        OwlScorer(None, np.zeros(4, np.float32), family="owlv2", patch_size=32)
    with pytest.raises(ValueError, match="family"):
        OWLInterface(synthetic_seed=0, family="owlv3")
    with pytest.raises(FileNotFoundError, match="owlv2"):
        OWLInterface(model_name_or_path="google/owlv2-base-patch16")
    monkeypatch.setenv("TSTAR_OWL_FAMILY", "owlv2")
    h = OWLInterface(synthetic_seed=0, max_batch=1, input_size=(64, 96))
    assert h.family == "owlv2" and h.geometry.npatch == 24
    h2 = OWLInterface(synthetic_seed=0, max_batch=1, input_size=(64, 96), family="owlvit", patch_size=16)     # the keyword wins
    assert h2.family == "owlvit"


def test_owlvit_b16_at_960_keeps_the_parents_bits():
    got, want = U.b16_960_crcs(), U.read_b16_960_golden()
    assert set(want) == set(U.B16_960_MODES)
    assert got == want, U.format_b16_960(got)
