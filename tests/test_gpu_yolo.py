"""YOLO-World backend (BASELINE configs[3]) on the GPU: the HIP f32-VALU detector (through the C ABI) against the CPU
oracle (oracle/yolo_ref.py) on the same seeded weights.  The oracle's parity against the REAL model is unpinned (its
source is not part of the reference tree); these tests pin the HIP path against an independent statement of the same
architecture:
  * dense per-anchor scores within 1e-3 (the north_star's per-score bound; observed ~1e-5) and boxes within 0.05 px,
  * the post-process (candidate order, class-aware NMS, top-k) BIT-EXACT when the oracle's selection is fed the GPU's
    own dense scores / boxes (teacher-forced),
  * the wrapper semantics the reference itself defines (score > 0.12, top-50, images[0], texts layout),
  * a whole T* search on the 3600-frame video replayed through the oracle searcher.
"""
import numpy as np
import pytest
import torch

import golden_util as GU

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-3


@pytest.fixture(scope="module")
def yolo():
    from tstar_amd import yolo_world as Y
    from tstar_amd.yolo import YoloDetector
    sd = Y.synthetic_state_dict(0, "l")
    det = YoloDetector(sd, "l", max_batch=2)
    rs = np.random.RandomState(0)
    txt = rs.standard_normal((4, 512)).astype(np.float32)
    txt /= np.linalg.norm(txt, axis=1, keepdims=True)
    det.set_text_feats(txt, [1.0, 0.5, 0.5, 0.5])
    return dict(det=det, sd=sd, txt=txt)


@pytest.mark.parametrize("H,W,rows,cols,B", [(380, 800, 4, 4, 3), (285, 600, 1, 1, 2), (1520, 3200, 16, 16, 1), (360, 640, 1, 1, 1), (800, 380, 4, 4, 1)])
def test_detector_vs_oracle(yolo, H, W, rows, cols, B):
    from oracle import yolo_ref as R, searcher_ref as S
    imgs = np.stack([GU.detector_test_image(50 + b, H, W) for b in range(B)])
    r = yolo["det"].detect(torch.from_numpy(imgs).cuda(), rows, cols, want_dense=True)
    torch.cuda.synchronize()
    ref = R.detect(yolo["sd"], list(imgs), yolo["txt"])
    dsc, dbx = r.dense_scores.cpu().numpy(), r.dense_boxes.cpu().numpy()
    texts = [["couch"], ["tv"], ["chair"], [" "]]
    o2w = {"couch": 1.0, "tv": 0.5, "chair": 0.5}
    for b in range(B):
        err = np.abs(dsc[b] - ref[b]["dense_scores"]).max()
        assert err < SCORE_TOL and err < 1e-4, err
        assert np.abs(dbx[b] - ref[b]["dense_boxes"]).max() < 0.05 * max(1.0, max(H, W) / 640)
        # teacher-forced post-process: the oracle's selection on the GPU's own dense outputs -> identical detections
        sel = R.select(dsc[b], dbx[b], (H, W))
        n = int(r.n_kept[b])
        assert n == len(sel["scores"]) and n > 0
        assert np.array_equal(r.scores[b, :n].cpu().numpy(), sel["scores"])
        assert np.array_equal(r.labels[b, :n].cpu().numpy(), sel["labels"])
        assert np.array_equal(r.boxes[b, :n].cpu().numpy(), sel["xyxy"])
        assert (r.labels[b, n:].cpu().numpy() == -1).all()
        # ... and against the free-running oracle: same detections unless a near-tie flipped an NMS decision
        same = len(ref[b]["scores"]) == n and np.array_equal(ref[b]["anchors"], sel["anchors"]) and np.array_equal(ref[b]["labels"], sel["labels"])
        if same:
            assert np.abs(ref[b]["scores"] - sel["scores"]).max() < 1e-4
        print(f"{H}x{W} image {b}: {n} detections, max dense score error {err:.2e}, free-running selection {'identical' if same else 'differs'}")
        # grid-cell aggregation of the <= 50 detections: the reference loop, bit-exact
        cm, names = S.image_grid_score(sel["xyxy"], sel["labels"], sel["scores"], texts, o2w, H, W, rows, cols)
        assert np.array_equal(r.cell_conf[b].cpu().numpy().reshape(rows, cols), cm)
        mask = r.cell_mask[b].cpu().numpy().astype(np.uint32)
        for cell in range(rows * cols):
            want = 0
            for nme in names[cell]:
                want |= 1 << [t[0] for t in texts].index(nme)
            assert mask[cell] == want


@pytest.mark.parametrize("thr,max_dets", [(0.0005, 300), (0.12, 300)])
def test_wide_open_wrapper_through_the_forward(yolo, thr, max_dets):
    """The public path with the wrapper's knobs at their far ends, teacher-forced against the LITERAL statement of the
    post-process (tests/yolo_post_util.py: no shortcut at the wrapper threshold or at 300).  With score_threshold = 0.0005
    every candidate of the synthetic detector passes it: more than 16384 keys, the global-memory sort of sort_nms_kernel, and
    more than 30000, the nms_pre cut, through the real forward.  max_dets = 300 is the ABI's limit."""
    import yolo_post_util as U
    from oracle import yolo_ref as R
    H, W = 380, 800
    imgs = np.stack([GU.detector_test_image(50 + b, H, W) for b in range(2)])
    r = yolo["det"].detect(torch.from_numpy(imgs).cuda(), 4, 4, score_threshold=thr, max_dets=max_dets, want_dense=True)
    torch.cuda.synchronize()
    dsc, dbx = r.dense_scores.cpu().numpy(), r.dense_boxes.cpu().numpy()
    for b in range(2):
        lit = U.literal_select(dsc[b], dbx[b], (H, W), wrapper_thr=thr, max_dets=max_dets)
        assert U.same_selection(lit, R.select(dsc[b], dbx[b], (H, W), wrapper_thr=thr, max_dets=max_dets))
        reach = U.reach(lit, thr)
        print(f"threshold {thr} image {b}: {reach}")
        if thr < 0.001:
            assert reach["candidates"] > 30000 and reach["above"] > 16384
        n = int(r.n_kept[b])
        assert n == len(lit["scores"]) and n > 50
        assert np.array_equal(r.scores[b, :n].cpu().numpy(), lit["scores"])
        assert np.array_equal(r.labels[b, :n].cpu().numpy(), lit["labels"])
        assert np.array_equal(r.boxes[b, :n].cpu().numpy(), lit["xyxy"])
        assert (r.labels[b, n:].cpu().numpy() == -1).all() and (r.scores[b, n:].cpu().numpy() == 0).all()


@pytest.mark.parametrize("scale", ["s", "m", "x", "xl"])
def test_other_model_scales(scale):
    """The layer program is data: YOLO-World-v2-S / M / X (other widths, depths, head counts -- X is what the reference's
    hard-coded config names) run through the same kernels; dense scores vs the CPU statement, selection teacher-forced."""
    from oracle import yolo_ref as R
    from tstar_amd import yolo_world as Y
    from tstar_amd.yolo import YoloDetector
    sd = Y.synthetic_state_dict(2, scale)
    det = YoloDetector(sd, scale, max_batch=1)
    rs = np.random.RandomState(7)
    txt = rs.standard_normal((5, 512)).astype(np.float32)
    txt /= np.linalg.norm(txt, axis=1, keepdims=True)
    det.set_text_feats(txt, [1.0, 1.0, 0.5, 0.5, 0.5])
    img = GU.detector_test_image(80, 285, 600)
    r = det.detect(torch.from_numpy(img).cuda().unsqueeze(0), 1, 1, want_dense=True)
    torch.cuda.synchronize()
    ref = R.detect(sd, [img], txt)[0]
    dsc, dbx = r.dense_scores[0].cpu().numpy(), r.dense_boxes[0].cpu().numpy()
    err = np.abs(dsc - ref["dense_scores"]).max()
    # the contract; S / M / L land at ~3e-7; the synthetic X has logits of magnitude 10-60, where the same relative f32
    # noise (1e-5 of the logit: two different summation orders) is ~1e-4 of a score
    assert err < SCORE_TOL, err
    assert np.median(np.abs(dsc - ref["dense_scores"])) < 2e-5
    assert np.abs(dbx - ref["dense_boxes"]).max() < 0.05
    print(f"YOLO-World-v2-{scale.upper()}: max dense score error {err:.2e}")
    sel = R.select(dsc, dbx, (285, 600))
    n = int(r.n_kept[0])
    assert n == len(sel["scores"]) and np.array_equal(r.scores[0, :n].cpu().numpy(), sel["scores"])
    assert np.array_equal(r.labels[0, :n].cpu().numpy(), sel["labels"]) and np.array_equal(r.boxes[0, :n].cpu().numpy(), sel["xyxy"])
    det.close()


@pytest.mark.parametrize("scale,batch", [("s", 3), ("m", 2)])
def test_conv_kernels_bit_identical(scale, batch):
    """The VALU convolution kernels (LDS-tiled with 128- / 64-pixel tiles, scalar-weight with 8 / 4 pixels per lane, and its
    halo-tile forms for 3x3 layers: 8 x 40 patches on the 160- / 80- / 40-wide maps, 16 x 20 patches over the row-stacked
    batch on the 20-wide maps -- with batch 3 and 2 a patch spans two images there, the zero-row case -- each with 16 or 8
    channels per wave) accumulate
    every output in the same fmaf order: a whole forward is BIT-identical whichever kernel the per-layer policy picks.
    The policy is read from the environment once per process, so each variant runs in its own interpreter.  Scale M has
    channel counts that are not multiples of 64 (48, 96, 192 ...): partially filled channel blocks."""
    import os
    import subprocess
    import sys
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "yolo_conv_variant_probe.py")
    out = {}
    for name, env in [("tile128", {"TSTAR_YOLO_SW": "0", "TSTAR_YOLO_TM": "8", "TSTAR_YOLO_HALO": "0"}), ("tile64", {"TSTAR_YOLO_SW": "0", "TSTAR_YOLO_TM": "4", "TSTAR_YOLO_HALO": "0"}),
                      ("sw8", {"TSTAR_YOLO_SW": "1", "TSTAR_YOLO_SW_P": "8", "TSTAR_YOLO_HALO": "0"}),
                      ("sw4", {"TSTAR_YOLO_SW": "1", "TSTAR_YOLO_SW_P": "4", "TSTAR_YOLO_HALO": "0"}),
                      ("halo16", {"TSTAR_YOLO_HALO": "2", "TSTAR_YOLO_HALO_NCH": "16"}), ("halo8", {"TSTAR_YOLO_HALO": "2", "TSTAR_YOLO_HALO_NCH": "8"}),
                      ("policy", {})]:
        e = dict(os.environ, **env)
        for k in ("TSTAR_YOLO_SW", "TSTAR_YOLO_SW_P", "TSTAR_YOLO_SW_MIN", "TSTAR_YOLO_TM", "TSTAR_YOLO_TM_MIN", "TSTAR_YOLO_TN", "TSTAR_YOLO_HALO",
                  "TSTAR_YOLO_HALO_NCH", "TSTAR_YOLO_HALO8_MAX", "TSTAR_YOLO_HALO8_MIN"):
            if k not in env:
                e.pop(k, None)
        p = subprocess.run([sys.executable, probe, scale, str(batch)], env=e, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        out[name] = [ln for ln in p.stdout.splitlines() if ln.startswith("SHA")][0]
    assert len(set(out.values())) == 1, out


def test_large_batch_default_policy_vs_oracle(yolo):
    """B = 16 puts the 160x160 / 80x80 layers above the thresholds at which the per-layer policy switches to the
    scalar-weight kernels (both variants): images 0 and 15 of the batch against the CPU statement, and image 0 bit-equal
    to the same image scored alone (batch-size independence across kernels)."""
    from oracle import yolo_ref as R
    from tstar_amd.yolo import YoloDetector
    det = YoloDetector(yolo["sd"], "l", max_batch=16)
    det.set_text_feats(yolo["txt"], [1.0, 0.5, 0.5, 0.5])
    imgs = np.stack([GU.detector_test_image(120 + b, 285, 600) for b in range(16)])
    r = det.detect(torch.from_numpy(imgs).cuda(), 1, 1, want_dense=True)
    r1 = det.detect(torch.from_numpy(imgs[:1]).cuda(), 1, 1, want_dense=True)
    torch.cuda.synchronize()
    assert torch.equal(r.dense_scores[0], r1.dense_scores[0]) and torch.equal(r.dense_boxes[0], r1.dense_boxes[0])
    ref = R.detect(yolo["sd"], [imgs[0], imgs[15]], yolo["txt"])
    for j, b in enumerate((0, 15)):
        err = np.abs(r.dense_scores[b].cpu().numpy() - ref[j]["dense_scores"]).max()
        assert err < SCORE_TOL, err
        assert np.abs(r.dense_boxes[b].cpu().numpy() - ref[j]["dense_boxes"]).max() < 0.05
    det.close()


def test_letterbox_input_is_byte_exact(yolo):
    """The ingest (keep-ratio AREA / LINEAR resize, pad 114, channel swap, / 255) feeds the first conv; it is integer work
    and must agree with the oracle exactly -- checked through a 1-query detector whose stem sees only that input: here via
    dense scores being reproducible for a padded-only image and via the chunking path (B = 3 > max_batch = 2)."""
    imgs = np.stack([GU.detector_test_image(70 + b, 285, 600) for b in range(3)])
    det = yolo["det"]
    a = det.detect(torch.from_numpy(imgs).cuda(), 1, 1, want_dense=True)
    torch.cuda.synchronize()
    for b in range(3):
        one = det.detect(torch.from_numpy(imgs[b:b + 1]).cuda(), 1, 1, want_dense=True)
        assert torch.equal(one.dense_scores[0], a.dense_scores[b]) and torch.equal(one.boxes[0], a.boxes[b])
        assert int(one.n_kept[0]) == int(a.n_kept[b])


def test_wrapper_semantics_and_query_sets(yolo):
    """score_threshold / max_dets are the wrapper's (interface_heuristic.py:136, 148-152); per-image query sets."""
    det = yolo["det"]
    img = torch.from_numpy(np.stack([GU.detector_test_image(60, 380, 800)] * 2)).cuda()
    base = det.detect(img[:1], 4, 4, want_dense=True)
    few = det.detect(img[:1], 4, 4, max_dets=7)
    assert int(few.n_kept[0]) == 7 and torch.equal(few.scores[0, :7], base.scores[0, :7])
    hi = float(base.scores[0, 9])
    strict = det.detect(img[:1], 4, 4, score_threshold=hi)
    assert int(strict.n_kept[0]) == 9                      # strictly greater
    none = det.detect(img[:1], 4, 4, score_threshold=0.999)
    assert int(none.n_kept[0]) == 0 and float(none.cell_conf.abs().sum()) == 0.0
    # a second query set with other texts: image 1 scored against it, image 0 unchanged
    rs = np.random.RandomState(5)
    t2 = rs.standard_normal((6, 512)).astype(np.float32)
    det.set_text_feats(t2 / np.linalg.norm(t2, axis=1, keepdims=True), [1.0] * 6, slot=3)
    both = det.detect(img, 4, 4, image_sets=[0, 3])
    assert torch.equal(both.scores[0], base.scores[0]) and torch.equal(both.boxes[0], base.boxes[0])
    alone = det.detect(img[1:], 4, 4, image_sets=[3])
    assert torch.equal(both.scores[1], alone.scores[0]) and torch.equal(both.labels[1], alone.labels[0])
    assert int(both.labels[1].max()) <= 5
    from tstar_amd import _lib
    with pytest.raises(_lib.TStarHipError, match="no text features installed"):
        det.detect(img, 4, 4, image_sets=[0, 9])



def test_yolo_staging_grows_and_is_reused():
    """The handle's grow-on-demand staging over a call sequence that grows all of it: slot 0 with Q = 2, a B = 1 detection; then
    slot 1 with Q = 5 (four times the candidate entries per image) and a B = 2 detection of a larger source image with
    image_sets = [1, 0] (the image -> query-set array, the resized u8 images).  Each image of the batch equals its single-image
    call bit for bit, and the first call repeated returns what it returned at the start."""
    from tstar_amd import yolo_world as Y
    from tstar_amd.yolo import YoloDetector
    det = YoloDetector(Y.synthetic_state_dict(0, "s"), "s", max_batch=2)
    rs = np.random.RandomState(3)
    txt = rs.standard_normal((7, 512)).astype(np.float32)
    txt /= np.linalg.norm(txt, axis=1, keepdims=True)
    keys = ("scores", "labels", "boxes", "n_kept", "cell_conf", "cell_mask")
    same = lambda a, i, b, ks: all(torch.equal(getattr(a, k)[i], getattr(b, k)[0]) for k in ks)
    det.set_text_feats(txt[:2], [1.0, 0.5])
    small = torch.from_numpy(GU.detector_test_image(70, 95, 200)).cuda().unsqueeze(0)
    first = det.detect(small, 2, 2, score_threshold=0.001, want_dense=True)
    det.set_text_feats(txt[2:], [1.0, 0.5, 0.5, 0.25, 0.25], slot=1)
    big = torch.from_numpy(np.stack([GU.detector_test_image(71 + b, 300, 400) for b in range(2)])).cuda()
    both = det.detect(big, 2, 2, score_threshold=0.001, image_sets=[1, 0])
    assert int(both.n_kept.min()) > 0 and int(first.n_kept[0]) > 0
    for b, slot in enumerate([1, 0]):
        one = det.detect(big[b:b + 1], 2, 2, score_threshold=0.001, image_sets=[slot], want_dense=True)
        assert same(both, b, one, keys), b
        assert one.dense_scores.shape[2] == (5, 2)[b] and int(one.labels[0].max()) < (5, 2)[b]
    again = det.detect(small, 2, 2, score_threshold=0.001, want_dense=True)
    assert same(first, 0, again, keys + ("dense_scores", "dense_boxes"))
    det.close()


def test_interface_surface_and_search_replay():
    """initialize_heuristic("yolo-World") -> YoloWorldInterface with the reference's surface; a T* search on the 3600-frame
    video through the fast path, replayed through the oracle searcher (same sampled seconds, histories, keyframes); the
    generic path (inference_detector + the Python cell loop) gives the same search."""
    from oracle import replay
    from tstar_amd.interface_heuristic import Detections, YoloWorldInterface, initialize_heuristic
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    with pytest.raises(FileNotFoundError, match="no YOLO-World checkpoint"):
        initialize_heuristic("yolo-World")
    h = initialize_heuristic("yolo-World", synthetic_seed=0, scale="l", max_batch=16)
    assert isinstance(h, YoloWorldInterface) and h.scale == "l"
    h.reparameterize_object_list(["couch "], ["tv", "chair"])
    assert h.texts == [["couch"], ["tv"], ["chair"], [" "]]
    img = GU.detector_test_image(61, 380, 800)
    dets = h.inference_detector([img, img[::-1]])                    # only images[0]
    assert len(dets) == 1 and isinstance(dets[0], Detections) and h.detections_inbatch is dets
    d = dets[0]
    assert 0 < len(d) <= 50 and d.xyxy.dtype == np.float32 and d.class_id.dtype == np.int64
    assert (d.confidence > 0.12).all() and np.all(np.diff(d.confidence) <= 0)
    assert d.xyxy.min() >= 0 and d.xyxy[:, 0::2].max() <= 800 and d.xyxy[:, 1::2].max() <= 380
    assert len(h.inference_detector([img], max_dets=5)[0]) == 5
    anno = h.bbox_visualization([img], dets)
    assert anno[0].shape == img.shape and anno[0] is not img and not np.array_equal(anno[0], img)
    # search + teacher-forced replay
    N, g, K, seed = 3600, 4, 8, 2025
    store = synthetic_video(N, seed=0)
    rec = replay.Recorder(h, keep_images=False)
    s = TStarSearcher(video_path=store, heuristic=h, target_objects=["couch"], cue_objects=["tv", "chair"], search_nframes=K,
                      image_grid_shape=(g, g), search_budget=0.02, confidence_threshold=0.6, rng=np.random.RandomState(seed),
                      keep_visual_history=False)
    log = []
    orig = s.sample_frames
    s.sample_frames = lambda num: (lambda r: (log.append(list(r[0])), r)[1])(orig(num))
    _, ts = s.search()
    rec.restore()
    assert s.iterations == 5                                         # budget 72 -> 5 iterations of 16
    ref, ts_ref = replay.replay_through_oracle(rec.calls, h.texts, ["couch"], ["tv", "chair"], N, g, K, 0.02, 0.6, seed)
    assert [it["secs"] for it in ref.trace] == log and ts_ref == [float(t) for t in ts]
    assert np.array_equal(s.score_distribution, ref.score)
    assert np.array_equal(np.asarray(s.P_history[-1]), ref.P_history[-1])

    class Foreign:                                                   # only the reference's duck-typed surface
        def __init__(self, inner):
            self.inner, self.texts, self.detections_inbatch = inner, inner.texts, []

        def reparameterize_object_list(self, t, c):
            self.inner.reparameterize_object_list(t, c)
            self.texts = self.inner.texts

        def inference_detector(self, images, **kw):
            self.detections_inbatch = self.inner.inference_detector(images, **kw)
            return self.detections_inbatch

        def bbox_visualization(self, images, detections_inbatch):
            return self.inner.bbox_visualization(images, detections_inbatch)

    b = TStarSearcher(video_path=store, heuristic=Foreign(h), target_objects=["couch"], cue_objects=["tv", "chair"], search_nframes=K,
                      image_grid_shape=(g, g), search_budget=0.02, confidence_threshold=0.6, rng=np.random.RandomState(seed),
                      keep_visual_history=False)
    _, tb = b.search()
    assert [float(t) for t in tb] == [float(t) for t in ts] and np.array_equal(b.score_distribution, s.score_distribution)
    print(f"yolo search: keyframes {ts_ref}, {s.detector_calls} detector calls, {s.frames_scored} frames scored")


def test_search_replay_randomized():
    """Six seeded random searches on the YOLO-World backend (scale S) -- video length, grid, K, threshold, budget, targets
    and cues -- closed-loop on the HIP pipeline, the recorded confidences replayed through the oracle searcher: the same
    sampled seconds every iteration, the same histories and keyframes, no detector batch the reference loop would not ask
    for."""
    from oracle import replay
    from tstar_amd.interface_heuristic import initialize_heuristic
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    rs = np.random.RandomState(777)
    objs = ["couch", "tv", "chair", "dog", "ball", "lamp", "cup"]
    h = initialize_heuristic("yolo-World", synthetic_seed=1, scale="s", max_batch=16)
    for case in range(6):
        g = int(rs.choice([2, 3, 4, 5]))
        N = int(rs.randint(max(2 * g * g, 40), 1500))
        K = int(rs.randint(1, 10))
        thr = float(rs.choice([0.05, 0.3, 0.6, 0.95]))
        budget = float(rs.choice([0.1, 0.3])) if rs.rand() < 0.6 else int(rs.randint(g * g, 5 * g * g))
        pick = list(rs.permutation(objs))
        targets, cues = [str(x) for x in pick[:int(rs.randint(1, 3))]], [str(x) for x in pick[3:3 + int(rs.randint(0, 3))]]
        seed = int(rs.randint(0, 10000))
        rec = replay.Recorder(h, keep_images=False)
        s = TStarSearcher(video_path=synthetic_video(N, seed=300 + case), heuristic=h, target_objects=targets, cue_objects=cues,
                          search_nframes=K, image_grid_shape=(g, g), search_budget=budget, confidence_threshold=thr,
                          rng=np.random.RandomState(seed), keep_visual_history=False)
        log = []
        orig = s.sample_frames
        s.sample_frames = lambda num, orig=orig, log=log: (lambda r: (log.append(list(r[0])), r)[1])(orig(num))
        _, ts = s.search()
        rec.restore()
        ref, ts_ref = replay.replay_through_oracle(rec.calls, h.texts, targets, cues, N, g, K, budget, thr, seed)
        assert [it["secs"] for it in ref.trace] == log, case
        assert ts_ref == [float(t) for t in ts], case
        assert np.array_equal(s.score_distribution, ref.score), case
        for i in range(s.iterations):
            assert np.array_equal(np.asarray(s.P_history[i]), ref.P_history[i]), (case, i)
        print(f"case {case}: N={N} g={g} K={K} thr={thr} budget={budget} {targets} {cues}: {s.iterations} iterations, keyframes {ts_ref}")


def test_alternating_lockstep_groups_on_the_yolo_backend():
    """Two lock-step groups alternating on the GPU with the YOLO-World backend (scale S) against the same items searched one
    by one: the same keyframes, score distributions, call counts and P, bit for bit (the group's questions go through one
    text-tower forward, the constructor's slot-0 install stays pending, candidates come from the cell bitmasks)."""
    from tstar_amd.interface_heuristic import initialize_heuristic
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.lockstep import search_lockstep_groups
    from tstar_amd.video import synthetic_video
    rs = np.random.RandomState(31337)
    objs = ["couch", "tv", "chair", "dog", "ball", "lamp", "cup"]
    h = initialize_heuristic("yolo-World", synthetic_seed=1, scale="s", max_batch=16)
    specs = []
    for grp, (g, n_items) in enumerate([(3, 4), (4, 3)]):
        row = []
        for i in range(n_items):
            pick = [str(x) for x in rs.permutation(objs)]
            row.append(dict(store=synthetic_video(int(rs.randint(60, 400)), seed=700 + 10 * grp + i), g=g, t=pick[:int(rs.randint(1, 3))],
                            c=pick[3:3 + int(rs.randint(0, 3))], K=int(rs.randint(1, 7)), thr=float(rs.choice([0.05, 0.3, 0.6])),
                            b=float(rs.choice([0.2, 0.5])), seed=int(rs.randint(0, 10000))))
        specs.append(row)

    def make(sp):
        return TStarSearcher(sp["store"], h, list(sp["t"]), list(sp["c"]), search_nframes=sp["K"], image_grid_shape=(sp["g"], sp["g"]),
                             search_budget=sp["b"], confidence_threshold=sp["thr"], rng=np.random.RandomState(sp["seed"]),
                             keep_visual_history=False)

    seq = []
    for row in specs:
        for sp in row:
            s = make(sp)
            fr, ts = s.search()
            seq.append((fr, ts, s.score_distribution, s.frames_scored, s.detector_calls, s.iterations, s.P_history[-1]))
    groups = [[make(sp) for sp in row] for row in specs]
    res = search_lockstep_groups(groups)
    flat = [(s, r) for ss, rr in zip(groups, res) for s, r in zip(ss, rr)]
    for k, ((s, r), e) in enumerate(zip(flat, seq)):
        assert r[1] == e[1] and np.array_equal(r[0], e[0]), k
        assert np.array_equal(s.score_distribution, e[2]), k
        assert (s.frames_scored, s.detector_calls, s.iterations) == e[3:6], k
        assert s.P_history[-1] == e[6], k
