"""Detector parity on the GPU: HIP OWL-ViT scorer (through the C ABI) vs the CPU oracle
(oracle/owl_ref.py, pinned against HF transformers) on the same seeded inputs.

Tolerance: per-frame detector scores within 1e-3 (BASELINE.json north_star); the
assertions below use tighter bounds that reflect what fp32 MFMA actually delivers.
Byte/integer stages (bicubic resize, normalisation LUT, patchify, grid-cell mapping)
are bit-exact.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-3     # the contract
TIGHT = 5e-5         # what we expect from exact-f32 MFMA vs CPU fp32


def _token_ids(names):
    """Hand-made CLIP-style ids (no vocab offline): [BOS, toks.., EOS, 0 pad]."""
    ids = np.zeros((len(names), 16), dtype=np.int64)
    am = np.zeros((len(names), 16), dtype=np.int64)
    for i, n in enumerate(names):
        toks = [49406] + [1000 + (sum(map(ord, w)) * 31 + len(w)) % 40000 for w in n.split()] + [49407]
        ids[i, :len(toks)] = toks
        am[i, :len(toks)] = 1
    return ids, am


@pytest.fixture(scope="module")
def setup():
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    sd = W.synthetic_state_dict(0)
    vb = W.pack_blob(sd, W.vision_spec())
    tb = W.pack_blob(sd, W.text_spec())
    scorer = OwlScorer(vb, tb, max_batch=2)
    wv = W.unpack_blob(vb, W.vision_spec())
    wt = W.unpack_blob(tb, W.text_spec())
    names = ["couch", "tv", "chair", " "]
    ids, am = _token_ids(["couch", "tv", "chair", ""])
    weights = [1.0, 0.5, 0.5, 0.5]
    scorer.set_queries(ids, am, weights)
    return dict(scorer=scorer, wv=wv, wt=wt, ids=ids, am=am, names=names, weights=weights, vb=vb, tb=tb)


@pytest.fixture(scope="module")
def setup_x3(setup):
    """The same weights and queries on a scorer in the f32x3 mode."""
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    sd = W.synthetic_state_dict(0)
    sc = OwlScorer(W.pack_blob(sd, W.vision_spec()), W.pack_blob(sd, W.text_spec()), max_batch=2, weights_mode="f32x3")
    sc.set_queries(setup["ids"], setup["am"], setup["weights"])
    yield sc
    sc.close()


_ORACLE_CACHE = {}          # (H, W, B) -> oracle detect() of _images(B, H, W, 3): shared by the weight modes


def _images(B, H, W, seed):
    rs = np.random.RandomState(seed)
    low = rs.randint(0, 256, (B, H // 8 + 1, W // 8 + 1, 3)).astype(np.float32)
    img = np.repeat(np.repeat(low, 8, axis=1), 8, axis=2)[:, :H, :W]
    img = img + rs.randint(-20, 20, (B, H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def test_text_tower(setup):
    from oracle import owl_ref
    ref = owl_ref.text_query_embeds(setup["ids"], setup["am"], setup["wt"]).numpy()
    got = setup["scorer"].get_query_embeds()
    assert np.abs(got - ref).max() < 2e-6
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("H,W", [(380, 800), (285, 600), (1520, 3200)])
def test_preprocess_bit_exact(setup, H, W):
    from oracle import resize_ref as R
    img = _images(1, H, W, 7)
    u8, pat = setup["scorer"].debug_preprocess(torch.from_numpy(img).cuda())
    torch.cuda.synchronize()
    ref_u8 = R.pil_bicubic_resize(img[0], 768, 768)
    assert np.array_equal(u8[0].cpu().numpy(), ref_u8)
    ref_pat = R.patchify(R.hf_rescale_normalize(ref_u8))
    assert np.array_equal(pat.cpu().numpy(), ref_pat)


def test_preprocess_random_source_sizes(setup):
    """Pillow's bicubic resample to 768x768 from 14 seeded random source sizes with dense noise (upscales, 20x decimation,
    extreme aspect ratios, the 768x768 identity, every grid size 95g x 200g is covered above): resized bytes and patch
    matrix bit-exact against the oracle (itself bit-equal to the real Pillow / HF image processor)."""
    from oracle import resize_ref as R
    rs = np.random.RandomState(123)
    sizes = [(768, 768), (2, 2), (3, 1500), (1536, 1536), (240, 427), (95, 200)]
    while len(sizes) < 14:
        sizes.append((int(rs.randint(4, 1700)), int(rs.randint(4, 3300))))
    for H, W in sizes:
        img = rs.randint(0, 256, (1, H, W, 3), dtype=np.uint8)
        u8, pat = setup["scorer"].debug_preprocess(torch.from_numpy(img).cuda())
        torch.cuda.synchronize()
        ref_u8 = R.pil_bicubic_resize(img[0], 768, 768)
        assert np.array_equal(u8[0].cpu().numpy(), ref_u8), (H, W)
        assert np.array_equal(pat.cpu().numpy(), R.patchify(R.hf_rescale_normalize(ref_u8))), (H, W)


# (380,800,4,4) = the reference's default grid; (285,600,1,1) = a verification frame; (1520,3200,16,16) = BASELINE
# configs[1] (256 frames per grid image, what bench.py times); (1425,3000,15,15) = configs[4]
@pytest.mark.parametrize("H,W,rows,cols,B", [(380, 800, 4, 4, 3), (285, 600, 1, 1, 2), (1520, 3200, 16, 16, 2),
                                              (1425, 3000, 15, 15, 1)])
@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_detector_vs_oracle(setup, setup_x3, mode, H, W, rows, cols, B):
    """Both weight modes against the SAME oracle figures at the SAME bounds: "f32" = the exact-f32 MFMA tile, "f32x3" = the
    headline mode of round 5 (every GEMM / attention operand as three exact bf16 terms on the bf16 matrix pipe)."""
    from oracle import owl_ref, resize_ref as R, searcher_ref as S
    img = _images(B, H, W, 3)
    scorer = setup["scorer"] if mode == "f32" else setup_x3
    r = scorer.score(torch.from_numpy(img).cuda(), rows, cols, want_logits=True)
    torch.cuda.synchronize()
    key = (H, W, B)
    if key not in _ORACLE_CACHE:
        px = np.stack([R.owl_preprocess(im) for im in img])
        qe = owl_ref.text_query_embeds(setup["ids"], setup["am"], setup["wt"]).numpy()
        qmask = setup["ids"][:, 0] > 0
        _ORACLE_CACHE[key] = owl_ref.detect(px, qe, setup["wv"], H, W, query_mask=qmask)
    ref = _ORACLE_CACHE[key]
    logits = r.logits.cpu().numpy()
    assert np.abs(logits - ref["logits"]).max() < 2e-4
    assert np.abs(r.boxes_cxcywh.cpu().numpy() - ref["boxes"]).max() < TIGHT
    d_score, d_lab, d_xyxy = ref["dense"]
    scores = r.scores.cpu().numpy()
    assert np.abs(scores - d_score).max() < SCORE_TOL
    assert np.abs(scores - d_score).max() < TIGHT
    assert np.abs(r.boxes.cpu().numpy() - d_xyxy).max() < TIGHT * max(H, W)    # pixels: the cxcywh bound scaled by the image
    # labels: equal wherever the oracle's top-2 margin is not at rounding level
    srt = np.sort(ref["logits"], axis=-1)
    clear = (srt[..., -1] - srt[..., -2]) > 1e-4
    labels = r.labels.cpu().numpy()
    assert np.array_equal(labels[clear], d_lab[clear])
    assert clear.mean() > 0.9
    # grid-cell aggregation: replay the reference loop on the GPU's own detections -> bit-exact
    texts = [[n] for n in setup["names"]]
    o2w = {"couch": 1.0, "tv": 0.5, "chair": 0.5}
    cc = r.cell_conf.cpu().numpy()
    cm = r.cell_mask.cpu().numpy().astype(np.uint32)
    nk = r.n_kept.cpu().numpy()
    boxes = r.boxes.cpu().numpy()
    for b in range(B):
        keep = scores[b] > np.float32(0.005)
        assert nk[b] == keep.sum()
        conf_map, names = S.image_grid_score(boxes[b][keep], labels[b][keep], scores[b][keep], texts, o2w, H, W, rows, cols)
        assert np.array_equal(cc[b].reshape(rows, cols), conf_map)
        for cell in range(rows * cols):
            want = 0
            for n in names[cell]:
                want |= 1 << setup["names"].index(n)
            assert cm[b, cell] == want


def test_chunked_mixed_query_set_batch_equals_per_image_calls():
    """One tstar_owl_score call with B = 300 verification images (285x600) against THREE resident query sets of different
    sizes on a scorer with max_batch = 256 -- i.e. one full chunk + a 44-image remainder chunk, the shape bench.py's
    lock-step verification batches have -- must equal 300 single-image calls bit for bit: scores, labels, boxes, cell
    confidences, class masks, kept counts."""
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    sd = W.synthetic_state_dict(0)
    sc = OwlScorer(W.pack_blob(sd, W.vision_spec()), W.pack_blob(sd, W.text_spec()), max_batch=256)
    sets = {0: ["couch", "tv", "chair", ""], 3: ["dog", "leash", ""], 7: ["red car", "road", "tree", "sign", "bus", ""]}
    for slot, names in sets.items():
        ids, am = _token_ids(names)
        sc.set_queries(ids, am, [1.0] + [0.5] * (len(names) - 1), slot=slot)
    B = 300
    rs = np.random.RandomState(12)
    base = _images(8, 285, 600, 21)
    img = torch.from_numpy(base).cuda()[torch.from_numpy(rs.randint(0, 8, B)).cuda()].contiguous()
    img[:, :40, :40, :] = torch.from_numpy(rs.randint(0, 256, (B, 40, 40, 3)).astype(np.uint8)).cuda()   # all distinct
    image_sets = [list(sets)[i % 3] for i in range(B)]
    big = sc.score(img, 1, 1, image_sets=image_sets)
    torch.cuda.synchronize()
    for b in range(B):
        one = sc.score(img[b:b + 1], 1, 1, image_sets=[image_sets[b]])
        assert torch.equal(one.scores[0], big.scores[b]), b
        assert torch.equal(one.labels[0], big.labels[b]) and torch.equal(one.boxes[0], big.boxes[b])
        assert torch.equal(one.cell_conf[0], big.cell_conf[b]) and torch.equal(one.cell_mask[0], big.cell_mask[b])
        assert int(one.n_kept[0]) == int(big.n_kept[b])
    for slot, names in sets.items():          # a label never exceeds its own set's query count
        m = torch.tensor([s_ == slot for s_ in image_sets], device="cuda")
        assert int(big.labels[m].max()) < len(names)
    sc.close()


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_second_workspace_lane_same_bits_alone_and_concurrently(mode):
    """Round 6: ``tstar_owl_score_lane`` -- lane 1 is a second, small activation workspace of the same handle (4 images, grown to the
    largest batch it has seen).  A forward in lane 1 gives the bits of the same forward in lane 0 (B = 1, and B = 6 after the workspace grew),
    and a lane-1 grid forward enqueued on ANOTHER stream while a lane-0 verification-size batch is running returns the same bits as
    when each runs alone (the two share no mutable state): what the searcher's speculative next-grid forward relies on."""
    from tstar_amd.interface_heuristic import OWLInterface
    h = OWLInterface(synthetic_seed=0, max_batch=16, weights_dtype=mode)
    h.reparameterize_object_list(["couch"], ["tv", "chair"])
    g = torch.Generator(device="cuda").manual_seed(11)
    grid = torch.randint(0, 255, (1, 380, 800, 3), dtype=torch.uint8, device="cuda", generator=g)
    ver = torch.randint(0, 255, (12, 285, 600, 3), dtype=torch.uint8, device="cuda", generator=g)
    six = torch.randint(0, 255, (6, 285, 600, 3), dtype=torch.uint8, device="cuda", generator=g)
    keys = ("scores", "labels", "boxes", "cell_conf", "cell_mask", "n_kept")
    same = lambda a, b: all(torch.equal(getattr(a, k), getattr(b, k)) for k in keys)
    g0, v0, s0 = h.score_batch(grid, 4, 4), h.score_batch(ver, 1, 1), h.score_batch(six, 1, 1)
    g1, s1 = h.score_batch(grid, 4, 4, lane=1), h.score_batch(six, 1, 1, lane=1)
    torch.cuda.synchronize()
    assert same(g0, g1) and same(s0, s1)
    aux = torch.cuda.Stream()
    for _ in range(3):
        aux.wait_stream(torch.cuda.current_stream())
        vb = [h.score_batch(ver, 1, 1) for _ in range(3)]             # lane 0, this stream: ~20 ms of work
        with torch.cuda.stream(aux):
            gb = [h.score_batch(grid, 4, 4, lane=1) for _ in range(3)]     # lane 1, the other stream, at the same time
        torch.cuda.synchronize()
        assert all(same(v0, r) for r in vb) and all(same(g0, r) for r in gb)
    with pytest.raises(Exception, match="lane must be 0 or 1"):
        h.score_batch(grid, 4, 4, lane=2)


def test_non_dyadic_class_weights_are_float64(setup):
    """object2weight is a constructor argument of the searcher (interface_searcher.py:31,88-91,136): with a weight such as
    0.7 the confidence ``np.float32 score * Python float`` is a float64 product under the reference's pinned numpy 1.26;
    the float32 product differs in the last bits (and feeds the percentile thresholds and the spline fit).  The cell
    aggregation must be the float64 product, bit for bit."""
    from oracle import searcher_ref as S
    scorer = setup["scorer"]
    weights = [1.0, 0.7, 0.3, 0.7]
    scorer.set_class_weights(weights)
    try:
        H, W, rows, cols = 380, 800, 4, 4
        img = _images(2, H, W, 5)
        r = scorer.score(torch.from_numpy(img).cuda(), rows, cols)
        torch.cuda.synchronize()
        scores, labels, boxes = r.scores.cpu().numpy(), r.labels.cpu().numpy(), r.boxes.cpu().numpy()
        cc = r.cell_conf.cpu().numpy()
        texts = [[n] for n in setup["names"]]
        o2w = dict(zip(setup["names"], weights))
        n_f32_differs = 0
        for b in range(2):
            keep = scores[b] > np.float32(0.005)
            cm, _ = S.image_grid_score(boxes[b][keep], labels[b][keep], scores[b][keep], texts, o2w, H, W, rows, cols)
            assert np.array_equal(cc[b].reshape(rows, cols), cm)
            f32 = (scores[b][keep] * np.array([weights[l] for l in labels[b][keep]], np.float32)).astype(np.float64)
            f64 = scores[b][keep].astype(np.float64) * np.array([weights[l] for l in labels[b][keep]])
            n_f32_differs += int(np.count_nonzero(f32 != f64))
        assert n_f32_differs > 0          # the case does distinguish the two products
    finally:
        scorer.set_class_weights(setup["weights"])


def test_detector_f32x3_mode_at_the_f32_bound(setup):
    """weights_mode "f32x3" (f32 checkpoint on the bf16 matrix pipe, three exact bf16 terms per operand, six products;
    attention / LayerNorm / head tails stay f32): the gate of the round-3 review -- detector scores, logits and boxes against
    the f32 CPU oracle inside the UNCHANGED tight bound of the exact-f32 tile (TIGHT = 5e-5; contract 1e-3), the exact-f32
    tile's own error printed next to it."""
    from oracle import owl_ref, resize_ref as R
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    sd = W.synthetic_state_dict(0)
    sc = OwlScorer(W.pack_blob(sd, W.vision_spec()), W.pack_blob(sd, W.text_spec()), max_batch=2, weights_mode="f32x3")
    sc.set_queries(setup["ids"], setup["am"], setup["weights"])
    H, Wd, B = 380, 800, 3
    img = _images(B, H, Wd, 3)
    r = sc.score(torch.from_numpy(img).cuda(), 4, 4, want_logits=True)
    r32 = setup["scorer"].score(torch.from_numpy(img).cuda(), 4, 4, want_logits=True)
    torch.cuda.synchronize()
    px = np.stack([R.owl_preprocess(im) for im in img])
    qe = owl_ref.text_query_embeds(setup["ids"], setup["am"], setup["wt"]).numpy()
    ref = owl_ref.detect(px, qe, setup["wv"], H, Wd, query_mask=setup["ids"][:, 0] > 0)
    d_score = ref["dense"][0]
    err = np.abs(r.scores.cpu().numpy() - d_score).max()
    err32 = np.abs(r32.scores.cpu().numpy() - d_score).max()
    lerr = np.abs(r.logits.cpu().numpy() - ref["logits"]).max()
    lerr32 = np.abs(r32.logits.cpu().numpy() - ref["logits"]).max()
    print(f"f32x3: max score error {err:.2e} (exact-f32 tile {err32:.2e}), max logit error {lerr:.2e} ({lerr32:.2e})")
    assert err < TIGHT
    assert lerr < 2e-4                                              # the logits bound of test_detector_vs_oracle
    assert np.abs(r.boxes_cxcywh.cpu().numpy() - ref["boxes"]).max() < TIGHT
    # query embeddings come from the text tower run in the same mode
    assert np.abs(sc.get_query_embeds() - qe).max() < 2e-6
    sc.close()


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
@pytest.mark.parametrize("k", [0, 1])
def test_g7_hip_vs_reference_detector_golden(golden_dir, mode, k):
    """DIRECT comparison of the HIP path with REFERENCE outputs (no oracle in between): golden G7 holds what the reference's
    own ``OWLInterface.inference_detector`` (/root/reference/TStar/interface_heuristic.py:232-246, HF transformers'
    OwlViTForObjectDetection + post_process_object_detection at threshold 0.005) produced for ``detector_test_image(40 + k)``
    at both image shapes (380x800 grid image, 285x600 verification frame): raw logits, pred_boxes, text embeddings and the
    kept (xyxy, confidence, class_id).  Gated at the contract (scores within 1e-3 fp32) and at the tight f32 bound; the
    measured errors are printed.  Both weight modes: native f32 MFMA tile and f32x3 (three exact bf16 terms per operand)."""
    import os
    import golden_util as GU
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    g7 = np.load(os.path.join(golden_dir, "g7_g8_detector.npz"), allow_pickle=False)
    sd = W.synthetic_state_dict(0)
    sc = OwlScorer(W.pack_blob(sd, W.vision_spec()), W.pack_blob(sd, W.text_spec()), max_batch=1, weights_mode=mode)
    try:
        ids, am = g7["ids"], g7["mask"]
        sc.set_queries(ids, am, [1.0] * len(ids))
        seed, H, Wd = [int(v) for v in g7[f"img_meta{k}"]]
        img = GU.detector_test_image(seed, H, Wd)
        assert GU.sha(img) == str(g7[f"img_sha{k}"][0])
        r = sc.score(torch.from_numpy(img).cuda().unsqueeze(0), 1, 1, want_logits=True)
        torch.cuda.synchronize()
        e_q = np.abs(sc.get_query_embeds() - g7[f"query_embeds{k}"]).max()
        logits, cxcywh = r.logits[0].cpu().numpy(), r.boxes_cxcywh[0].cpu().numpy()
        e_logit = np.abs(logits - g7[f"logits{k}"]).max()
        e_box = np.abs(cxcywh - g7[f"boxes{k}"]).max()
        # the reference's dense per-patch scores / labels from ITS logits (sigmoid of the max, arg-max: the statement of
        # post_process_object_detection) against the HIP kernel's
        ref_logits = g7[f"logits{k}"]
        ref_score = (1.0 / (1.0 + np.exp(-ref_logits.max(-1).astype(np.float64)))).astype(np.float32)
        scores, labels, boxes = r.scores[0].cpu().numpy(), r.labels[0].cpu().numpy(), r.boxes[0].cpu().numpy()
        e_score = np.abs(scores - ref_score).max()
        print(f"G7[{k}] {mode}: query embeds {e_q:.2e}, logits {e_logit:.2e}, pred_boxes {e_box:.2e}, dense scores {e_score:.2e}")
        assert e_q < 2e-6 and e_logit < 2e-4 and e_box < TIGHT
        assert e_score < SCORE_TOL and e_score < TIGHT
        # kept detections: the reference keeps score > 0.005 in patch order
        keep = scores > np.float32(0.005)
        ref_keep = ref_score > np.float32(0.005)
        margin = np.abs(ref_score - np.float32(0.005)) > 1e-4          # patches not sitting on the threshold
        assert np.array_equal(keep[margin], ref_keep[margin]) and int(r.n_kept[0]) == int(keep.sum())
        if np.array_equal(keep, ref_keep):
            det_conf, det_cls, det_xyxy = g7[f"det_conf{k}"], g7[f"det_cls{k}"], g7[f"det_xyxy{k}"]
            assert len(det_conf) == int(keep.sum())
            assert np.abs(scores[keep] - det_conf).max() < TIGHT
            assert np.abs(boxes[keep] - det_xyxy).max() < TIGHT * max(H, Wd) + 1e-3
            srt = np.sort(ref_logits[keep], axis=-1)
            clear = (srt[:, -1] - srt[:, -2]) > 1e-4
            assert np.array_equal(labels[keep][clear], det_cls[clear]) and clear.mean() > 0.9
    finally:
        sc.close()


def test_unknown_weights_mode_rejected():
    from tstar_amd.owl import OwlScorer
    with pytest.raises(ValueError, match="weights_mode"):
        OwlScorer(np.zeros(4, np.float32), None, weights_mode="fp8")


def test_score_requires_queries():
    from tstar_amd import _lib
    from tstar_amd.owl import OwlScorer
    from tstar_amd import weights as W
    sd = W.synthetic_state_dict(0, "vision")
    s = OwlScorer(W.pack_blob(sd, W.vision_spec()), None, max_batch=1)
    with pytest.raises(_lib.TStarHipError, match="no queries"):
        s.score(torch.zeros((1, 95, 200, 3), dtype=torch.uint8, device="cuda"), 1, 1)
    with pytest.raises(_lib.TStarHipError, match="without text weights"):
        s.set_queries(np.zeros((1, 16), np.int32), np.ones((1, 16), np.int32), [1.0])


def test_install_queries_many_equals_one_by_one():
    """A lock-step group installs the questions of all its items through ONE text-tower forward
    (tstar_owl_set_queries_many): query embeddings, masks and class weights must equal one install per item bit for bit --
    also when the text-only handle of the YOLO-World backend (40 sequences per forward) has to cut the group into several
    forwards -- and an image scored against a slot gives the same scores either way."""
    import golden_util as GU
    from tstar_amd.interface_heuristic import OWLInterface, YoloWorldInterface
    questions = [(["couch"], ["tv", "chair"]), (["dog"], ["leash", "park bench"]), (["red car"], ["road"]), (["laptop", "mug"], ["desk"]),
                 (["a"], []), (["person riding a horse on the beach"], ["sand", "sea", "sky", "sun"])]
    h = OWLInterface(synthetic_seed=0, max_batch=2)
    items = [(k + 1, list(t), list(c), {t[0]: 0.75}) for k, (t, c) in enumerate(questions)]
    texts_many = h.install_queries_many(items)
    many = [(h.scorer.get_query_embeds(slot).copy(), h.scorer.Qs[slot]) for slot, *_ in items]
    img = torch.from_numpy(GU.detector_test_image(5, 285, 600)).cuda().unsqueeze(0)
    r_many = [h.score_batch(img, 1, 1, image_sets=[slot]).scores.clone() for slot, *_ in items]
    for (slot, t, c, o2w), tm, (e_many, q_many), sc in zip(items, texts_many, many, r_many):
        tx = h.install_queries(slot, t, c, o2w)
        assert tx == tm and h.scorer.Qs[slot] == q_many
        assert np.array_equal(h.scorer.get_query_embeds(slot), e_many), slot
        assert torch.equal(h.score_batch(img, 1, 1, image_sets=[slot]).scores, sc), slot
    with pytest.raises(ValueError, match="slot must be in 1..63"):
        h.install_queries_many([(0, ["a"], [], None)])
    # text-only handle: 12 items x 5 queries = 60 sequences > 40 per forward
    y = YoloWorldInterface(synthetic_seed=0, scale="s", max_batch=1)
    yitems = [(k + 1, [f"thing {k}"], ["one", "two three", "four"], None) for k in range(12)]
    y.install_queries_many(yitems)
    feats = [y.text_tower.get_query_embeds(slot).copy() for slot, *_ in yitems]
    for (slot, t, c, o2w), f in zip(yitems, feats):
        y.install_queries(slot, t, c, o2w)
        assert np.array_equal(y.text_tower.get_query_embeds(0), f), slot          # install_queries encodes through text slot 0


_RESULT_KEYS = ("scores", "labels", "boxes", "cell_conf", "cell_mask", "n_kept")


def _same_image(batch, b, one, keys):
    return all(torch.equal(getattr(batch, k)[b], getattr(one, k)[0]) for k in keys)


@pytest.mark.parametrize("family", ["owlvit", "owlv2"])
def test_owl_staging_grows_and_is_reused(family):
    """The handle's grow-on-demand staging (image -> query-set array, the u8 image of the horizontal resampling pass; OWLv2: the
    per-image clip bounds) over a call sequence that grows it, reuses it and grows it again, on the smallest geometry (input 64 x 96:
    6 patches at B/32, 24 at OWLv2's B/16) with two resident query sets of different sizes: every batch equals its single-image calls bit for bit, and
    the first call repeated at the end returns what it returned at the start."""
    from tstar_amd.owl import OwlScorer
    keys, kw = (_RESULT_KEYS, {}) if family == "owlvit" else (("scores", "objectness"), {"objectness": True})
    sc = OwlScorer.synthetic(0, max_batch=4, input_size=(64, 96), family=family)
    assert sc.num_patches == (6 if family == "owlvit" else 24)
    sets = {0: ["couch", "tv", "chair", ""], 5: ["dog", "leash", ""]}
    for slot, names in sets.items():
        ids, am = _token_ids(names)
        sc.set_queries(ids, am, [1.0] + [0.5] * (len(names) - 1), slot=slot)
    img, big = torch.from_numpy(_images(3, 40, 56, 31)).cuda(), torch.from_numpy(_images(4, 88, 120, 32)).cuda()
    # B = 1; B = 3 grows image_set (and tmp_u8 / minmax); B = 2 fits; OWL-ViT: B = 4 of the larger source grows tmp_u8 again
    calls = [(img[:1], [5]), (img, [0, 5, 0]), (img[1:], [5, 0])] + ([(big, [5, 0, 0, 5])] if family == "owlvit" else [])
    batches = [sc.score(x, 2, 2, image_sets=s, **kw) for x, s in calls]
    for (x, s), r in zip(calls, batches):
        for b in range(len(s)):
            one = sc.score(x[b:b + 1], 2, 2, image_sets=s[b:b + 1], **kw)
            assert _same_image(r, b, one, keys), (len(s), b)
    again = sc.score(img[:1], 2, 2, image_sets=[5], **kw)
    assert _same_image(batches[0], 0, again, keys)
    assert int(batches[1].labels[1].max()) < 3 and int(batches[1].labels[0].max()) < 4      # a label stays inside its own set
    sc.close()


def test_set_queries_many_group_boundaries(setup):
    """tstar_owl_set_queries_many where lane 0 holds 40 sequences per forward (max_batch = 1 at 768 x 768, B/32: 640 rows -- the
    text-only handle of the YOLO-World backend has the same lane; this one has a vision tower too, so that query masks and class
    weights show in a score): set sizes (32, 8, 1) -- the first group exactly full -- then (32, 9) -- a set that does not fit opens
    the next group.  Embeddings, Qs and, through the logits (a masked query's are -inf-like constants) and the cell confidences,
    masks and weights of every slot equal one set_queries per slot bit for bit; tstar_owl_debug_text returns the same rows before
    and after the batched call grew the staging; a token id out of range in the LAST set refuses the whole call before any slot is
    installed."""
    from tstar_amd import _lib, weights as W
    from tstar_amd.owl import OwlScorer
    sc = OwlScorer(setup["vb"], setup["tb"], max_batch=1)
    rs = np.random.RandomState(7)
    img = torch.from_numpy(_images(1, 95, 200, 41)).cuda()

    def entry(slot, Q):
        # [BOS or 0 (query mask 0: every fourth row, the first of a set among them), random ids, EOS, sometimes twice (first maximum), padding]
        ids, am = np.zeros((Q, 16), np.int32), np.zeros((Q, 16), np.int32)
        for q in range(Q):
            toks = [49406 if q % 4 else 0] + list(rs.randint(1, 49000, rs.randint(0, 12))) + [49407] * int(rs.randint(1, 3))
            ids[q, :len(toks)] = toks
            am[q, :len(toks)] = 1
        return (slot, ids, am, rs.uniform(0.1, 1.0, Q))

    def debug_text(ids, am, stage):
        out = np.empty((ids.shape[0] * (16 if stage == 0 else 1), 512), np.float32)
        rc = sc._lib.tstar_owl_debug_text(sc._h, ids.ctypes.data, am.ctypes.data, ids.shape[0], stage, out.ctypes.data, _lib.stream_ptr())
        _lib.check(rc, "tstar_owl_debug_text")
        return out

    def installed(slot):
        r = sc.score(img, 1, 1, image_sets=[slot], want_logits=True, boxes=False)
        return sc.Qs[slot], sc.get_query_embeds(slot), r.logits.cpu().numpy(), r.cell_conf.cpu().numpy(), r.cell_mask.cpu().numpy()

    first = entry(1, 32)
    before = [debug_text(first[1], first[2], stage) for stage in (0, 1)]
    for sizes in ((32, 8, 1), (32, 9)):
        entries = [first] + [entry(2 + k, Q) for k, Q in enumerate(sizes[1:])]
        sc.set_queries_many(entries)
        many = [installed(e[0]) for e in entries]
        for (slot, ids, am, w), m in zip(entries, many):
            sc.set_queries(ids, am, w, slot=slot)
            one = installed(slot)
            assert m[0] == one[0] == ids.shape[0]
            assert all(np.array_equal(a, b) for a, b in zip(m[1:], one[1:])), (sizes, slot)
    for stage in (0, 1):
        assert np.array_equal(debug_text(first[1], first[2], stage), before[stage]), stage
    # refused before anything is launched or installed: every slot keeps its size and its rows
    held = {slot: sc.get_query_embeds(slot) for slot in (1, 2)}
    qs = dict(sc.Qs)
    bad = [entry(1, 3), entry(2, 4), entry(9, 2)]
    bad[2][1][1, 3] = W.VOCAB
    with pytest.raises(_lib.TStarHipError, match="tstar_owl_set_queries_many: token id out of range"):
        sc.set_queries_many(bad)
    assert sc.Qs == qs and 9 not in sc.Qs
    for slot, e in held.items():
        assert np.array_equal(sc.get_query_embeds(slot), e), slot
    sc.close()
