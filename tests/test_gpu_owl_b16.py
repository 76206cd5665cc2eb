"""OWL-ViT B/16 on the HIP detector path (patch 16: 48 x 48 = 2304 patches, T = 2305 tokens).

* an HF-initialised B/16 checkpoint directory through ``OWLInterface(model_name_or_path=dir)`` against HF's own CPU forward;
* the P = 16 im2col of the preprocess kernel, bit for bit;
* the three attention kernels at T = 2305 against float64;
* B/32 through ``tstar_owl_create_ex`` equal to ``tstar_owl_create``;
* forward chunking (max_batch smaller than the batch, and a B/16 handle past its 256-image chunk cap);
* a teacher-forced search, the device painter, and a lock-step group on a B/16 heuristic."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def make_b16_checkpoint_dir(dirpath: str, seed: int = 0):
    """tests/hf_checkpoint_util.make_checkpoint_dir with patch 16: HF's ``OwlViTForObjectDetection`` at its own init, the
    class head's scale / shift and the box head shrunk the same way (unsaturated scores and boxes), ``save_pretrained``
    + a CLIP vocabulary."""
    import transformers
    from clip_vocab_util import write_clip_vocab
    torch.manual_seed(seed)
    m = transformers.OwlViTForObjectDetection(transformers.OwlViTConfig(vision_config={"patch_size": 16})).eval()
    with torch.no_grad():
        for lin in (m.class_head.logit_scale, m.class_head.logit_shift):
            lin.weight.mul_(0.01)
            lin.bias.mul_(0.01)
        for lin in (m.box_head.dense0, m.box_head.dense1, m.box_head.dense2):
            lin.weight.mul_(lin.weight.shape[1] ** -0.5)
    os.makedirs(dirpath, exist_ok=True)
    m.save_pretrained(dirpath, safe_serialization=True)
    write_clip_vocab(dirpath)
    return m


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from transformers import CLIPTokenizer
    d = str(tmp_path_factory.mktemp("owlvit_b16_ckpt"))
    m = make_b16_checkpoint_dir(d, seed=1)
    return d, m, CLIPTokenizer.from_pretrained(d, local_files_only=True)


def _test_images():
    from oracle import resize_ref as R
    from tstar_amd.video import synthetic_frames_numpy
    out = []
    for k, (H_, W_) in enumerate([(285, 600), (1520, 3200)]):
        out.append(R.cv_bilinear_resize(synthetic_frames_numpy([7 + k], 40, 360, 640, seed=5)[0], W_, H_))
    return out


_REF = {}


def _hf_ref(key, model, tok, img, names):
    import hf_checkpoint_util as H
    if key not in _REF:
        _REF[key] = H.hf_detect(model, tok, img, names)
    return _REF[key]


@pytest.mark.parametrize("mode", ["f32", "f32x3", "bf16", "bf16_exact"])
def test_b16_checkpoint_matches_hf(ckpt, mode):
    """Checkpoint parity at B/16: text embeds within 1e-5, dense scores within 1e-3 (observed value printed), 2304 detections
    at threshold 0.005 in patch order, boxes within 1e-2 px; on a 285x600 frame and a 1520x3200 grid image.  The bf16 modes
    are compared with HF run on the same bf16-rounded weights."""
    import copy
    from tstar_amd import weights as W
    from tstar_amd.interface_heuristic import OWLInterface
    d, m, tok = ckpt
    h = OWLInterface(model_name_or_path=d, max_batch=2, weights_dtype=mode)
    assert h.geometry == W.B16 and h.scorer.num_patches == 2304
    assert h.weights_source == os.path.join(d, "model.safetensors")
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
    for k, img in enumerate(_test_images()):
        H_, W_ = img.shape[:2]
        ref = _hf_ref((wkey, k), ref_model, tok, img, names)
        if k == 0:
            assert np.abs(h.scorer.get_query_embeds() - ref["text_embeds"]).max() < 1e-5
        det = h.inference_detector([img])[0]
        r = h.scorer.score(torch.from_numpy(img).cuda().unsqueeze(0), 1, 1)
        dense = r.scores[0].cpu().numpy()
        assert dense.shape == (2304,)
        err = float(np.abs(dense - ref["dense_scores"]).max())
        assert 0.05 < ref["dense_scores"].min() and ref["dense_scores"].max() < 0.95       # not a saturated comparison
        assert len(det) == len(ref["scores"]) == 2304                    # threshold 0.005: every patch kept, patch order
        assert np.abs(det.confidence - ref["scores"]).max() < 1e-3
        box_err = float(np.abs(det.xyxy - ref["xyxy"]).max())
        wh = ref["xyxy"][:, 2:] - ref["xyxy"][:, :2]
        assert wh.min() > 1.0 and wh.max() < max(H_, W_)                # real boxes, not saturated sigmoids
        print(f"B/16 {mode} {H_}x{W_}: max |score - HF| = {err:.2e}, max |box - HF| = {box_err:.2e} px")
        assert err < 1e-3, err
        assert box_err < 1e-2, box_err
    del h


@pytest.mark.parametrize("H,Wd", [(285, 600), (1520, 3200), (97, 301)])
def test_b16_patchify_bit_exact(H, Wd):
    """The P = 16 im2col (row = (y/16)*48 + x/16, col = c*256 + (y%16)*16 + x%16) of the normalised image, bit for bit."""
    from oracle import resize_ref as R
    from tstar_amd.owl import OwlScorer
    rs = np.random.RandomState(H * 7 + Wd)
    img = rs.randint(0, 256, (2, H, Wd, 3)).astype(np.uint8)
    s = OwlScorer.synthetic(0, max_batch=2, with_text=False, patch_size=16)
    u8, pat = s.debug_preprocess(torch.from_numpy(img).cuda())
    torch.cuda.synchronize()
    assert pat.shape == (2 * 2304, 768)
    pat = pat.cpu().numpy().reshape(2, 2304, 768)
    for b in range(2):
        ref_u8 = R.pil_bicubic_resize(img[b], 768, 768)
        assert np.array_equal(u8[b].cpu().numpy(), ref_u8)
        x = R.hf_rescale_normalize(ref_u8).reshape(3, 48, 16, 48, 16).transpose(1, 3, 0, 2, 4).reshape(2304, 768)
        assert np.array_equal(pat[b].view(np.uint32), np.ascontiguousarray(x).view(np.uint32)), b


def _attn_ref64(qkv, B, T, heads):
    D = heads * 64
    out = []
    for b in range(B):                                                  # one image at a time: T^2 * heads float64 scores
        q, k, v = qkv[b * T:(b + 1) * T].double().view(T, 3 * D).split(D, dim=-1)
        q = q.view(T, heads, 64).transpose(0, 1)
        k = k.view(T, heads, 64).transpose(0, 1)
        v = v.view(T, heads, 64).transpose(0, 1)
        att = torch.softmax(torch.matmul(q, k.transpose(1, 2)) * 0.125, dim=-1)
        out.append(torch.matmul(att, v).transpose(0, 1).reshape(T, D))
    return torch.cat(out)


@pytest.mark.parametrize("B", [1, 2])
def test_attention_kernels_at_t2305(B):
    """All three attention kernels at T = 2305 = 72 * 32 + 1 = 18 * 128 + 1 (the straggler-key fold, a last query tile
    holding one query), 12 heads, against float64 with the bounds of the T = 577 cases of test_gpu_kernels.py."""
    from tstar_amd import _lib
    lib = _lib.load()
    T, heads = 2305, 12
    D = heads * 64
    g = torch.Generator().manual_seed(B * 1000 + T + heads)
    qkv = torch.randn(B * T, 3 * D, generator=g)
    st = torch.cuda.current_stream().cuda_stream
    dqkv = qkv.cuda()
    out32 = torch.full((B * T, D), float("nan"), device="cuda")
    _lib.check(lib.tstar_attention_f32(dqkv.data_ptr(), out32.data_ptr(), B, T, heads, 0, None, st))
    torch.cuda.synchronize()
    ref = _attn_ref64(qkv, B, T, heads)
    err_plain = (out32.cpu().double() - ref).abs().max().item()
    assert torch.isfinite(out32).all() and err_plain < 2e-5, err_plain            # test_attention_full's bound
    # the bf16-pipe kernels on the peaky-softmax inputs of test_attention_split / test_attention_x3
    qkv[:, :D] *= 3.0
    dqkv = qkv.cuda()
    ref = _attn_ref64(qkv, B, T, heads)
    outs = {}
    for name in ("f32", "split", "x3"):
        o = torch.full((B * T, D), float("nan"), device="cuda")
        if name == "f32":
            rc = lib.tstar_attention_f32(dqkv.data_ptr(), o.data_ptr(), B, T, heads, 0, None, st)
        elif name == "split":
            rc = lib.tstar_attention_split(dqkv.data_ptr(), o.data_ptr(), B, T, heads, st)
        else:
            rc = lib.tstar_attention_x3(dqkv.data_ptr(), o.data_ptr(), B, T, heads, st)
        _lib.check(rc)
        outs[name] = o
    torch.cuda.synchronize()
    e = {k: (v.cpu().double() - ref) for k, v in outs.items()}
    err = {k: v.abs().max().item() for k, v in e.items()}
    rms = {k: v.pow(2).mean().sqrt().item() for k, v in e.items()}
    print(f"T=2305 B={B}: max err f32 {err['f32']:.3e} split {err['split']:.3e} x3 {err['x3']:.3e}; "
          f"rms f32 {rms['f32']:.3e} x3 {rms['x3']:.3e}")
    assert all(torch.isfinite(v).all() for v in outs.values())
    assert err["split"] < 2e-4 and err["split"] < 60 * err["f32"] + 1e-5
    assert err["x3"] < 2e-5
    assert rms["x3"] <= rms["f32"] * 1.05 + 1e-9
    assert err["x3"] <= 1.5 * err["f32"] + 1e-7


def _legacy_b32_scorer(vb, tb, max_batch, mode):
    """An OwlScorer around a handle from tstar_owl_create (the pre-geometry entry point)."""
    from tstar_amd import _lib, weights as W
    from tstar_amd.owl import OwlScorer, normalize_lut
    s = OwlScorer.__new__(OwlScorer)
    s._torch, s._lib = torch, _lib.load()
    lut = normalize_lut()
    h = C.c_void_p()
    _lib.check(s._lib.tstar_owl_create(C.byref(h), vb.ctypes.data, vb.size, tb.ctypes.data, tb.size, lut.ctypes.data, max_batch,
                                       OwlScorer.WEIGHTS_MODES[mode]), "tstar_owl_create")
    s._h, s.geometry, s.num_patches, s.max_batch = h, W.B32, 576, max_batch
    s.Qs, s._pending, s.device = {}, {}, torch.device("cuda", torch.cuda.current_device())
    assert s._lib.tstar_owl_num_patches(h) == 576
    return s


def _queries():
    from tstar_amd.tokenizer import encode_queries
    ids, am = encode_queries([["couch"], ["tv"], ["chair"], [" "]], "google/owlvit-base-patch32", allow_standin=True)
    return ids, am, [1.0, 0.5, 0.5, 0.5]


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_b32_create_ex_equals_create(mode):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    sd = W.synthetic_state_dict(0)
    vb, tb = W.pack_blob(sd, W.vision_spec()), W.pack_blob(sd, W.text_spec())
    new = OwlScorer(vb, tb, max_batch=3, weights_mode=mode, patch_size=32)
    old = _legacy_b32_scorer(vb, tb, 3, mode)
    ids, am, w = _queries()
    rs = np.random.RandomState(3)
    imgs = torch.from_numpy(rs.randint(0, 256, (3, 380, 800, 3)).astype(np.uint8)).cuda()
    res = []
    for s in (new, old):
        s.set_queries(ids, am, w)
        r = s.score(imgs, 4, 4, want_logits=True)
        torch.cuda.synchronize()
        res.append(r)
    a, b = res
    for f in ("scores", "labels", "boxes", "cell_conf", "cell_mask", "n_kept", "logits", "boxes_cxcywh"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.scores.shape == (3, 576)
    new.close()
    old.close()


def _synthetic_b16(max_batch, mode="f32"):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    sd = W.synthetic_state_dict(0, geometry=W.B16)
    return OwlScorer(W.pack_blob(sd, W.vision_spec(W.B16)), W.pack_blob(sd, W.text_spec()), max_batch=max_batch, weights_mode=mode,
                     patch_size=16)


def _fields(r, b):
    return {f: getattr(r, f)[b].cpu().numpy() for f in ("scores", "labels", "boxes", "cell_conf", "cell_mask", "n_kept")}


def test_b16_chunking_is_bit_identical():
    """B = 5 images through a max_batch 2 handle (chunks of 2, 2 and 1) give the bits of one image at a time; so does a
    handle whose max_batch (300) is past the B/16 chunk cap of 256 images, on a batch of 257 (chunks of 256 and 1)."""
    ids, am, w = _queries()
    rs = np.random.RandomState(11)
    imgs = torch.from_numpy(rs.randint(0, 256, (5, 190, 400, 3)).astype(np.uint8)).cuda()
    s = _synthetic_b16(2)
    s.set_queries(ids, am, w)
    assert s.num_patches == 2304
    batch = s.score(imgs, 2, 3)
    torch.cuda.synchronize()
    batch = [_fields(batch, b) for b in range(5)]
    one = []
    for b in range(5):
        r = s.score(imgs[b:b + 1], 2, 3)
        torch.cuda.synchronize()
        one.append(_fields(r, 0))
    for b in range(5):
        for f in one[b]:
            assert np.array_equal(batch[b][f], one[b][f]), (b, f)
    assert batch[0]["scores"].shape == (2304,) and int(batch[0]["n_kept"]) > 0
    s.close()
    big = _synthetic_b16(300)
    big.set_queries(ids, am, w)
    many = torch.from_numpy(np.random.RandomState(12).randint(0, 256, (257, 64, 96, 3)).astype(np.uint8)).cuda()
    r = big.score(many, 1, 2)
    torch.cuda.synchronize()
    for b in (0, 255, 256):
        r1 = big.score(many[b:b + 1].contiguous(), 1, 2)
        torch.cuda.synchronize()
        got, want = _fields(r, b), _fields(r1, 0)
        for f in want:
            assert np.array_equal(got[f], want[f]), (b, f)
    big.close()


def test_b16_search_teacher_forced_and_painter():
    """TStarSearcher with a B/16 synthetic heuristic (synthetic_video(900), 6x6 grid, K = 8) replayed through the oracle
    searcher: the same sampled seconds, histories and keyframes; the first grid image's cells equal image_grid_score on
    its 2304 recorded detections; with visual history on, the device painter equals the host painter."""
    from oracle import searcher_ref as S
    from oracle.replay import Recorder, replay_through_oracle
    from tstar_amd.interface_heuristic import OWLInterface, Detections, draw_boxes
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    from tstar_amd import weights as W
    N, g, K, seed = 900, 6, 8, 2025
    h = OWLInterface(synthetic_seed=0, max_batch=64, patch_size=16)
    assert h.geometry == W.B16
    rec = Recorder(h)
    s = TStarSearcher(synthetic_video(N, seed=3), h, ["couch"], ["tv", "chair"], search_nframes=K, image_grid_shape=(g, g),
                      search_budget=0.3, confidence_threshold=0.6, rng=np.random.RandomState(seed), keep_visual_history=True)
    frames, ts = s.search()
    assert len(ts) == K
    ref, ts_ref = replay_through_oracle(rec.calls, h.texts, ["couch"], ["tv", "chair"], N, g, K, 0.3, 0.6, seed)
    assert ts_ref == [float(t) for t in ts]
    for i in range(s.iterations):
        assert np.array_equal(np.asarray(s.Score_history[i]), ref.Score_history[i])
        assert np.array_equal(np.asarray(s.non_visiting_history[i]), ref.unvisited_history[i])
        assert np.array_equal(np.asarray(s.P_history[i]), ref.P_history[i])
    first = rec.calls[0]
    assert first["rows"] == g and first["scores"].shape == (1, 2304)
    texts = [list(t) for t in h.texts]
    o2w = {"couch": 1.0, "tv": 0.5, "chair": 0.5}
    keep = first["scores"][0] > np.float32(0.005)
    Hg, Wg = first["images"][0].shape[:2]
    cm, _ = S.image_grid_score(first["boxes"][0][keep], first["labels"][0][keep], first["scores"][0][keep], texts, o2w, Hg, Wg, g, g)
    assert np.array_equal(first["conf"][0].reshape(g, g), cm)
    # visual history: the grid painted on the device (tstar_draw_boxes_np over 2304 detections) against the host painter
    det = Detections(xyxy=first["boxes"][0][keep], confidence=first["scores"][0][keep], class_id=first["labels"][0][keep].astype(np.int64))
    host = draw_boxes(first["images"][0].copy(), det)
    assert len(s.detect_bbox_iters[0][0]) == int(keep.sum())               # the first entry is iteration 0's grid
    assert np.array_equal(s.detect_annotot_iters[0][0], host)
    assert not np.array_equal(host, first["images"][0])                # boxes were painted


def test_b16_lockstep_equals_solo():
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.lockstep import search_lockstep
    from tstar_amd.video import synthetic_video
    h = OWLInterface(synthetic_seed=0, max_batch=16, patch_size=16)
    stores = [synthetic_video(160, seed=31), synthetic_video(120, seed=32)]
    items = [(["couch"], ["tv"], 4), (["dog", "lamp"], [], 3)]

    def make(i):
        t, c, k = items[i]
        return TStarSearcher(stores[i], h, list(t), list(c), search_nframes=k, image_grid_shape=(3, 3), search_budget=0.4,
                             confidence_threshold=0.6, rng=np.random.RandomState(70 + i), keep_visual_history=False)

    solo = []
    for i in range(2):
        s = make(i)
        fr, ts = s.search()
        solo.append((fr, ts, s.score_distribution))
    group = [make(i) for i in range(2)]
    res = search_lockstep(group)
    for i in range(2):
        assert res[i][1] == solo[i][1] and np.array_equal(res[i][0], solo[i][0])
        assert np.array_equal(group[i].score_distribution, solo[i][2])


def test_b16_rejections_before_the_device(ckpt):
    """patch_size that disagrees with the checkpoint, and unsupported patch sizes, raise ValueError; initialize_heuristic
    takes the checkpoint override."""
    from tstar_amd import weights as W
    from tstar_amd.interface_heuristic import OWLInterface, initialize_heuristic
    d, _, _ = ckpt
    with pytest.raises(ValueError, match="disagrees"):
        OWLInterface(model_name_or_path=d, patch_size=32, max_batch=1)
    with pytest.raises(ValueError, match="not supported"):
        OWLInterface(synthetic_seed=0, patch_size=14, max_batch=1)
    h = initialize_heuristic("owl-vit", model_name_or_path=d, max_batch=1)
    assert h.geometry == W.B16 and h.model_name_or_path == d
