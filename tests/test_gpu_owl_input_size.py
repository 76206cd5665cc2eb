"""OWL-ViT at an input size other than the checkpoint's 768 x 768 on the HIP detector path.

* the three attention kernels at token counts that are not 32 n + 1 (a masked last key tile) against float64, with the
  workspace rows behind the last image poisoned, and their bits at T = 577 / 2305 against the CRCs recorded from the commit
  before this feature (tests/golden/attention_t32n1_crc.txt);
* the resampler + im2col against HF's own Pillow image processor at four sizes, bit for bit;
* HF-initialised B/32 and B/16 checkpoints through ``OWLInterface(model_name_or_path=dir, input_size=...)`` against HF's own
  CPU forward with ``interpolate_pos_encoding=True``;
* ``input_size=(768, 768)`` equal to no keyword; chunking and lanes; searches on a (448, 768) heuristic."""
import os

import numpy as np
import pytest
import torch

import owl_input_size_util as U

pytestmark = pytest.mark.gpu

SIZES = [(32, (448, 768)), (32, (384, 800)), (32, (352, 640)), (16, (384, 800))]


# ---------------------------------------------------------------------------------------------------------------- attention
def _run3(lib, qkv_np, B, T, heads, poison=None):
    """The three kernels on qkv [B*T, 3D]; the device buffer holds 64 more rows behind the last image, filled with ``poison``
    (the last image of a chunk sits at the end of the workspace: whatever lies behind it must never reach the result)."""
    from tstar_amd import _lib
    D = heads * 64
    buf = torch.zeros((B * T + 64, 3 * D), device="cuda")
    if poison is not None:
        buf[B * T:] = poison
    buf[:B * T] = torch.from_numpy(qkv_np).cuda()
    outs = {}
    for name in U.ATTN_KERNELS:
        o = torch.full((B * T, D), float("nan"), device="cuda")
        _lib.check(U.run_attention(lib, name, buf, o, B, T, heads))
        outs[name] = o
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in outs.items()}


MIN_ELEMENTS = 2 * 577 * 3 * 64          # 221568: the smallest T = 577 case of tests/test_gpu_kernels.py::test_attention_x3, (B, T, heads) = (2, 577, 3)


def _shape_for(T):
    """(B, heads) of a case.  The x3-against-f32 gate compares two rms ESTIMATES over the B T 64 heads output elements, each with
    a relative sampling error of about 1 / sqrt(2 N); 5 % means something only when N is large.  The T = 577 cases that the
    bounds come from have at least MIN_ELEMENTS elements, so every case here gets as many: B grows as T shrinks (145 images
    at T = 2).  Measured while writing this test, T = 2, 12 heads, four seeds each: rms(x3) / rms(f32) = 0.88 .. 1.07 over 3072
    elements (B = 2), 0.90 .. 1.00 over 49152 (B = 32), 0.97 .. 1.00 over 786432 (B = 512): the spread is the estimator's, the
    kernels' errors are equal.  Large T: fewer heads, the float64 reference holds T^2 x heads scores per image."""
    heads = 12 if T <= 400 else 3
    B = max(1 if T > 2000 else 2, -(-MIN_ELEMENTS // (T * heads * 64)))
    return B, heads


@pytest.mark.parametrize("T", [2, 33, 64, 100, 221, 301, 337, 1201, 3601])
def test_attention_any_token_count(T):
    """Bounds of tests/test_gpu_kernels.py at T = 577: the f32 kernel within 2e-5 on unit-normal inputs; on the peaky-softmax
    inputs (q x 3) the split kernel within 2e-4 and 60 x the f32 kernel's error + 1e-5, the x3 kernel within 2e-5 and no worse
    than the f32 kernel (rms x 1.05 + 1e-9, max x 1.5 + 1e-7).  Rows behind the last image filled with NaN: same bits."""
    from tstar_amd import _lib
    lib = _lib.load()
    B, heads = _shape_for(T)
    D = heads * 64
    qkv = U.attention_input(T, B, heads, seed=1000 + T)
    out = _run3(lib, qkv, B, T, heads)
    ref = U.attn_ref64(torch.from_numpy(qkv), B, T, heads)
    err_plain = (out["f32"].double() - ref).abs().max().item()
    print(f"T={T}: f32 kernel, unit-normal input: max err {err_plain:.3e}")
    assert torch.isfinite(out["f32"]).all() and err_plain < 2e-5, err_plain
    qkv[:, :D] *= 3.0
    out = _run3(lib, qkv, B, T, heads)
    nan = _run3(lib, qkv, B, T, heads, poison=float("nan"))
    ref = U.attn_ref64(torch.from_numpy(qkv), B, T, heads)
    e = {k: v.double() - ref for k, v in out.items()}
    err = {k: v.abs().max().item() for k, v in e.items()}
    rms = {k: v.pow(2).mean().sqrt().item() for k, v in e.items()}
    print(f"T={T} B={B} heads={heads}: max err f32 {err['f32']:.3e} split {err['split']:.3e} x3 {err['x3']:.3e}; "
          f"rms f32 {rms['f32']:.3e} x3 {rms['x3']:.3e}")
    for k in U.ATTN_KERNELS:
        assert torch.isfinite(out[k]).all(), k
        assert torch.equal(out[k].view(torch.int32), nan[k].view(torch.int32)), k
    assert err["f32"] < 2e-5
    assert err["split"] < 2e-4 and err["split"] < 60 * err["f32"] + 1e-5
    assert err["x3"] < 2e-5
    assert rms["x3"] <= rms["f32"] * 1.05 + 1e-9
    assert err["x3"] <= 1.5 * err["f32"] + 1e-7


@pytest.mark.parametrize("T", [221, 301, 337, 1201, 3601])
def test_attention_dominant_key_in_the_masked_tile(T):
    """A key INSIDE the last, partial key tile dominates the softmax late (an early big one before it): the online-softmax
    rescale across the masked tile, with the bounds of the spiked tests at T = 577 (f32 / x3 5e-5, split 2e-2)."""
    from tstar_amd import _lib
    lib = _lib.load()
    B, heads = 1, 2
    D = heads * 64
    assert T % 32 not in (0, 1)
    spike = (T // 32) * 32 + (T % 32) // 2                    # inside the partial tile, valid keys on both sides
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(B * T, 3 * D, generator=g)
    qkv[spike, D:2 * D] *= 40.0
    qkv[3, D:2 * D] *= 25.0
    qkv[T // 2, D:2 * D] *= 30.0
    ref = U.attn_ref64(qkv, B, T, heads)
    out = _run3(lib, qkv.numpy(), B, T, heads, poison=float("nan"))
    err = {k: (v.double() - ref).abs().max().item() for k, v in out.items()}
    print(f"T={T} spiked key {spike}: max err f32 {err['f32']:.3e} split {err['split']:.3e} x3 {err['x3']:.3e}")
    assert all(torch.isfinite(v).all() for v in out.values())
    assert err["f32"] < 5e-5 and err["x3"] < 5e-5 and err["split"] < 2e-2


def test_attention_t32n1_bits_are_the_parents():
    got, want = U.attention_crcs(), U.read_crc_golden()
    assert set(want) == {(k, T) for k in U.ATTN_KERNELS for T in U.CRC_CASES}
    assert got == want, U.format_crcs(got)


# ------------------------------------------------------------------------------------------------------------ pre-processing
@pytest.mark.parametrize("H,Wd", [(285, 600), (1520, 3200), (97, 301)])
@pytest.mark.parametrize("patch,size", SIZES)
def test_preprocess_is_hfs_processor_bit_for_bit(patch, size, H, Wd):
    from PIL import Image
    from tstar_amd.owl import OwlScorer
    h, w = size
    gh, gw, P = h // patch, w // patch, patch
    rs = np.random.RandomState(H * 7 + Wd + h)
    img = rs.randint(0, 256, (2, H, Wd, 3)).astype(np.uint8)
    s = OwlScorer.synthetic(0, max_batch=2, with_text=False, patch_size=patch, input_size=size)
    assert s.num_patches == gh * gw
    u8, pat = s.debug_preprocess(torch.from_numpy(img).cuda())
    torch.cuda.synchronize()
    assert u8.shape == (2, h, w, 3) and pat.shape == (2 * gh * gw, 3 * P * P)
    pat = pat.cpu().numpy().reshape(2, gh * gw, 3 * P * P)
    for b in range(2):
        ref_u8 = np.asarray(Image.fromarray(img[b]).resize((w, h), Image.BICUBIC))          # HF's PilBackend.resize statement
        assert np.array_equal(u8[b].cpu().numpy(), ref_u8), b
        px = U.hf_pixels(img[b], size)
        assert px.shape == (3, h, w)
        x = px.reshape(3, gh, P, gw, P).transpose(1, 3, 0, 2, 4).reshape(gh * gw, 3 * P * P)
        assert np.array_equal(pat[b].view(np.uint32), np.ascontiguousarray(x).view(np.uint32)), b
    s.close()


# --------------------------------------------------------------------------------------------------------- checkpoint parity
@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    from transformers import CLIPTokenizer
    out = {}
    for patch in (32, 16):
        d = str(tmp_path_factory.mktemp(f"owlvit_b{patch}_ckpt"))
        m = U.make_checkpoint_dir(d, patch, seed=2)
        out[patch] = (d, m, CLIPTokenizer.from_pretrained(d, local_files_only=True))
    return out


def _test_images():
    from oracle import resize_ref as R
    from tstar_amd.video import synthetic_frames_numpy
    out = []
    for k, (H_, W_) in enumerate([(285, 600), (1520, 3200)]):
        out.append(R.cv_bilinear_resize(synthetic_frames_numpy([7 + k], 40, 360, 640, seed=5)[0], W_, H_))
    return out


_REF = {}


@pytest.mark.parametrize("mode", ["f32", "f32x3", "bf16", "bf16_exact"])
@pytest.mark.parametrize("patch,size", [(32, (448, 768)), (32, (384, 800)), (16, (384, 800)), (16, (448, 768))])
def test_checkpoint_matches_hf_at_input_size(ckpts, patch, size, mode):
    """tests/test_gpu_owl_b16.py::test_b16_checkpoint_matches_hf at another input size: HF's CPU forward with
    ``interpolate_pos_encoding=True`` on pixels from HF's own image processor at that size.  Text embeds within 1e-5, dense
    scores within 1e-3, boxes within 1e-2 px (observed maxima printed), unsaturated reference; a 285x600 frame and a 1520x3200
    grid image.  B/16 at (448, 768) has T = 1345 = 32 n + 1: the geometry without the masked key tile."""
    import copy
    from tstar_amd import weights as W
    from tstar_amd.interface_heuristic import OWLInterface
    d, m, tok = ckpts[patch]
    h = OWLInterface(model_name_or_path=d, max_batch=2, weights_dtype=mode, input_size=size)
    np_ = (size[0] // patch) * (size[1] // patch)
    assert h.geometry == W.with_input_size(W.geometry_for_patch(patch), size) and h.geometry.checkpoint in (W.B32, W.B16)
    assert h.scorer.num_patches == np_ == h.geometry.npatch
    h.reparameterize_object_list(["couch"], ["tv", "remote control"])
    names = [t[0] for t in h.texts]
    ref_model = m
    if mode in ("bf16", "bf16_exact"):
        ref_model = _REF.get(("bf16_model", patch))
        if ref_model is None:
            sd = W.round_weights_to_bf16({k: v.numpy() for k, v in m.state_dict().items()})
            ref_model = copy.deepcopy(m)
            ref_model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            _REF[("bf16_model", patch)] = ref_model
    wkey = "bf16" if mode.startswith("bf16") else "f32"
    for k, img in enumerate(_test_images()):
        H_, W_ = img.shape[:2]
        key = (wkey, patch, size, k)
        if key not in _REF:
            _REF[key] = U.hf_detect_at(ref_model, tok, img, names, size)
        ref = _REF[key]
        if k == 0:
            assert np.abs(h.scorer.get_query_embeds() - ref["text_embeds"]).max() < 1e-5
        det = h.inference_detector([img])[0]
        r = h.scorer.score(torch.from_numpy(img).cuda().unsqueeze(0), 1, 1)
        dense = r.scores[0].cpu().numpy()
        assert dense.shape == (np_,)
        err = float(np.abs(dense - ref["dense_scores"]).max())
        assert 0.05 < ref["dense_scores"].min() and ref["dense_scores"].max() < 0.95       # not a saturated comparison
        assert len(det) == len(ref["scores"]) == np_                      # threshold 0.005: every patch kept, patch order
        assert np.abs(det.confidence - ref["scores"]).max() < 1e-3
        box_err = float(np.abs(det.xyxy - ref["xyxy"]).max())
        wh = ref["xyxy"][:, 2:] - ref["xyxy"][:, :2]
        assert wh.min() > 1.0 and wh.max() < max(H_, W_)                # real boxes, not saturated sigmoids
        print(f"B/{patch} at {size[0]}x{size[1]} {mode} {H_}x{W_}: max |score - HF| = {err:.2e}, max |box - HF| = {box_err:.2e} px")
        assert err < 1e-3, err
        assert box_err < 1e-2, box_err
    del h


# ------------------------------------------------------------------------------------------- default, chunking, lanes
def _queries():
    from tstar_amd.tokenizer import encode_queries
    ids, am = encode_queries([["couch"], ["tv"], ["chair"], [" "]], "google/owlvit-base-patch32", allow_standin=True)
    return ids, am, [1.0, 0.5, 0.5, 0.5]


def _synthetic(max_batch, mode="f32", patch=32, size=None):
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    g = W.with_input_size(W.geometry_for_patch(patch), size)
    sd = W.synthetic_state_dict(0, geometry=g)
    s = OwlScorer(W.pack_blob(sd, W.vision_spec(g), g), W.pack_blob(sd, W.text_spec()), max_batch=max_batch, weights_mode=mode,
                  patch_size=patch, input_size=size)
    s.set_queries(*_queries())
    return s


FIELDS = ("scores", "labels", "boxes", "cell_conf", "cell_mask", "n_kept")


def _fields(r, b):
    return {f: getattr(r, f)[b].cpu().numpy() for f in FIELDS}


@pytest.mark.parametrize("mode", ["f32", "f32x3", "bf16"])
def test_default_size_keyword_changes_no_bit(mode):
    rs = np.random.RandomState(3)
    imgs = torch.from_numpy(rs.randint(0, 256, (3, 380, 800, 3)).astype(np.uint8)).cuda()
    res = []
    for size in (None, (768, 768)):
        s = _synthetic(3, mode, 32, size)
        assert s.num_patches == 576
        res.append(s.score(imgs, 4, 4, want_logits=True))
        torch.cuda.synchronize()
        s.close()
    a, b = res
    for f in FIELDS + ("logits", "boxes_cxcywh"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_interface_default_size_from_keyword_and_environment(monkeypatch):
    from tstar_amd import weights as W
    from tstar_amd.interface_heuristic import OWLInterface
    monkeypatch.delenv("TSTAR_INPUT_SIZE", raising=False)
    img = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (1, 285, 600, 3)).astype(np.uint8)).cuda()
    out = []
    for kw, env in (({}, None), (dict(input_size=(768, 768)), "448x768"), ({}, "448x768"), (dict(input_size=(448, 768)), "rubbish")):
        if env is None:
            monkeypatch.delenv("TSTAR_INPUT_SIZE", raising=False)
        else:
            monkeypatch.setenv("TSTAR_INPUT_SIZE", env)
        h = OWLInterface(synthetic_seed=0, max_batch=1, **kw)
        h.reparameterize_object_list(["couch"], ["tv"])
        r = h.score_batch(img, 1, 1)
        torch.cuda.synchronize()
        out.append((h.geometry, r.scores.cpu(), r.boxes.cpu()))
        del h
    assert out[0][0] == out[1][0] == W.B32 and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])     # the keyword wins
    assert out[2][0] == out[3][0] == W.with_input_size(W.B32, (448, 768)) and out[2][1].shape == (1, 336)
    assert torch.equal(out[2][1], out[3][1]) and torch.equal(out[2][2], out[3][2])


def test_chunking_and_lanes_are_bit_identical():
    """(448, 768) at B/32, T = 337: B = 5 through a max_batch 2 handle (chunks of 2, 2, 1) gives the bits of one image at a
    time, in both weight modes whose attention kernels differ; lane 1 gives the bits of lane 0.  B/16 at (960, 960), T = 3601:
    a max_batch 200 handle is past the chunk limit of 164 images (590848 rows / 3601), a batch of 165 runs as 164 + 1."""
    rs = np.random.RandomState(11)
    imgs = torch.from_numpy(rs.randint(0, 256, (5, 190, 400, 3)).astype(np.uint8)).cuda()
    for mode in ("f32", "f32x3"):
        s = _synthetic(2, mode, 32, (448, 768))
        assert s.num_patches == 336
        batch = s.score(imgs, 2, 3)
        torch.cuda.synchronize()
        batch = [_fields(batch, b) for b in range(5)]
        lane1 = s.score(imgs, 2, 3, lane=1)
        torch.cuda.synchronize()
        for b in range(5):
            r = s.score(imgs[b:b + 1], 2, 3)
            torch.cuda.synchronize()
            one, l1 = _fields(r, 0), _fields(lane1, b)
            for f in one:
                assert np.array_equal(batch[b][f], one[f]), (mode, b, f)
                assert np.array_equal(l1[f], one[f]), (mode, "lane 1", b, f)
        assert batch[0]["scores"].shape == (336,) and int(batch[0]["n_kept"]) > 0
        s.close()
    big = _synthetic(200, "f32x3", 16, (960, 960))
    assert big.num_patches == 3600
    many = torch.from_numpy(np.random.RandomState(12).randint(0, 256, (165, 64, 96, 3)).astype(np.uint8)).cuda()
    r = big.score(many, 1, 2)
    torch.cuda.synchronize()
    for b in (0, 163, 164):
        r1 = big.score(many[b:b + 1].contiguous(), 1, 2)
        torch.cuda.synchronize()
        got, want = _fields(r, b), _fields(r1, 0)
        for f in want:
            assert np.array_equal(got[f], want[f]), (b, f)
    big.close()


# -------------------------------------------------------------------------------------------------------------------- search
def test_search_teacher_forced_and_painter_at_448x768():
    """tests/test_gpu_owl_b16.py::test_b16_search_teacher_forced_and_painter on a (448, 768) B/32 heuristic: 336 detections."""
    from oracle import searcher_ref as S
    from oracle.replay import Recorder, replay_through_oracle
    from tstar_amd import _lib
    from tstar_amd.interface_heuristic import OWLInterface, Detections, draw_boxes
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    N, g, K, seed = 900, 6, 8, 2025
    h = OWLInterface(synthetic_seed=0, max_batch=64, input_size=(448, 768))
    assert h.geometry.npatch == 336 and _lib.load().tstar_owl_num_patches(h.scorer._h) == 336 == h.scorer.num_patches
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
    assert first["rows"] == g and first["scores"].shape == (1, 336)
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
    return TStarSearcher(store, h, list(targets), list(cues), search_nframes=k, image_grid_shape=(3, 3), search_budget=0.4,
                         confidence_threshold=thr, rng=np.random.RandomState(seed), keep_visual_history=False)


@pytest.mark.parametrize("thr", [0.05, 0.6])
def test_solo_search_equals_the_sequential_loop_at_448x768(monkeypatch, thr):
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.video import synthetic_video
    h = OWLInterface(synthetic_seed=0, max_batch=16, input_size=(448, 768), weights_dtype="f32x3")
    store = synthetic_video(700, seed=9)
    res = []
    for sequential in (False, True):
        if sequential:
            monkeypatch.setenv("TSTAR_SOLO_SEQUENTIAL", "1")
        else:
            monkeypatch.delenv("TSTAR_SOLO_SEQUENTIAL", raising=False)
        s = _make_searcher(h, store, ["couch"], ["chair"], 4, 123, thr)
        frames, ts = s.search()
        res.append((frames, ts, np.asarray(s.score_distribution), s.iterations, s.frames_scored,
                    [np.asarray(x) for x in s.Score_history], [np.asarray(x) for x in s.P_history]))
    a, b = res
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[3:5] == b[3:5]
    assert len(a[5]) == len(b[5]) and all(np.array_equal(x, y) for x, y in zip(a[5], b[5]))
    assert all(np.array_equal(x, y) for x, y in zip(a[6], b[6]))


def test_lockstep_group_of_three_equals_solo_at_448x768():
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.lockstep import search_lockstep
    from tstar_amd.video import synthetic_video
    h = OWLInterface(synthetic_seed=0, max_batch=16, input_size=(448, 768))
    stores = [synthetic_video(160, seed=31), synthetic_video(120, seed=32), synthetic_video(200, seed=33)]
    items = [(["couch"], ["tv"], 4), (["dog", "lamp"], [], 3), (["tv"], ["chair", "couch"], 5)]

    def make(i):
        t, c, k = items[i]
        return _make_searcher(h, stores[i], t, c, k, 70 + i)

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
