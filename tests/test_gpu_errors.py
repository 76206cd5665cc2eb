"""Error behaviour of the C ABI and the Python mirror: bad arguments return TSTAR_ERR_ARG / raise with a
message (like the reference raises ValueError), nothing crashes, nothing falls back to the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from tstar_amd import _lib
    from tstar_amd.interface_heuristic import OWLInterface
    return _lib, _lib.load(), OWLInterface(synthetic_seed=0, max_batch=2)


def test_owl_score_argument_validation(env):
    L, lib, h = env
    h.reparameterize_object_list(["couch"], [])
    img = torch.zeros((1, 95, 200, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="cuda uint8"):
        h.scorer.score(img.float(), 1, 1)
    with pytest.raises(ValueError, match="cuda uint8"):
        h.scorer.score(img[0], 1, 1)
    with pytest.raises(ValueError, match="at least 1x1"):
        h.scorer.score(img, 0, 1)
    with pytest.raises(L.TStarHipError, match="1..4096 cells"):
        h.scorer.score(img, 100, 100)
    with pytest.raises(ValueError, match="one slot per image"):
        h.scorer.score(img, 1, 1, image_sets=[0, 0])
    with pytest.raises(L.TStarHipError, match="query_set must be in 0..63"):
        h.scorer.score(img, 1, 1, image_sets=[64])
    r = h.scorer.score(img, 1, 1)                                   # still healthy afterwards
    assert torch.isfinite(r.scores).all()


def test_query_limits(env):
    L, lib, h = env
    ids = np.zeros((33, 16), np.int32); ids[:, 0] = 49406; ids[:, 1] = 49407
    with pytest.raises(L.TStarHipError, match="Q must be in 1..32"):
        h.scorer.set_queries(ids, np.ones_like(ids), [1.0] * 33)
    bad = np.full((1, 16), 60000, np.int32)
    with pytest.raises(L.TStarHipError, match="token id out of range"):
        h.scorer.set_queries(bad, np.ones_like(bad), [1.0])
    with pytest.raises(ValueError, match=r"\[Q,16\]"):
        h.scorer.set_queries(np.zeros((2, 8), np.int32), np.zeros((2, 8), np.int32), [1.0, 1.0])
    # 32 queries (the maximum) work end to end
    names = [f"thing{i}" for i in range(31)]
    h.reparameterize_object_list(names[:1], names[1:])
    assert h.scorer.Q == 32
    r = h.scorer.score(torch.zeros((1, 95, 200, 3), dtype=torch.uint8, device="cuda"), 1, 1)
    assert int(r.labels.max()) < 32


def test_searcher_state_validation(env):
    L, lib, h = env
    from tstar_amd.interface_searcher import _DeviceState
    with pytest.raises(L.TStarHipError, match="n_frames must be in"):
        _DeviceState(0, 1e-6, 0.1)
    st = _DeviceState(50, 1e-6, 0.1)
    conf = torch.zeros(4, dtype=torch.float64, device="cuda")
    with pytest.raises(L.TStarHipError, match="second out of range"):
        st.apply_grid([0, 1, 2, 50], conf)
    with pytest.raises(L.TStarHipError, match="bad sample count"):
        st.sampler_prep(51, 0.1)
    with pytest.raises(L.TStarHipError, match="bad spline"):
        st.set_spline(np.zeros(4), np.zeros(4), 3)
    with pytest.raises(L.TStarHipError, match="index out of range"):
        st.exclude([60])


def test_searcher_python_level_errors(env):
    L, lib, h = env
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import FrameStore, synthetic_video
    st = synthetic_video(20, seed=1)
    s = TStarSearcher(st, h, ["a"], [], search_nframes=30, image_grid_shape=(2, 2), search_budget=0.5,
                      rng=np.random.RandomState(0), keep_visual_history=False)
    with pytest.raises(ValueError, match="larger sample than population"):       # numpy's message, as the reference
        s.pop_frames(None, 30)
    # grid larger than the video: the reference clamps the sample count and then fails in create_image_grid
    s2 = TStarSearcher(st, h, ["a"], [], image_grid_shape=(5, 5), rng=np.random.RandomState(0))
    with pytest.raises(ValueError, match="Frame count does not match grid dimensions"):
        s2.search()
    with pytest.raises(ValueError, match="fewer frames"):
        TStarSearcher(FrameStore(st.frames[:5], 1.0, raw_total_frames=20), h, ["a"], [])
    with pytest.raises(ValueError, match="fmt must be"):
        FrameStore(st.frames, 1.0, fmt="yuv")
    # no targets: the loop never runs, keyframes come from the flat initial scores (reference behaviour)
    s3 = TStarSearcher(st, h, [], ["tv"], search_nframes=3, image_grid_shape=(2, 2), rng=np.random.RandomState(1))
    fr, ts = s3.search()
    assert len(ts) == 3 and s3.iterations == 0 and s3.P_history == []


def test_kernel_entry_point_validation(env):
    L, lib, h = env
    d = torch.zeros(1024, device="cuda")
    assert lib.tstar_layernorm_f32(d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), 1, 300, None) == 1
    assert b"512 or 768" in lib.tstar_last_error()
    assert lib.tstar_attention_f32(d.data_ptr(), d.data_ptr(), 1, 4, 1, 1, None, None) == 1      # mode 1 needs a mask
    assert lib.tstar_gemm_f32(d.data_ptr(), d.data_ptr(), d.data_ptr(), None, None, 0, 128, 32, 0, None) == 1
    assert lib.tstar_gemm_f32_cfg(d.data_ptr(), d.data_ptr(), d.data_ptr(), None, None, 8, 128, 32, 0, 9, None) == 1
    assert lib.tstar_topk_seconds(d.data_ptr(), 10, 5, 3, 1, d.data_ptr(), None) == 1
    assert lib.tstar_ssim_pairwise(None, 1, None, 1, 4, 4, None, None, None) == 1
    n = C.c_longlong(); ms = C.c_double(); fl = C.c_double()
    assert lib.tstar_prof_read(7, C.byref(n), C.byref(ms), C.byref(fl)) == 1


def test_round3_entry_points_validate_their_arguments(env):
    """The entries added in round 3: marker kernels, algorithmic-byte counters, prepared-weights bf16 GEMM, RCCL availability."""
    L, lib, h = env
    st = torch.cuda.current_stream().cuda_stream
    assert lib.tstar_prof_mark(2, st) == 1 and b"0 (begin) or 1 (end)" in lib.tstar_last_error()
    assert lib.tstar_prof_mark(0, st) == 0 and lib.tstar_prof_mark(1, st) == 0
    by = C.c_double(-1.0)
    assert lib.tstar_prof_read_bytes(7, C.byref(by)) == 1
    L.check(lib.tstar_prof_enable(1))
    A = torch.randn(256, 64, device="cuda")
    Wb = torch.randn(128, 64, device="cuda").to(torch.bfloat16)
    Cc = torch.empty(256, 128, device="cuda")
    assert lib.tstar_gemm_bf16w_pre(A.data_ptr(), Wb.data_ptr(), Cc.data_ptr(), None, None, 256, 128, 64, 0, 4, -1, st) == 1     # a_terms 2 or 3
    assert lib.tstar_gemm_bf16w_pre(A.data_ptr(), Wb.data_ptr(), Cc.data_ptr(), None, None, 256, 100, 64, 0, 2, -1, st) == 1     # N % 128
    L.check(lib.tstar_gemm_bf16w_pre(A.data_ptr(), Wb.data_ptr(), Cc.data_ptr(), None, None, 256, 128, 64, 0, 2, -1, st))
    L.check(lib.tstar_gemm_bf16w_pre(A.data_ptr(), Wb.data_ptr(), Cc.data_ptr(), None, None, 256, 128, 64, 0, 3, -1, st))
    torch.cuda.synchronize()
    ref = A.double() @ Wb.double().t()
    assert (Cc.double() - ref).abs().max().item() < 1e-4
    n, ms, fl = C.c_longlong(0), C.c_double(0), C.c_double(0)
    L.check(lib.tstar_prof_read(0, C.byref(n), C.byref(ms), C.byref(fl)))
    L.check(lib.tstar_prof_read_bytes(0, C.byref(by)))
    na, fa = C.c_longlong(0), C.c_double(0)
    L.check(lib.tstar_prof_read_totals(0, C.byref(na), C.byref(fa)))
    assert lib.tstar_prof_read_totals(9, C.byref(na), C.byref(fa)) == 1
    assert na.value == 2 and fa.value == fl.value                                         # stride 1: every launch is sampled
    L.check(lib.tstar_prof_enable(0))
    assert n.value == 2 and fl.value == 2 * 2.0 * 256 * 128 * 64
    assert by.value == 2 * (4.0 * 256 * 64 + 2.0 * 128 * 64 + 4.0 * 256 * 128)            # A (f32) + W (bf16) + C, per launch
    assert lib.tstar_comm_available() == 0                                                # torch's RCCL is loadable on a GPU box


def test_owl_tail_diagnostic_entries_validate_their_arguments(env):
    """tstar_owl_debug_heads / tstar_owl_debug_merge / tstar_cell_reduce: one case per refusal; nothing is launched on a refusal and
    the handle is healthy afterwards."""
    L, lib, h = env
    h.reparameterize_object_list(["couch"], [])
    sc = h.scorer
    sc.get_query_embeds()                                    # slot 0's recorded queries go through the text tower now
    sc.set_query_embeds(np.eye(3, 512, dtype=np.float32), [1, 1, 1], [1.0, 0.5, 0.5], slot=1)      # a set of another size than slot 0's
    st = torch.cuda.current_stream().cuda_stream
    npatch, B = sc.num_patches, 2
    f = torch.zeros((B * npatch, 768), device="cuda")
    c = torch.zeros((B * npatch, 512), device="cuda")
    x = torch.zeros((B * (npatch + 1), 768), device="cuda")
    o = torch.full((B * npatch, 4), 7.0, device="cuda")
    lab = torch.full((B * npatch,), 7, dtype=torch.int32, device="cuda")
    big = torch.zeros((B * npatch, 32), device="cuda")
    sco = torch.full((B * npatch,), 7.0, device="cuda")
    held = []                                                # the host arrays the calls below point into

    def sets(*v):
        held.append(np.ascontiguousarray(v, dtype=np.int32))
        return held[-1].ctypes.data

    def heads(hd=sc._h, feats=f.data_ptr(), cls=c.data_ptr(), boxh=f.data_ptr(), b=B, H=95, W=200, s=None, scores=sco.data_ptr(), labels=lab.data_ptr(),
              xyxy=o.data_ptr(), logits=None, cxcywh=None, oh=None, ob=None):
        return lib.tstar_owl_debug_heads(hd, feats, cls, boxh, b, H, W, s, scores, labels, xyxy, logits, cxcywh, oh, ob, st)

    for bad, code, msg in ((dict(hd=None), 1, b"null argument"), (dict(feats=None), 1, b"null argument"), (dict(cls=None), 1, b"null argument"),
                           (dict(boxh=None), 1, b"null argument"), (dict(scores=None), 1, b"null argument"), (dict(labels=None), 1, b"null argument"),
                           (dict(xyxy=None), 1, b"null argument"), (dict(b=0), 1, b"B must be in 1..max_batch"), (dict(b=3), 1, b"B must be in 1..max_batch"),
                           (dict(H=0), 1, b"empty image"), (dict(s=sets(0, 64)), 1, b"query_set must be in 0..63"),
                           (dict(s=sets(0, 9)), 3, b"no queries installed"), (dict(s=sets(0, 1), logits=big.data_ptr()), 1, b"same query count"),
                           (dict(oh=f.data_ptr(), ob=o.data_ptr()), 1, b"objectness needs an OWLv2 handle"),
                           (dict(oh=f.data_ptr()), 1, b"go together")):
        assert heads(**bad) == code and msg in lib.tstar_last_error(), (bad, lib.tstar_last_error())
    for args, msg in (((None, x.data_ptr(), B, 0, f.data_ptr()), b"null argument"), ((sc._h, None, B, 0, f.data_ptr()), b"null argument"),
                      ((sc._h, x.data_ptr(), B, 0, None), b"null argument"), ((sc._h, x.data_ptr(), 0, 0, f.data_ptr()), b"B must be in 1..max_batch"),
                      ((sc._h, x.data_ptr(), 3, 1, f.data_ptr()), b"B must be in 1..max_batch")):
        assert lib.tstar_owl_debug_merge(*args, st) == 1 and msg in lib.tstar_last_error(), (args, lib.tstar_last_error())
    torch.cuda.synchronize()
    assert (o == 7.0).all() and (sco == 7.0).all() and (lab == 7).all() and not f.any() and not x.any()      # nothing ran
    wts = np.full((2, 32), 0.5)
    conf = torch.full((B, 4), -1.0, dtype=torch.float64, device="cuda")
    mask = torch.full((B, 4), -1, dtype=torch.int32, device="cuda")
    kept = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    s1 = torch.full((B, npatch), 0.5, device="cuda")

    def cells(scores=s1.data_ptr(), labels=lab.data_ptr(), xyxy=o.data_ptr(), w=wts.ctypes.data, n_sets=2, s=None, b=B, n=npatch, W=200, H=95, rows=2, cols=2,
              cf=conf.data_ptr(), mk=mask.data_ptr(), kp=kept.data_ptr()):
        return lib.tstar_cell_reduce(scores, labels, xyxy, w, n_sets, s, b, n, W, H, rows, cols, 0.005, cf, mk, kp, st)

    for bad, msg in ((dict(scores=None), b"null argument"), (dict(labels=None), b"null argument"), (dict(xyxy=None), b"null argument"),
                     (dict(w=None), b"null argument"), (dict(cf=None), b"null argument"), (dict(mk=None), b"null argument"), (dict(kp=None), b"null argument"),
                     (dict(b=0), b"empty batch or image"), (dict(n=0), b"empty batch or image"), (dict(W=0), b"empty batch or image"),
                     (dict(n_sets=0), b"n_sets must be in 1..64"), (dict(n_sets=65), b"n_sets must be in 1..64"), (dict(s=sets(0, 2)), b"image set out of range"),
                     (dict(rows=0), b"1..4096 cells"), (dict(rows=1, cols=4097), b"1..4096 cells")):
        assert cells(**bad) == 1 and msg in lib.tstar_last_error(), (bad, lib.tstar_last_error())
    torch.cuda.synchronize()
    assert (conf == -1.0).all() and (mask == -1).all() and (kept == -1).all()                    # nothing ran
    # healthy afterwards: both weight rows, labels 7 everywhere, every box the point (7, 7) of cell 0
    assert cells(s=sets(1, 0)) == 0
    torch.cuda.synchronize()
    assert kept.tolist() == [npatch, npatch] and conf[:, 0].tolist() == [0.25, 0.25] and (conf[:, 1:] == 0).all() and (mask[:, 0] == 1 << 7).all()
    assert heads(cxcywh=big.data_ptr()) == 0 and lib.tstar_owl_debug_merge(sc._h, x.data_ptr(), B, 1, f.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o).all() and torch.isfinite(sco).all() and int(lab.max()) < sc.Q and torch.isfinite(f).all() and x[0].any() and not x[1].any()


def test_owl_front_diagnostic_entries_validate_their_arguments(env):
    """tstar_gemm_patch_embed / tstar_owl_debug_embed / tstar_owl_debug_text: one case per refusal, each message names its entry;
    nothing is launched on a refusal and the entries work afterwards."""
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    L, lib, h = env
    sc = h.scorer
    st = torch.cuda.current_stream().cuda_stream
    B, npatch, N, K = 2, 3, 256, 64
    A = torch.ones((B * npatch, K), device="cuda")
    Wt = torch.ones((N, K), device="cuda")
    pos = torch.ones((npatch + 1, N), device="cuda")
    X = torch.full((B * (npatch + 1), N), 7.0, device="cuda")

    def patch(a=A.data_ptr(), w=Wt.data_ptr(), x=X.data_ptr(), p=pos.data_ptr(), b=B, n=npatch, N=N, K=K, mode=0, cfg=-1):
        return lib.tstar_gemm_patch_embed(a, w, x, p, b, n, N, K, mode, cfg, st)

    for bad, msg in ((dict(a=None), b"null argument"), (dict(w=None), b"null argument"), (dict(x=None), b"null argument"), (dict(p=None), b"null argument"),
                     (dict(b=0), b"B and np must be at least 1"), (dict(n=0), b"B and np must be at least 1"), (dict(b=1 << 30, n=3), b"do not fit an int"),
                     (dict(mode=2), b"unknown weights_mode"), (dict(mode=5), b"unknown weights_mode"), (dict(K=48), b"multiple of 32"), (dict(K=0), b"multiple of 32"),
                     (dict(N=192), b"N must be a multiple of 128"), (dict(N=0), b"multiple of 32"), (dict(cfg=7), b"tile_cfg must be -1..6"),
                     (dict(cfg=-2), b"tile_cfg must be -1..6"), (dict(cfg=6), b"tile_cfg 6"), (dict(mode=4, cfg=6), b"tile_cfg 6"),
                     (dict(mode=1, cfg=6), b"tile_cfg 6")):        # two-term mode, but no full 128-row panel in 6 rows
        assert patch(**bad) == 1 and b"tstar_gemm_patch_embed" in lib.tstar_last_error() and msg in lib.tstar_last_error(), (bad, lib.tstar_last_error())
    torch.cuda.synchronize()
    assert (X == 7.0).all()                                  # nothing ran
    for mode in (0, 1, 3, 4):
        assert patch(mode=mode) == 0
        torch.cuda.synchronize()
        assert (X.view(B, npatch + 1, N)[:, 0] == 7.0).all() and (X.view(B, npatch + 1, N)[:, 1:] == K + 1.0).all()
        X.fill_(7.0)

    pk, ntok = 3 * 32 * 32, sc.num_patches + 1
    P = torch.zeros((2 * sc.num_patches, pk), device="cuda")
    x = torch.full((2 * ntok, 768), 7.0, device="cuda")
    text_only = OwlScorer(None, W.pack_blob(W.synthetic_state_dict(0, "text"), W.text_spec()), max_batch=1)
    vision_only = OwlScorer.synthetic(0, max_batch=1, with_text=False, input_size=(64, 96))
    for args, code, msg in (((None, P.data_ptr(), 2, 0, x.data_ptr()), 1, b"null argument"), ((sc._h, None, 2, 0, x.data_ptr()), 1, b"null argument"),
                            ((sc._h, P.data_ptr(), 2, 0, None), 1, b"null argument"), ((sc._h, P.data_ptr(), 0, 0, x.data_ptr()), 1, b"B must be in 1.."),
                            ((sc._h, P.data_ptr(), 3, 0, x.data_ptr()), 1, b"B must be in 1.."), ((sc._h, P.data_ptr(), 2, 2, x.data_ptr()), 1, b"stage must be 0"),
                            ((sc._h, P.data_ptr(), 2, -1, x.data_ptr()), 1, b"stage must be 0"),
                            ((text_only._h, P.data_ptr(), 1, 0, x.data_ptr()), 3, b"without vision weights")):
        assert lib.tstar_owl_debug_embed(*args, st) == code and b"tstar_owl_debug_embed" in lib.tstar_last_error() and msg in lib.tstar_last_error(), (args, lib.tstar_last_error())
    torch.cuda.synchronize()
    assert (x == 7.0).all()                                  # nothing ran
    for stage in (0, 1):
        assert lib.tstar_owl_debug_embed(sc._h, P.data_ptr(), 2, stage, x.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(x).all() and torch.equal(x[:ntok], x[ntok:])

    ids = np.zeros((2, 16), np.int32); ids[:, 0] = 49406; ids[:, 1] = 49407
    am = np.ones_like(ids)
    bad_ids = ids.copy(); bad_ids[1, 5] = 49408
    neg_ids = ids.copy(); neg_ids[0, 0] = -1
    out = np.full((2 * 16, 512), np.float32(7.0))
    hx = text_only._h
    for args, code, msg in (((None, ids.ctypes.data, am.ctypes.data, 2, 0, out.ctypes.data), 1, b"null argument"),
                            ((hx, None, am.ctypes.data, 2, 0, out.ctypes.data), 1, b"null argument"), ((hx, ids.ctypes.data, None, 2, 0, out.ctypes.data), 1, b"null argument"),
                            ((hx, ids.ctypes.data, am.ctypes.data, 2, 0, None), 1, b"null argument"), ((hx, ids.ctypes.data, am.ctypes.data, 0, 0, out.ctypes.data), 1, b"Q must be in 1..32"),
                            ((hx, ids.ctypes.data, am.ctypes.data, 33, 0, out.ctypes.data), 1, b"Q must be in 1..32"),
                            ((hx, ids.ctypes.data, am.ctypes.data, 2, 2, out.ctypes.data), 1, b"stage must be 0"),
                            ((hx, bad_ids.ctypes.data, am.ctypes.data, 2, 1, out.ctypes.data), 1, b"token id out of range"),
                            ((hx, neg_ids.ctypes.data, am.ctypes.data, 2, 0, out.ctypes.data), 1, b"token id out of range"),
                            ((vision_only._h, ids.ctypes.data, am.ctypes.data, 2, 0, out.ctypes.data), 3, b"without text weights")):
        assert lib.tstar_owl_debug_text(*args, st) == code and b"tstar_owl_debug_text" in lib.tstar_last_error() and msg in lib.tstar_last_error(), (args, lib.tstar_last_error())
    torch.cuda.synchronize()
    assert (out == np.float32(7.0)).all()                    # nothing was copied out
    assert lib.tstar_owl_debug_text(hx, ids.ctypes.data, am.ctypes.data, 2, 0, out.ctypes.data, st) == 0
    assert np.isfinite(out).all() and np.array_equal(out[:16], out[16:])
    assert lib.tstar_owl_debug_text(hx, ids.ctypes.data, am.ctypes.data, 2, 1, out.ctypes.data, st) == 0
    assert np.array_equal(out[0], out[1]) and text_only.Qs == {}
    text_only.close()
    vision_only.close()


def test_yolo_postprocess_argument_validation(env):
    """tstar_yolo_postprocess checks what tstar_yolo_detect checks, plus its own level arrays."""
    L, lib, _ = env
    from tstar_amd import yolo_world as Y
    from tstar_amd.yolo import YoloDetector
    det = YoloDetector(Y.synthetic_state_dict(2, "s"), "s", max_batch=1)
    t = np.zeros((2, 512), np.float32)
    t[0, 0] = t[1, 1] = 1.0
    emb = [torch.zeros((n * n, 512), device="cuda") for n in (80, 40, 20)]
    dfl = [torch.zeros((n * n, 64), device="cuda") for n in (80, 40, 20)]
    with pytest.raises(L.TStarHipError, match="no text features installed"):
        det.postprocess(emb, dfl, 1, 640, 640)
    det.set_text_feats(t, [1.0, 0.5])
    for bad, msg in ((dict(max_dets=301), "max_dets must be in 1..300"),
                     (dict(grid_rows=100, grid_cols=100), "1..4096 cells"), (dict(image_sets=[64]), "query_set must be in 0..63"),
                     (dict(image_sets=[5]), "no text features installed")):
        with pytest.raises(L.TStarHipError, match=msg):
            det.postprocess(emb, dfl, 1, 640, 640, **bad)
    with pytest.raises(L.TStarHipError, match="outside the letterbox geometry"):
        det.postprocess(emb, dfl, 1, 2, 4000)
    with pytest.raises(ValueError, match="one slot per image"):
        det.postprocess(emb, dfl, 1, 640, 640, image_sets=[0, 0])
    with pytest.raises(ValueError, match="level tensors"):
        det.postprocess(emb, [dfl[0], dfl[1], dfl[2][:-16]], 1, 640, 640)
    with pytest.raises(ValueError, match="per head level"):
        det.postprocess(emb[:2], dfl[:2], 1, 640, 640)
    # the C entry itself: null arguments, a wrong level count, a null level tensor
    out = [torch.zeros(4, device="cuda") for _ in range(3)] + [torch.zeros(1, dtype=torch.int32, device="cuda")]
    pe = (C.c_void_p * 3)(*[e.data_ptr() for e in emb])
    pd = (C.c_void_p * 3)(*[d.data_ptr() for d in dfl])
    tail = (1, 640, 640, 1, 1, None, C.c_float(0.12), 1, out[0].data_ptr(), out[3].data_ptr(), out[1].data_ptr(), out[3].data_ptr(), None, None, None, None, None)
    assert lib.tstar_yolo_postprocess(det._h, None, pd, 3, *tail) == 1 and b"null argument" in lib.tstar_last_error()
    assert lib.tstar_yolo_postprocess(None, pe, pd, 3, *tail) == 1
    assert lib.tstar_yolo_postprocess(det._h, pe, pd, 2, *tail) == 1 and b"n_levels" in lib.tstar_last_error()
    hole = (C.c_void_p * 3)(emb[0].data_ptr(), None, emb[2].data_ptr())
    assert lib.tstar_yolo_postprocess(det._h, hole, pd, 3, *tail) == 1 and b"null level tensor" in lib.tstar_last_error()
    zero = list(tail)
    zero[7] = 0
    assert lib.tstar_yolo_postprocess(det._h, pe, pd, 3, *zero) == 1 and b"max_dets must be in 1..300" in lib.tstar_last_error()
    labels = torch.zeros(1, dtype=torch.int32, device="cuda")
    ok = list(tail)
    ok[9] = labels.data_ptr()
    assert lib.tstar_yolo_postprocess(det._h, pe, pd, 3, *ok) == 0                          # still healthy afterwards
    r = det.postprocess(emb, dfl, 1, 640, 640)
    torch.cuda.synchronize()
    assert int(r.n_kept[0]) == 0 and int(r.labels[0, -1]) == -1
    det.close()


def test_yolo_layer_op_entries_validate_their_arguments(env):
    """tstar_yolo_buffer_copy / tstar_yolo_run_ops: null handle, bad buffer index, B over max_batch; a null form array is allowed; the
    handle is healthy afterwards."""
    L, lib, _ = env
    import yolo_ops_util as OU
    from tstar_amd.yolo import FORM_NAMES, YoloDetector
    case = OU.CONV_CASES[0]
    prog, where = OU.conv_program([case])
    det = YoloDetector.from_program(prog, max_batch=2)
    st = torch.cuda.current_stream().cuda_stream
    n_bufs = len(prog["bufs"])
    t = torch.zeros(2 * 640 * 640 * 3, device="cuda")
    forms = np.zeros(len(prog["ops"]), np.int32)
    assert lib.tstar_yolo_buffer_copy(None, 0, t.data_ptr(), 1, 1, st) == 1 and b"null argument" in lib.tstar_last_error()
    assert lib.tstar_yolo_buffer_copy(det._h, 0, None, 1, 1, st) == 1 and b"null argument" in lib.tstar_last_error()
    for bad in (-1, n_bufs):
        assert lib.tstar_yolo_buffer_copy(det._h, bad, t.data_ptr(), 1, 1, st) == 1 and b"no such activation buffer" in lib.tstar_last_error()
    for bad in (0, 3):
        assert lib.tstar_yolo_buffer_copy(det._h, 0, t.data_ptr(), bad, 1, st) == 1 and b"B must be in 1..max_batch" in lib.tstar_last_error()
        assert lib.tstar_yolo_run_ops(det._h, bad, None, forms.ctypes.data, st) == 1 and b"B must be in 1..max_batch" in lib.tstar_last_error()
    assert lib.tstar_yolo_run_ops(None, 1, None, forms.ctypes.data, st) == 1 and b"null argument" in lib.tstar_last_error()
    with pytest.raises(ValueError, match="no such activation buffer"):
        det.read_buffer(n_bufs, 1)
    with pytest.raises(ValueError, match="B \\* H \\* W \\* C"):
        det.write_buffer(0, t[:5], 1)
    with pytest.raises(L.TStarHipError, match="B must be in 1..max_batch"):
        det.read_buffer(0, 3)
    # still healthy: the case runs, with and without a form array, and gives the reference's values
    d = OU.conv_data(case)
    w = where[0]
    det.write_buffer(w["src"], torch.from_numpy(d.src[:2]).cuda(), 2)
    det.write_buffer(w["dst"], torch.from_numpy(d.dst[:2]).cuda(), 2)
    assert lib.tstar_yolo_run_ops(det._h, case.B, None, None, st) == 0
    got = det.read_buffer(w["dst"], 2).cpu().numpy()
    f = det.run_ops(case.B)
    from tstar_amd.yolo import conv_plan
    assert FORM_NAMES[f[w["op"]]] == conv_plan(case.cin, case.src_c, case.src_off, case.H, case.W, case.cout, case.dst_c, case.dst_off, case.k, case.s, 0,
                                               case.B, 2, True)[0]
    ref, bound, _ = OU.case_reference(case, d)
    out = got[:case.B, :, :, case.dst_off:case.dst_off + case.cout]
    assert (np.abs(out - ref) <= bound).all()
    assert np.array_equal(det.read_buffer(w["dst"], 2).cpu().numpy().view(np.uint32), got.view(np.uint32))
    # a program with attention layers needs text features, as tstar_yolo_detect does
    gprog, _ = OU.gate_program()
    gdet = YoloDetector.from_program(gprog, max_batch=1)
    with pytest.raises(L.TStarHipError, match="no text features installed"):
        gdet.run_ops(1)
    gdet.set_text_feats(OU.gate_text(2), [1.0])
    with pytest.raises(L.TStarHipError, match="query_set must be in 0..63"):
        gdet.run_ops(1, image_sets=[64])
    with pytest.raises(ValueError, match="one slot per image"):
        gdet.run_ops(1, image_sets=[0, 0])
    assert (gdet.run_ops(1) == -1).all()
    gdet.close()
    det.close()


def test_yolo_create_refuses_ops_the_kernels_cannot_serve(env):
    """Shapes that used to fail at the first forward (in the launcher) or not at all are refused by tstar_yolo_create: the table of
    yolo_ops_util.refused_programs (which tests/test_yolo_program_host.py runs through tstar_yolo_check_program without a GPU)."""
    L, lib, _ = env
    import yolo_ops_util as OU
    from tstar_amd.yolo import YoloDetector
    YoloDetector.from_program(OU.crafted_program(), max_batch=1).close()                      # the unmutated program is accepted
    for name, prog, msg in OU.refused_programs():
        with pytest.raises(L.TStarHipError, match=msg):
            YoloDetector.from_program(prog, max_batch=1)
    # and the library is healthy afterwards
    det = YoloDetector.from_program(OU.crafted_program(), max_batch=1)
    assert (det.run_ops(1)[:3] >= 0).all()
    det.close()
