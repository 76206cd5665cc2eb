"""GPU: JPEG decode at 1/2, 1/4, 1/8 size -- the reduced inverse-DCT kernels and the scaled colour stage against the host twin (which
tests/test_jpeg_scale_host.py pins to Pillow's draft), the slots entry, open_video(jpeg_scale=s) in every mode against Pillow's draft,
and a whole search on a scaled store.  Every comparison is an equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_scale_util as SU  # noqa: E402
import jpeg_util as JU  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = [(40, 24), (77, 45), (33, 31)]                                  # (W, H)


def _case(W, H, sampling, n):
    datas = [JU.encode(SU.picture(SU.KINDS[i % 3], W, H, seed=i), sampling, (75, 100, 30)[i % 3]) for i in range(n)]
    return SU.coefficients(datas)


def _device_inputs(coef, quant):
    return torch.from_numpy(coef).cuda(), torch.from_numpy(quant.view(np.int16)).cuda()


@pytest.mark.parametrize("s", SU.SCALES)
@pytest.mark.parametrize("sampling", SU.SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_device_entry_equals_the_host_twin(size, sampling, s):
    """n = 1, 3, 5 frames (the blocks of a component fill one workgroup of 32, cross into the next and are no multiple of it), the
    plane workspace poisoned, 0xA5 in front of and behind the picture, which starts at a multiple of 4 (the dword stores of the
    colour stage) and one byte further (its byte stores)."""
    from tstar_amd import _lib
    lib = _lib.load()
    W, H = size
    geom, coef, quant = _case(W, H, sampling, 5)
    rc, ow, oh, plane_bytes, cov = SU.sizes(geom, s)
    assert rc == 0 and cov == 1 and (ow, oh) == (SU.ceil_div(W, s), SU.ceil_div(H, s))
    rc, want = SU.reconstruct_host(geom, coef, quant, s, threads=2)
    assert rc == 0
    d_coef, d_quant = _device_inputs(coef, quant)
    for n in (1, 3, 5):
        for shift in (0, 1):
            planes = torch.full((n * plane_bytes + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
            nbytes = n * oh * ow * 3
            buf = torch.full((GUARD + shift + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            assert (buf.data_ptr() + GUARD) % 4 == 0
            _lib.check(lib.tstar_jpeg_reconstruct_scaled(d_coef.data_ptr(), d_quant.data_ptr(), n, *geom, s, planes.data_ptr(),
                                                         buf.data_ptr() + GUARD + shift, _lib.stream_ptr()), "tstar_jpeg_reconstruct_scaled")
            torch.cuda.synchronize()
            out = buf.cpu().numpy()
            assert (out[:GUARD + shift] == 0xA5).all() and (out[GUARD + shift + nbytes:] == 0xA5).all(), "a write outside the picture"
            assert (planes[n * plane_bytes:] == 0xEE).all(), "a write behind the plane workspace"
            got = out[GUARD + shift:GUARD + shift + nbytes].reshape(n, oh, ow, 3)
            diff = np.nonzero(got != want[:n])
            assert len(diff[0]) == 0, f"n={n} shift={shift}: {len(diff[0])} bytes differ, first at {[int(a[0]) for a in diff]}"


def test_device_entries_refuse_what_the_host_entry_refuses():
    from tstar_amd import _lib
    lib = _lib.load()
    geom, coef, quant = _case(16, 16, "422", 1)
    d_coef, d_quant = _device_inputs(coef, quant)
    planes = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    slots = torch.zeros(1, dtype=torch.int32, device="cuda")
    for s in (4, 3, 0, 16):                                             # 4: a chroma row of 2 samples is not covered
        assert lib.tstar_jpeg_reconstruct_scaled(d_coef.data_ptr(), d_quant.data_ptr(), 1, *geom, s, planes.data_ptr(), buf.data_ptr(),
                                                 _lib.stream_ptr()) == 1, s
        assert lib.tstar_jpeg_reconstruct_slots_scaled(d_coef.data_ptr(), d_quant.data_ptr(), 1, *geom, s, planes.data_ptr(), buf.data_ptr(), 1,
                                                       slots.data_ptr(), _lib.stream_ptr()) == 1, s
    assert lib.tstar_jpeg_reconstruct_scaled(None, d_quant.data_ptr(), 1, *geom, 2, planes.data_ptr(), buf.data_ptr(), _lib.stream_ptr()) == 1
    assert lib.tstar_jpeg_reconstruct_scaled(d_coef.data_ptr(), d_quant.data_ptr(), 1, *geom, 8, planes.data_ptr() + 4, buf.data_ptr(),
                                             _lib.stream_ptr()) == 1       # the plane workspace wants 8-byte alignment
    torch.cuda.synchronize()
    assert (buf == 0xA5).all() and (planes == 0xEE).all()


@pytest.mark.parametrize("s", SU.SCALES)
@pytest.mark.parametrize("size,sampling", [((33, 31), "420"), ((77, 45), "422"), ((40, 24), "444"), ((33, 31), "gray")])
def test_slots_entry_equals_the_host_twin(size, sampling, s):
    """Slots out of order and not neighbours, one below and one above the pool skipped, every other slot and 64 sentinel bytes on
    both sides of the pool untouched."""
    from tstar_amd import _lib
    lib = _lib.load()
    W, H = size
    geom, coef, quant = _case(W, H, sampling, 5)
    _, ow, oh, plane_bytes, _ = SU.sizes(geom, s)
    rc, want = SU.reconstruct_host(geom, coef, quant, s)
    assert rc == 0
    d_coef, d_quant = _device_inputs(coef, quant)
    planes = torch.full((5 * plane_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    P, per = 6, oh * ow * 3
    slots = [4, -1, 0, P, 2]
    buf = torch.full((GUARD + P * per + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_slots = torch.tensor(slots, dtype=torch.int32, device="cuda")
    _lib.check(lib.tstar_jpeg_reconstruct_slots_scaled(d_coef.data_ptr(), d_quant.data_ptr(), 5, *geom, s, planes.data_ptr(),
                                                       buf.data_ptr() + GUARD, P, d_slots.data_ptr(), _lib.stream_ptr()),
               "tstar_jpeg_reconstruct_slots_scaled")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == 0xA5).all() and (out[-GUARD:] == 0xA5).all(), "a write outside the pool"
    pool = out[GUARD:-GUARD].reshape(P, oh, ow, 3)
    for j, slot in enumerate(slots):
        if 0 <= slot < P:
            assert np.array_equal(pool[slot], want[j]), f"frame {j} in slot {slot}"
    for slot in (1, 3, 5):
        assert (pool[slot] == 0xA5).all(), f"slot {slot} was written"


# ------------------------------------------------------------------------------------------------ open_video
def _list(sampling, n=12, W=77, H=45):
    return [JU.encode(SU.picture(SU.KINDS[i % 3], W, H, seed=20 + i), sampling, 90) for i in range(n)]


@pytest.mark.parametrize("s", SU.SCALES)
@pytest.mark.parametrize("sampling", ["420", "422"])
def test_open_video_gives_pillows_draft_in_every_mode(sampling, s, monkeypatch):
    """12 frames of 77 x 45 with a progressive one among them: host entropy, device entropy with the split path running, and the
    compressed-resident store with 4 slots of oh * ow * 3 bytes."""
    assert JU.turbo(), "Pillow here is not built on libjpeg-turbo: the byte-equality yardstick does not apply"
    from tstar_amd.video import JpegFrameStore, open_video
    W, H = 77, 45
    datas = _list(sampling)
    datas[5] = JU.encode(SU.picture("gradient", W, H, seed=25), sampling, 90, progressive=True)
    want = np.stack([SU.pillow_draft(d, s) for d in datas])
    ow, oh = SU.ceil_div(W, s), SU.ceil_div(H, s)
    st = open_video(datas, jpeg_scale=s, jpeg_entropy="host")
    assert tuple(st.frames.shape) == (12, oh, ow, 3) and np.array_equal(st.frames.cpu().numpy(), want)
    assert st.decode_stats == {"device": 11, "host": 0, "pillow": 1} and (st.jpeg_scale, st.source_size) == (s, (W, H))
    monkeypatch.setenv("TSTAR_JPEG_SPLIT_BYTES", "256")
    st = open_video(datas, jpeg_scale=s, jpeg_entropy="device")
    assert np.array_equal(st.frames.cpu().numpy(), want)
    assert st.entropy_stats == {"device": 11, "host": 1} and st.entropy_split_stats["split"] > 0
    rs = open_video(datas, jpeg_scale=s, resident="jpeg", pool_frames=4)
    assert isinstance(rs, JpegFrameStore) and rs.shape == (12, oh, ow, 3) and (rs.jpeg_scale, rs.source_size) == (s, (W, H))
    assert rs.pool_stats()["pool_bytes"] == (4 + 1) * oh * ow * 3 and rs.pool_stats()["exceptions"] == 1
    assert rs.decode_stats == st.decode_stats and rs.entropy_stats == st.entropy_stats
    assert np.array_equal(rs.host_frames(list(range(12))), want)
    lease = rs.lease([7, 2, 5, 7])
    got = lease.frames.index_select(0, lease.idx.long()).cpu().numpy()
    lease.done()
    assert lease.frames.shape[1:] == (oh, ow, 3) and np.array_equal(got, want[[7, 2, 5, 7]]) and rs.fetch_errors() == 0


# ------------------------------------------------------------------------------------------------ a whole search
def test_a_search_on_a_scaled_store_is_the_search_on_pillows_draft(tmp_path):
    """64 frames of 72 x 128 at 1/2 size, a 2 x 2 grid, synthetic weights: keyframes, timestamps, scores and P are those of a search on a
    FrameStore built from Pillow's draft of the same files -- a scaled store is an ordinary RGB store."""
    assert JU.turbo(), "Pillow here is not built on libjpeg-turbo: the byte-equality yardstick does not apply"
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import FrameStore, open_video, synthetic_frames_numpy
    n = 64
    frames = synthetic_frames_numpy(range(n), n, 72, 128, seed=3)
    datas = [JU.encode(f, "420", 90) for f in frames]
    path = str(tmp_path / "search.mjpeg")
    JU.write_mjpeg(path, datas)
    draft = np.stack([SU.pillow_draft(d, 2) for d in datas])
    stores = {"scaled": open_video(path, fps=1.0, jpeg_scale=2),
              "draft": FrameStore(torch.from_numpy(draft).cuda(), 1.0, n, name="draft")}
    assert stores["scaled"].shape == (n, 36, 64, 3) and torch.equal(stores["scaled"].frames, stores["draft"].frames)
    runs = {}
    for kind, store in stores.items():
        h = OWLInterface(synthetic_seed=0, max_batch=16, weights_dtype="f32", input_size=(64, 96))
        s = TStarSearcher(store, h, ["couch"], ["tv", "chair"], search_nframes=4, image_grid_shape=(2, 2), search_budget=0.5,
                          confidence_threshold=0.6, rng=np.random.RandomState(11), keep_visual_history=True)
        key_frames, ts = s.search()
        runs[kind] = dict(frames=np.asarray(key_frames), ts=list(ts), sd=np.array(s.score_distribution),
                          scores=[np.asarray(v) for v in s.Score_history], P=[np.asarray(v) for v in s.P_history], iterations=s.iterations)
        h.scorer.close()
    a, b = runs["scaled"], runs["draft"]
    assert a["iterations"] == b["iterations"] >= 1 and a["ts"] == b["ts"] and np.array_equal(a["frames"], b["frames"])
    assert a["frames"].shape[1:] == (36, 64, 3)
    assert np.array_equal(a["sd"], b["sd"])
    for key in ("scores", "P"):
        assert len(a[key]) == len(b[key]) > 0 and all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), key
