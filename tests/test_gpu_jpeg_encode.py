"""The JPEG encoder's kernels (csrc/jpeg_enc.hip) against the host twin, word for word and byte for byte, and against Pillow.

tests/test_jpeg_encode_host.py pins the twin against Pillow on the CPU; here the device path must give the same coefficients,
the same scans, lengths and statuses, keep to its slots, and carry frames out of a store, a search and into a Motion-JPEG file
that the ingest reads back.
"""
import io

import numpy as np
import pytest

from jpeg_encode_util import SUBSAMPLINGS, picture, pillow_bytes

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mixed_batch(H, W, n):
    """all-black (the shortest scan), noise (the longest), smooth, ... of one size"""
    kinds = ["black", "noise", "smooth", "white", "noise"]
    return np.stack([picture(kinds[i % 5], H, W) if i < 4 else picture("noise", H, W)[::-1, ::-1] for i in range(n)])


@pytest.mark.parametrize("size", [(1, 1), (17, 23), (24, 40), (33, 7), (90, 161)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_block_stage_equals_the_host_twin(size):
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    H, W = size
    store = np.stack([picture("noise", H, W), picture("smooth", H, W), picture("red", H, W)])
    order = [2, 0, 2, 1]                               # one index twice, out of order
    d_store, d_idx = cuda(store), cuda(np.asarray(order, dtype=np.int32))
    lib = _lib.load()
    for s in SUBSAMPLINGS:
        hs, vs = JE.sampling(s)
        blocks = JE.Plan(W, H, hs, vs).blocks
        for q in (5, 75, 100):
            want, want_quant = JE.blocks_host(store, q, s, idx=order)
            d_coef = torch.full((len(order), blocks * 64), 0x5A5A, dtype=torch.int16, device="cuda")
            quant = np.zeros((3, 64), dtype=np.uint16)
            _lib.check(lib.tstar_jpeg_encode_blocks(d_store.data_ptr(), 3, H, W, d_idx.data_ptr(), len(order), q, hs, vs, d_coef.data_ptr(),
                                                    quant.ctypes.data, _lib.stream_ptr()), "tstar_jpeg_encode_blocks")
            torch.cuda.synchronize()
            assert np.array_equal(quant, want_quant)
            assert np.array_equal(d_coef.cpu().numpy(), want), (size, s, q)


@pytest.mark.parametrize("n,chunk", [(1, None), (3, None), (5, 2)])
def test_whole_encode_equals_twin_and_pillow(n, chunk):
    from tstar_amd import jpeg_encode as JE
    H, W = 45, 80
    batch = mixed_batch(H, W, n)
    for q, s in ((100, "4:2:0"), (75, "4:2:2"), (100, "4:4:4"), (5, "4:2:0")):
        got = JE.encode_frames(cuda(batch), q, s, chunk=chunk)
        twin = JE.encode_frames(batch, q, s, device=False)
        assert got == twin, (n, q, s)
        assert got == [pillow_bytes(a, q, s) for a in batch], (n, q, s)


def test_whole_encode_lengths_and_statuses():
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    H, W, q, s = 24, 40, 100, "4:2:0"
    batch = mixed_batch(H, W, 3)
    hs, vs = JE.sampling(s)
    coef, _ = JE.blocks_host(batch, q, s)
    scans, lengths, status = JE.scan_host(coef, W, H, s)
    p = JE.Plan(W, H, hs, vs, 3, JE.Plan(W, H, hs, vs).max_scan_bytes)
    slot = p.max_scan_bytes
    d_out = torch.full((3, slot), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(3, dtype=torch.int32, device="cuda")
    d_st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    d_work = torch.empty(p.workspace_bytes, dtype=torch.uint8, device="cuda")
    d_coef = torch.empty(3 * p.coef_bytes, dtype=torch.uint8, device="cuda")
    d_frames, d_idx = cuda(batch), cuda(np.arange(3, dtype=np.int32))
    _lib.check(_lib.load().tstar_jpeg_encode(d_frames.data_ptr(), 3, H, W, d_idx.data_ptr(), 3, q, hs, vs, d_coef.data_ptr(), d_out.data_ptr(),
                                             slot, d_len.data_ptr(), d_st.data_ptr(), d_work.data_ptr(), p.workspace_bytes, _lib.stream_ptr()),
               "tstar_jpeg_encode")
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0, 0, 0] and d_len.cpu().tolist() == [int(v) for v in lengths]
    out = d_out.cpu().numpy()
    for i in range(3):
        assert out[i, :lengths[i]].tobytes() == scans[i]
        assert (out[i, lengths[i]:] == 0xA5).all()
    assert np.array_equal(d_coef.cpu().numpy().view(np.int16).reshape(3, -1), coef)
    assert lengths[0] < lengths[2] < lengths[1]        # black, smooth, noise


def test_360x640_at_the_defaults():
    from tstar_amd import jpeg_encode as JE
    batch = np.stack([picture("smooth", 360, 640), picture("noise", 360, 640)])
    stats = {}
    got = JE.encode_frames(cuda(batch), stats=stats)
    assert got == [pillow_bytes(a) for a in batch]
    assert stats["retried"] <= 1 and stats["block_ms"] > 0 and stats["entropy_ms"] > 0


def test_a_short_slot_is_refused_and_the_others_are_intact():
    """Per-frame capacity below the noise frame's need: that frame alone reports the short status, the others are intact, and the
    0xA5 fill behind every frame's bytes, in the refused frame's whole slot and behind the last slot is untouched."""
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    H, W, q, s = 45, 80, 100, "4:2:0"
    batch = mixed_batch(H, W, 3)
    hs, vs = JE.sampling(s)
    coef, _ = JE.blocks_host(batch, q, s)
    scans, lengths, _ = JE.scan_host(coef, W, H, s)
    need = [int(v) for v in lengths]
    assert need[1] > 2 * max(need[0], need[2])
    for slot in (need[1] - 1, (need[1] + max(need[0], need[2])) // 2, max(need[0], need[2])):
        p = JE.Plan(W, H, hs, vs, 3, slot)
        tail = 64
        d_out = torch.full((3 * slot + tail,), 0xA5, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(3, dtype=torch.int32, device="cuda")
        d_st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        d_work = torch.empty(p.workspace_bytes, dtype=torch.uint8, device="cuda")
        d_coef = cuda(coef)
        _lib.check(_lib.load().tstar_jpeg_encode_scan(d_coef.data_ptr(), 3, W, H, hs, vs, d_out.data_ptr(), slot, d_len.data_ptr(),
                                                      d_st.data_ptr(), d_work.data_ptr(), p.workspace_bytes, _lib.stream_ptr()),
                   "tstar_jpeg_encode_scan")
        torch.cuda.synchronize()
        assert d_st.cpu().tolist() == [0, 1, 0], slot
        out = d_out.cpu().numpy()
        for i in (0, 2):
            assert d_len[i].item() == need[i]
            assert out[i * slot:i * slot + need[i]].tobytes() == scans[i]
            assert (out[i * slot + need[i]:(i + 1) * slot] == 0xA5).all()
        assert (out[slot:2 * slot] == 0xA5).all() and (out[3 * slot:] == 0xA5).all()
    # the Python path encodes such a frame again at the bound and says so
    stats = {}
    got = JE.encode_frames(cuda(batch), q, s, slot_bytes=max(need[0], need[2]), stats=stats)
    assert stats["retried"] == 1 and got == [pillow_bytes(a, q, s) for a in batch]


def test_nv12_store():
    from tstar_amd.video import synthetic_video_nv12
    store = synthetic_video_nv12(12, H=90, W=160, seed=4)
    secs = [7, 0, 11, 7]
    got = store.jpeg_frames(secs)
    assert got == [pillow_bytes(a) for a in store.host_frames(secs)]
    with pytest.raises(IndexError):
        store.jpeg_frames([12])


def test_round_trip_through_the_ingest(tmp_path):
    from PIL import Image
    from tstar_amd.video import open_video, synthetic_video
    store = synthetic_video(40, H=90, W=160, seed=2)
    path = str(tmp_path / "store.avi")
    assert store.save_mjpeg(path, quality=90) == 40
    frames = store.host_frames(range(40))
    want = np.stack([np.asarray(Image.open(io.BytesIO(pillow_bytes(a, 90)))) for a in frames])
    for mode in ("device", "host"):
        back = open_video(path, jpeg_entropy=mode)
        assert back.num_seconds == 40 and back.raw_fps == 1.0
        assert back.decode_stats["pillow"] == 0, back.decode_stats
        assert np.array_equal(back.frames.cpu().numpy(), want), mode
    raw = str(tmp_path / "store.mjpeg")
    store.save_mjpeg(raw, quality=90)
    back = open_video(raw, fps=1.0)
    assert back.num_seconds == 40 and np.array_equal(back.frames.cpu().numpy(), want)


def test_out_of_a_search():
    import base64
    from PIL import Image
    from tstar_amd import jpeg_encode as JE
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import synthetic_video
    store = synthetic_video(160, seed=3)
    h = OWLInterface(synthetic_seed=0, max_batch=8, device="cuda:0")
    s = TStarSearcher(store, h, ["couch"], ["tv"], search_nframes=4, image_grid_shape=(3, 3), search_budget=0.2,
                      confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
    frames, ts = s.search()
    assert len(ts) == 4
    frames = np.asarray(frames)
    assert store.jpeg_frames(ts) == [pillow_bytes(a) for a in frames]
    want = []
    for a in frames:                                   # TStar/utilites.py:28-35
        buffered = io.BytesIO()
        Image.fromarray(a).save(buffered, format="JPEG")
        want.append(base64.b64encode(buffered.getvalue()).decode("utf-8"))
    assert JE.frames_to_base64(store, ts) == want
