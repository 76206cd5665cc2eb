"""Restart intervals in the JPEG encoder's kernels (csrc/jpeg_enc.hip) against the host twin and against Pillow.

tests/test_jpeg_encode_restart_host.py pins the twin against Pillow on the CPU over the same matrix; here the scan stage's kernels
with an interval (their RST = true forms) must give the twin's bytes, lengths, statuses and counters, keep to their slots, carry frames out of RGB and
NV12 stores, and write Motion-JPEG that the ingest reads back one lane per restart segment.
"""
import io

import numpy as np
import pytest

from jpeg_encode_util import picture, pillow_bytes
from jpeg_restart_util import GEOMETRIES, INTERVALS, QUALITIES, interval_of, pillow_restart_bytes, rst_picture

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mixed_batch(H, W, s, n):
    """noise, smooth, black (the shortest scan), white, then the first two mirrored, rolled, inverted ... of one geometry"""
    base = [rst_picture("noise", H, W, s), rst_picture("smooth", H, W, s), picture("black", H, W), picture("white", H, W)]
    out = []
    for i in range(n):
        a = base[i % 4] if i < 4 else base[i % 2]
        if i >= 4:
            a = np.roll(a[::-1] if i % 3 == 0 else a[:, ::-1], i, axis=1)
            if i % 5 == 0:
                a = 255 - a
        out.append(np.ascontiguousarray(a))
    return np.stack(out)


def device_scan(coef, W, H, s, restart, slot, tail=64):
    """tstar_jpeg_encode_scan_rst on host coefficients -> (bytes of all slots and the tail behind them, lengths, status, counters [n, 3])"""
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    hs, vs = JE.sampling(s)
    n = coef.shape[0]
    p = JE.Plan(W, H, hs, vs, n, slot, restart)
    d_out = torch.full((n * slot + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n, 3), 77, dtype=torch.int32, device="cuda")          # the call zeroes them
    d_work = torch.empty(p.workspace_bytes, dtype=torch.uint8, device="cuda")
    d_coef = cuda(coef)
    _lib.check(_lib.load().tstar_jpeg_encode_scan_rst(d_coef.data_ptr(), n, W, H, hs, vs, restart, d_out.data_ptr(), slot, d_len.data_ptr(),
                                                      d_st.data_ptr(), d_work.data_ptr(), p.workspace_bytes, d_cnt.data_ptr(),
                                                      _lib.stream_ptr()), "tstar_jpeg_encode_scan_rst")
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint32), d_st.cpu().numpy(), d_cnt.cpu().numpy()


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}")
def test_device_scan_equals_the_host_twin(geom):
    """The same coefficients through both scan stages: every byte of every slot (the 0xA5 fill behind a frame's bytes included),
    lengths, statuses and the interval counters frame by frame, in batches of 1, 3 and 17 mixed frames."""
    from tstar_amd import jpeg_encode as JE
    H, W, s = geom
    hs, vs = JE.sampling(s)
    for q in QUALITIES:
        coef17, _ = JE.blocks_host(mixed_batch(H, W, s, 17), q, s)
        for kw in INTERVALS:
            R = interval_of(H, W, s, **kw)
            slot = JE.Plan(W, H, hs, vs, restart=R).max_scan_bytes
            for n in (1, 3, 17):
                coef = coef17[:n] if n != 3 else coef17[[4, 2, 1]]
                counts = np.zeros((n, 3), dtype=np.uint64)
                scans, lengths, status = [], [], []
                for i in range(n):                     # frame by frame on the host: its counters are sums over a call
                    sc, ln, st = JE.scan_host(coef[i:i + 1], W, H, s, restart_counters=counts[i], **kw)
                    scans += sc
                    lengths.append(int(ln[0]))
                    status.append(int(st[0]))
                out, d_len, d_st, d_cnt = device_scan(coef, W, H, s, R, slot)
                assert d_st.tolist() == status == [0] * n and d_len.tolist() == lengths, (geom, q, kw, n)
                assert np.array_equal(d_cnt.astype(np.uint64), counts), (geom, q, kw, n, d_cnt.tolist(), counts.tolist())
                for i in range(n):
                    assert out[i * slot:i * slot + lengths[i]].tobytes() == scans[i], (geom, q, kw, n, i)
                    assert (out[i * slot + lengths[i]:(i + 1) * slot] == 0xA5).all()
                assert (out[n * slot:] == 0xA5).all()


def test_interval_zero_on_the_device_is_the_marker_free_encode():
    """tstar_jpeg_encode_scan_rst with interval 0 == tstar_jpeg_encode_scan, and the keywords at 0 / None == encode_frames without
    them == tstar_jpeg_encode.  jpeg_encode reaches the _rst entries alone, so the entries without an interval are called here as
    the ABI has them."""
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    for H, W, s in GEOMETRIES:
        hs, vs = JE.sampling(s)
        batch = mixed_batch(H, W, s, 5)
        slot = JE.Plan(W, H, hs, vs).max_scan_bytes
        p = JE.Plan(W, H, hs, vs, 5, slot)
        d_out = torch.full((5 * slot + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        o_len = torch.zeros(5, dtype=torch.int32, device="cuda")
        o_st = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        d_work = torch.empty(p.workspace_bytes, dtype=torch.uint8, device="cuda")
        d_coef = torch.empty(5 * p.coef_bytes, dtype=torch.uint8, device="cuda")
        d_frames, d_idx = cuda(batch), cuda(np.arange(5, dtype=np.int32))
        _lib.check(_lib.load().tstar_jpeg_encode(d_frames.data_ptr(), 5, H, W, d_idx.data_ptr(), 5, 100, hs, vs, d_coef.data_ptr(),
                                                 d_out.data_ptr(), slot, o_len.data_ptr(), o_st.data_ptr(), d_work.data_ptr(),
                                                 p.workspace_bytes, _lib.stream_ptr()))
        torch.cuda.synchronize()
        o_out, lens = d_out.cpu().numpy(), o_len.cpu().numpy().view(np.uint32)
        assert o_st.cpu().tolist() == [0] * 5
        want = [JE.header(W, H, 100, s) + o_out[i * slot:i * slot + lens[i]].tobytes() for i in range(5)]
        assert want == [pillow_bytes(a, 100, s) for a in batch]
        assert JE.encode_frames(cuda(batch), 100, s) == want
        assert JE.encode_frames(cuda(batch), 100, s, restart_rows=0, restart_blocks=0) == want
        assert JE.encode_frames(cuda(batch), 100, s, restart_rows=None, restart_blocks=None) == want
        coef, _ = JE.blocks_host(batch, 100, s)
        out, d_len, d_st, d_cnt = device_scan(coef, W, H, s, 0, slot)
        d_out.fill_(0xA5)
        o_len.zero_()
        o_st.fill_(-1)
        d_coef = cuda(coef)
        _lib.check(_lib.load().tstar_jpeg_encode_scan(d_coef.data_ptr(), 5, W, H, hs, vs, d_out.data_ptr(), slot, o_len.data_ptr(),
                                                      o_st.data_ptr(), d_work.data_ptr(), p.workspace_bytes, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(out, d_out.cpu().numpy()) and d_len.tolist() == o_len.cpu().numpy().view(np.uint32).tolist()
        assert d_st.tolist() == o_st.cpu().tolist() == [0] * 5 and not d_cnt.any()
        assert [JE.header(W, H, 100, s) + out[i * slot:i * slot + d_len[i]].tobytes() for i in range(5)] == want


@pytest.mark.parametrize("n,chunk", [(1, None), (3, None), (5, 2)])
def test_whole_encode_of_cuda_tensors_equals_pillow(n, chunk):
    from tstar_amd import jpeg_encode as JE
    for (H, W, s), q, kw in ((GEOMETRIES[0], 100, dict(restart_blocks=1)), (GEOMETRIES[1], 75, dict(restart_rows=1)),
                             (GEOMETRIES[2], 100, dict(restart_blocks=4)), (GEOMETRIES[4], 30, dict(restart_rows=2, restart_blocks=3)),
                             (GEOMETRIES[3], 75, dict(restart_blocks=1)), (GEOMETRIES[0], 75, dict(restart_blocks=16))):
        batch = mixed_batch(H, W, s, n)
        stats = {}
        got = JE.encode_frames(cuda(batch), q, s, chunk=chunk, stats=stats, **kw)
        assert got == [pillow_restart_bytes(a, q, s, **kw) for a in batch], (n, H, W, s, q, kw)
        assert got == JE.encode_frames(batch, q, s, device=False, **kw)
        c = np.zeros(3, dtype=np.uint64)
        JE.encode_host(batch, q, s, restart_counters=c, **kw)
        assert [stats[k] for k in JE.RESTART_COUNTERS] == c.tolist(), (stats, c)


def test_whole_encode_entry_with_an_interval():
    """tstar_jpeg_encode_rst: both stages in one call, frames by index out of a store."""
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    H, W, s = GEOMETRIES[0]
    q, R = 75, 4
    hs, vs = JE.sampling(s)
    store = mixed_batch(H, W, s, 4)
    order = [2, 0, 2, 1]
    slot = JE.Plan(W, H, hs, vs, restart=R).max_scan_bytes
    p = JE.Plan(W, H, hs, vs, 4, slot, R)
    d_out = torch.full((4, slot), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_st = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    d_work = torch.empty(p.workspace_bytes, dtype=torch.uint8, device="cuda")
    d_coef = torch.empty(4 * p.coef_bytes, dtype=torch.uint8, device="cuda")
    d_frames, d_idx = cuda(store), cuda(np.asarray(order, dtype=np.int32))
    _lib.check(_lib.load().tstar_jpeg_encode_rst(d_frames.data_ptr(), 4, H, W, d_idx.data_ptr(), 4, q, hs, vs, R, d_coef.data_ptr(),
                                                 d_out.data_ptr(), slot, d_len.data_ptr(), d_st.data_ptr(), d_work.data_ptr(),
                                                 p.workspace_bytes, d_cnt.data_ptr(), _lib.stream_ptr()), "tstar_jpeg_encode_rst")
    torch.cuda.synchronize()
    out, lens = d_out.cpu().numpy(), d_len.cpu().numpy()
    assert d_st.cpu().tolist() == [0] * 4 and d_cnt.cpu().numpy()[:, 0].tolist() == [3] * 4
    for i, k in enumerate(order):
        assert JE.header(W, H, q, s, restart_blocks=R) + out[i, :lens[i]].tobytes() == pillow_restart_bytes(store[k], q, s, restart_blocks=R)


def test_rgb_and_nv12_stores():
    from tstar_amd.video import synthetic_video, synthetic_video_nv12
    secs = [7, 0, 11, 7]
    for store in (synthetic_video(12, H=90, W=160, seed=4), synthetic_video_nv12(12, H=90, W=160, seed=4)):
        frames = store.host_frames(secs)
        for kw in (dict(restart_blocks=8), dict(restart_rows=1), dict(restart_blocks=1)):
            got = store.jpeg_frames(secs, **kw)
            assert got == [pillow_restart_bytes(a, 75, "4:2:0", **kw) for a in frames], (store.fmt, kw)
        assert store.jpeg_frames(secs, quality=90, subsampling="4:2:2", restart_rows=2) == \
            [pillow_restart_bytes(a, 90, "4:2:2", restart_rows=2) for a in frames]
        with pytest.raises(ValueError, match="restart"):
            store.jpeg_frames(secs, restart_blocks=-1)


def test_a_short_slot_is_refused_and_encoded_again():
    """Slots below the noise frames' need: those frames alone report the short status and leave their slots and everything behind the
    other frames' bytes as they were; encode_frames then encodes them again at the bound and says how many."""
    from tstar_amd import jpeg_encode as JE
    H, W, s = GEOMETRIES[0]
    q, kw = 100, dict(restart_blocks=1)
    batch = mixed_batch(H, W, s, 6)
    coef, _ = JE.blocks_host(batch, q, s)
    scans, lengths, _ = JE.scan_host(coef, W, H, s, **kw)
    need = [int(v) for v in lengths]
    small = max(need[2], need[3])                      # black, white
    big = min(need[0], need[4])                        # noise
    assert big > 2 * small + 64
    # one byte short of the smaller noise frame (its unstuffed bytes fit, its stuffed ones do not), far too short for noise, and
    # what just holds the flat frames
    for slot in (big - 1, (big + small) // 2, small):
        out, d_len, d_st, _ = device_scan(coef, W, H, s, 1, slot)
        assert d_st.tolist() == [int(v > slot) for v in need] and d_st[0] == d_st[4] == 1 and d_st[2] == d_st[3] == 0, slot
        for i in range(6):
            if d_st[i] == 0:
                assert d_len[i] == need[i] and out[i * slot:i * slot + need[i]].tobytes() == scans[i]
                assert (out[i * slot + need[i]:(i + 1) * slot] == 0xA5).all()
            else:
                assert (out[i * slot:(i + 1) * slot] == 0xA5).all()
        assert (out[6 * slot:] == 0xA5).all()
    stats = {}
    got = JE.encode_frames(cuda(batch), q, s, slot_bytes=small, stats=stats, **kw)
    assert stats["retried"] == sum(v > small for v in need) >= 2 and got == [pillow_restart_bytes(a, q, s, **kw) for a in batch]
    c = np.zeros(3, dtype=np.uint64)
    JE.encode_host(batch, q, s, restart_counters=c, **kw)
    assert [stats[k] for k in JE.RESTART_COUNTERS] == c.tolist()


def test_360x640_with_intervals():
    """23 x 40 MCUs, 5 520 blocks: more than the 1 024 blocks one tile of the workgroup's sums covers and more than 256 intervals
    (blocks=8 -> 114 markers; blocks=1 -> 919, the numbering wraps 114 times)."""
    from tstar_amd import jpeg_encode as JE
    batch = np.stack([picture("smooth", 360, 640), picture("noise", 360, 640), picture("noise", 360, 640)[::-1].copy(), picture("black", 360, 640)])
    d = cuda(batch)
    for kw in (dict(restart_blocks=8), dict(restart_rows=1), dict(restart_blocks=1)):
        stats = {}
        got = JE.encode_frames(d, stats=stats, **kw)
        assert got == [pillow_restart_bytes(a, **kw) for a in batch], kw
        assert stats["rst"] == 4 * ((23 * 40 - 1) // interval_of(360, 640, "4:2:0", **kw))


def test_round_trip_through_the_ingest(tmp_path):
    """save_mjpeg(restart_blocks=8) -> open_video in its three modes: every store is Pillow's decode of the written files, and the
    device mode takes every restart segment on one lane (nothing is cut)."""
    from PIL import Image
    from tstar_amd import jpeg
    from tstar_amd.video import open_video, synthetic_video
    store = synthetic_video(12, H=72, W=128, seed=5)
    path = str(tmp_path / "rst.avi")
    assert store.save_mjpeg(path, quality=90, restart_blocks=8) == 12
    src = jpeg.avi_mjpeg(path)
    try:
        files = [bytes(src.read(i)) for i in range(12)]
    finally:
        src.close()
    frames = store.host_frames(range(12))
    assert files == [pillow_restart_bytes(a, 90, "4:2:0", restart_blocks=8) for a in frames]
    want = np.stack([np.asarray(Image.open(io.BytesIO(f))) for f in files])
    host = open_video(path, jpeg_entropy="host")
    dev = open_video(path, jpeg_entropy="device")
    res = open_video(path, resident="jpeg", pool_frames=4)
    for st in (host, dev, res):
        assert st.num_seconds == 12 and st.decode_stats["pillow"] == 0, st.decode_stats
        assert np.array_equal(st.host_frames(list(range(12))), want)
    assert dev.entropy_stats == {"device": 12, "host": 0} and dev.entropy_split_stats == {"split": 0, "abandoned": 0, "rounds_max": 0}
    assert res.entropy_stats == dev.entropy_stats and res.entropy_split_stats == dev.entropy_split_stats
    for secs in ([11, 3], [0, 5, 6, 7], [2], [9, 8, 1, 10]):
        assert np.array_equal(res.host_frames(secs), want[secs])
    assert res.fetch_errors() == 0
    # and markers out of a compressed-resident store again
    assert res.jpeg_frames([4, 9], quality=90, restart_blocks=8) == [pillow_restart_bytes(want[i], 90, "4:2:0", restart_blocks=8) for i in (4, 9)]
