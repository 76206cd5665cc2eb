"""Optimised Huffman tables in the JPEG encoder's kernels (csrc/jpeg_enc.hip) against the host twin and against Pillow's
``optimize=True``.

tests/test_jpeg_optimize_host.py pins the twin and the table procedure against Pillow on the CPU; here the histogram kernel, the
table kernel and the bits kernel that codes with a frame's own tables must give the twin's counts, specs, scans and files, stage
by stage, keep to their slots, carry frames out of RGB and NV12 stores and write Motion-JPEG the ingest reads back.
"""
import io

import numpy as np
import pytest

from jpeg_encode_util import pillow_bytes
from jpeg_optimize_util import (GEOMETRIES, batch_of, deep_table_picture, fibonacci_counts, flat_picture, optimal_table,
                                pillow_optimize_bytes)
from jpeg_restart_util import interval_of, pillow_restart_bytes

pytestmark = pytest.mark.gpu

# the host matrix thinned: every geometry meets two qualities and three of the interval settings
THIN = {0: ((1, dict()), (75, dict(restart_blocks=4)), (100, dict(restart_rows=1))),
        1: ((30, dict(restart_blocks=1)), (100, dict()), (75, dict(restart_blocks=16))),
        2: ((75, dict()), (1, dict(restart_blocks=4)), (100, dict(restart_blocks=1))),
        3: ((30, dict()), (100, dict(restart_blocks=1)), (75, dict(restart_rows=1))),
        4: ((100, dict()), (30, dict(restart_rows=1)), (75, dict(restart_blocks=16)))}


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_scan_opt(coef, W, H, s, restart, slot, tail=64):
    """tstar_jpeg_encode_scan_opt on host coefficients -> (bytes of all slots and the tail behind them, lengths, status, specs [n, 4],
    hist [n, 4, 257] read out of the workspace)"""
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    hs, vs = JE.sampling(s)
    n = coef.shape[0]
    p = JE.Plan(W, H, hs, vs, n, slot, restart, optimize=True)
    d_out = torch.full((n * slot + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_specs = torch.full((n, 4 * JE.SPEC_BYTES), 0xA5, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(p.workspace_bytes, dtype=torch.uint8, device="cuda")
    d_coef = cuda(coef)
    _lib.check(_lib.load().tstar_jpeg_encode_scan_opt(d_coef.data_ptr(), n, W, H, hs, vs, restart, d_out.data_ptr(), slot, d_len.data_ptr(),
                                                      d_st.data_ptr(), d_specs.data_ptr(), d_work.data_ptr(), p.workspace_bytes, None,
                                                      _lib.stream_ptr()), "tstar_jpeg_encode_scan_opt")
    torch.cuda.synchronize()
    hist = d_work[p.off_hist:p.off_hist + n * 4 * JE.HIST_BINS * 4].cpu().numpy().view(np.uint32).reshape(n, 4, JE.HIST_BINS)
    specs = d_specs.cpu().numpy().view(JE.SPEC_DTYPE).reshape(n, 4)
    return d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint32), d_st.cpu().numpy(), specs, hist


@pytest.mark.parametrize("gi", range(len(GEOMETRIES)), ids=lambda i: "{}x{}-{}".format(*GEOMETRIES[i]))
def test_kernels_equal_the_twin_and_pillow_stage_by_stage(gi):
    """Three different pictures, two per chunk: counts [n][4][257], the four specs, the scans and the whole files."""
    from tstar_amd import jpeg_encode as JE
    H, W, s = GEOMETRIES[gi]
    hs, vs = JE.sampling(s)
    batch = batch_of(H, W, s, 3)
    for q, kw in THIN[gi]:
        R = interval_of(H, W, s, **kw)
        coef, _ = JE.blocks_host(batch, q, s)
        tabs = {}
        scans, lengths, status = JE.scan_host(coef, W, H, s, optimize=True, tables=tabs, **kw)
        slot = JE.Plan(W, H, hs, vs, restart=R, optimize=True).max_scan_bytes
        out, d_len, d_st, specs, hist = device_scan_opt(coef, W, H, s, R, slot)
        assert np.array_equal(hist, tabs["hist"]), (gi, q, kw)
        assert specs.tobytes() == tabs["specs"].tobytes(), (gi, q, kw)
        assert d_st.tolist() == status.tolist() == [0] * 3 and d_len.tolist() == lengths.tolist()
        for i in range(3):
            assert out[i * slot:i * slot + lengths[i]].tobytes() == scans[i], (gi, q, kw, i)
            assert (out[i * slot + lengths[i]:(i + 1) * slot] == 0xA5).all()
        assert (out[3 * slot:] == 0xA5).all()
        stats = {}
        files = JE.encode_frames(cuda(batch), q, s, chunk=2, optimize=True, stats=stats, **kw)
        want = [pillow_optimize_bytes(a, q, s, **kw) for a in batch]
        assert files == want, (gi, q, kw)
        assert files == JE.encode_frames(batch, q, s, device=False, optimize=True, **kw)
        assert stats["optimized"] == 3 and stats["table_bytes"] == sum(len(f) - len(sc) - 191 - (6 if R else 0) for f, sc in zip(files, scans))


def test_flat_frames_and_reordered_indices():
    """Four one-symbol tables (20-byte DHT segments), and frames taken by index in another order than they lie in the store."""
    import torch
    from tstar_amd import jpeg_encode as JE
    H, W, s = GEOMETRIES[0]
    store = np.concatenate([batch_of(H, W, s, 3), flat_picture(H, W)[None]])
    want = [pillow_optimize_bytes(a, 75, s) for a in store]
    assert JE.encode_frames(cuda(store), 75, s, optimize=True) == want
    assert want[3].count(b"\xff\xc4") == 4 and len(want[3]) < 191 + 4 * 20 + 40
    order = [3, 1, 0, 2, 1]
    got = JE._encode_device(cuda(store), torch.as_tensor(order, dtype=torch.int32, device="cuda"), 75, s, chunk=2, optimize=True)
    assert got == [want[i] for i in order]


def test_table_kernel_on_crafted_histograms():
    """The table kernel alone (tstar_jpeg_encode_tables, stage 2) on counts put into the workspace: random ones, all 256 symbols, one
    symbol, equal counts (every choice a tie), 1, 2, 3, 5, ... for 18, 30 and 32 symbols (code sizes above 16) and for 33 (above 32:
    the overflow status), and none -> the specs and codes of the table function of the twin."""
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    rs = np.random.RandomState(3)
    cases = [rs.randint(0, 1 << rs.randint(1, 20), 256) * (rs.rand(256) < rs.rand()) for _ in range(21)]
    cases = [c if c.any() else np.arange(256) for c in cases]
    cases += [rs.randint(1, 1000, 256), np.full(256, 9), np.where(np.arange(256) % 3 == 0, 1, 0), np.eye(256, dtype=np.int64)[0xF0] * 7,
              np.where(np.arange(256) < 162, 5, 0)]
    cases += [fibonacci_counts(n) for n in (18, 30, 32, 33)] + [np.zeros(256, dtype=np.int64), np.arange(256)[::-1] + 1]
    assert len(cases) % 4 == 0
    n = len(cases) // 4
    hist = np.zeros((n, 4, JE.HIST_BINS), dtype=np.uint32)
    hist[:, :, :256] = np.stack(cases).reshape(n, 4, 256)
    W, H, slot = 16, 16, 4096
    p = JE.Plan(W, H, 2, 2, n, slot, optimize=True)
    d_work = torch.zeros(p.workspace_bytes, dtype=torch.uint8, device="cuda")
    d_work[p.off_hist:p.off_hist + hist.nbytes] = cuda(hist.view(np.uint8).reshape(-1))
    d_specs = torch.full((n, 4 * JE.SPEC_BYTES), 0xA5, dtype=torch.uint8, device="cuda")
    d_coef = torch.zeros(n * p.coef_bytes, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().tstar_jpeg_encode_tables(d_coef.data_ptr(), n, W, H, 2, 2, 0, slot, 2, d_specs.data_ptr(), d_work.data_ptr(),
                                                    p.workspace_bytes, _lib.stream_ptr()), "tstar_jpeg_encode_tables")
    torch.cuda.synchronize()
    specs = d_specs.cpu().numpy().view(JE.SPEC_DTYPE).reshape(-1)
    codes = d_work[p.off_codes:p.off_codes + n * 4 * 768].cpu().numpy().reshape(-1, 768)
    flags = d_work[:n * 16].cpu().numpy().view(np.uint32).reshape(n, 4)[:, 3]
    statuses = []
    for k, f in enumerate(cases):
        want = JE.huff_optimal(f)
        got = specs[k]
        assert (got["bits"].tolist(), got["vals"][:int(got["nvals"])].tobytes(), int(got["status"])) == \
            (want["bits"].tolist(), want["vals"], want["status"]), k
        assert not got["vals"][int(got["nvals"]):].any()
        assert codes[k, :512].view(np.uint16).tolist() == want["code"].tolist() and codes[k, 512:].tolist() == want["len"].tolist(), k
        statuses.append(want["status"])
    assert statuses.count(JE.HUFF_CLEN_OVERFLOW) == 1 and statuses.count(JE.HUFF_EMPTY) == 1
    bad = np.asarray(statuses).reshape(n, 4).any(axis=1)
    assert ((flags != 0) == bad).all()                 # a frame with a table that has a status is never written


def test_the_deep_table_picture_equals_pillow():
    """One frame of 1368 x 512 whose AC-luma code sizes reach 19 before limiting (5 limiting steps), with and without an interval."""
    from tstar_amd import jpeg_encode as JE
    a = deep_table_picture(18)
    assert a.shape == (1368, 512, 3)
    d = cuda(a[None])
    for kw in (dict(), dict(restart_blocks=8)):
        want = pillow_optimize_bytes(a, 80, "4:4:4", **kw)
        assert JE.encode_frames(d, 80, "4:4:4", optimize=True, **kw) == [want], kw
    coef, _ = JE.blocks_host(a[None], 80, "4:4:4")
    tabs = {}
    JE.scan_host(coef, 512, 1368, "4:4:4", optimize=True, tables=tabs)
    assert optimal_table(tabs["hist"][0, 1, :256])[3] == 5
    *_, specs, hist = device_scan_opt(coef, 512, 1368, "4:4:4", 0, JE.Plan(512, 1368, 1, 1, optimize=True).max_scan_bytes)
    assert np.array_equal(hist, tabs["hist"]) and specs.tobytes() == tabs["specs"].tobytes()


def test_a_short_slot_is_encoded_again():
    from tstar_amd import jpeg_encode as JE
    H, W, s = GEOMETRIES[0]
    batch = np.concatenate([batch_of(H, W, s, 3), flat_picture(H, W)[None]])
    for kw in (dict(), dict(restart_blocks=1)):
        want = [pillow_optimize_bytes(a, 100, s, **kw) for a in batch]
        small = min(len(w) for w in want[:3]) // 2
        stats = {}
        got = JE.encode_frames(cuda(batch), 100, s, slot_bytes=small, chunk=3, optimize=True, stats=stats, **kw)
        assert got == want and stats["retried"] == 3 and stats["optimized"] == 4, (kw, stats)


def test_rgb_and_nv12_stores():
    from tstar_amd.video import synthetic_video, synthetic_video_nv12
    secs = [7, 0, 11, 7]
    for store in (synthetic_video(12, H=90, W=160, seed=4), synthetic_video_nv12(12, H=90, W=160, seed=4)):
        frames = store.host_frames(secs)
        assert store.jpeg_frames(secs, optimize=True) == [pillow_optimize_bytes(a, 75, "4:2:0") for a in frames], store.fmt
        assert store.jpeg_frames(secs, quality=90, subsampling="4:2:2", restart_rows=2, optimize=True) == \
            [pillow_optimize_bytes(a, 90, "4:2:2", restart_rows=2) for a in frames]
        assert all(len(o) < len(p) for o, p in zip(store.jpeg_frames(secs, optimize=True), store.jpeg_frames(secs)))


def test_round_trip_through_the_ingest(tmp_path):
    """save_mjpeg(optimize=True, restart_blocks=8) of 4 frames at 45 x 77 -> open_video with device entropy decode: the store is
    Pillow's decode of the written files, which are Pillow's own."""
    from PIL import Image
    from tstar_amd import jpeg
    from tstar_amd import jpeg_encode as JE
    from tstar_amd.video import FrameStore, open_video
    H, W, s = GEOMETRIES[0]
    frames = np.concatenate([batch_of(H, W, s, 3), flat_picture(H, W)[None]])
    store = FrameStore(cuda(frames), 1.0)
    path = str(tmp_path / "opt.avi")
    assert store.save_mjpeg(path, optimize=True, restart_blocks=8) == 4
    src = jpeg.avi_mjpeg(path)
    try:
        files = [bytes(src.read(i)) for i in range(4)]
    finally:
        src.close()
    assert files == [pillow_optimize_bytes(a, 90, s, restart_blocks=8) for a in frames]
    want = np.stack([np.asarray(Image.open(io.BytesIO(f))) for f in files])
    dev = open_video(path, jpeg_entropy="device")
    assert dev.num_seconds == 4 and np.array_equal(dev.host_frames(list(range(4))), want)
    assert JE.frames_to_base64(store, [2, 0], optimize=True) == JE.frames_to_base64(frames[[2, 0]], optimize=True)


def test_the_default_is_the_encode_without_the_keyword():
    """optimize=False: the bytes, the plan and the stats of the encode as it was."""
    from tstar_amd import jpeg_encode as JE
    for H, W, s in GEOMETRIES[:3]:
        hs, vs = JE.sampling(s)
        batch = batch_of(H, W, s, 3)
        d = cuda(batch)
        for kw in (dict(), dict(restart_blocks=4)):
            stats, plain = {}, {}
            got = JE.encode_frames(d, 75, s, chunk=2, optimize=False, stats=stats, **kw)
            assert got == JE.encode_frames(d, 75, s, chunk=2, stats=plain, **kw)
            assert got == [pillow_restart_bytes(a, 75, s, **kw) if kw else pillow_bytes(a, 75, s) for a in batch]
            assert "optimized" not in stats and "table_bytes" not in stats and set(stats) == set(plain)
        enc = JE.DeviceEncoder(W, H, 75, s, 2)
        assert enc.specs is None and not enc.optimize and enc.plan.workspace_bytes == JE.Plan(W, H, hs, vs, 2, enc.slot).workspace_bytes
