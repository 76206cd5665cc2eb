"""GPU: lossless JPEG re-coding with a restart interval -- the device path against the host twin byte for byte, the device-built
arena records against the planner field for field, output and record buffers between sentinels, the retry at the worst-case slot,
and open_video(resident="jpeg", recode_blocks=8) against the plain resident and the decoded store bit for bit.  Every comparison is
an equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_recode_util as U  # noqa: E402
import jpeg_util as JU  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64


class GuardedAlloc:
    """Hands out buffers of exactly the bytes asked for between GUARD sentinel bytes on either side."""

    def __init__(self):
        self.blocks = []

    def __call__(self, nbytes):
        buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.blocks.append((buf, nbytes))
        return buf[GUARD:GUARD + nbytes]

    def check(self):
        torch.cuda.synchronize()
        assert self.blocks
        for buf, n in self.blocks:
            h = buf.cpu().numpy()
            assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all(), "a write outside an output or record buffer"


def _device(files, n, **kw):
    from tstar_amd import jpeg_recode as JR
    alloc, stats, pieces = GuardedAlloc(), {}, []
    out = JR.recode_device(files, n, stats=stats, alloc=alloc, pieces_out=pieces, **kw)
    alloc.check()
    return out, stats, pieces


def _host(files, n):
    from tstar_amd import jpeg_encode as JE
    stats = {}
    return JE.recode_frames(files, restart_blocks=n, device=False, stats=stats), stats


def _assert_records_are_the_planners(pieces):
    """The device-built records of every piece, collected as an open collects them, against jpeg_plan_segments over the downloaded
    re-coded bytes."""
    from tstar_amd import jpeg, jpeg_recode as JR
    got, want = [], []
    for _, p in pieces:
        host = p.d_bytes.cpu().numpy()
        files = [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(p.plan.offsets, p.lens)]
        geom = next(g for g in map(JR.covered, files) if g is not None)
        got.append((p.plan, p.lens))
        want.append((jpeg.plan_segments(files, geom), [len(f) for f in files]))
    U.assert_arenas_equal(U.arena_of_plans(got), U.arena_of_plans(want))


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_device_recode_equals_the_host_twin(case):
    """n = 1, and a batch whose frames have different lengths with kept frames among them (grayscale, progressive, a coefficient of
    size category 11): the files are the host twin's, the kept ones their sources, and nothing else is kept."""
    W, H, s, n = case
    for name in ("noise100", "qtables"):
        one = [U.source(W, H, s, name)[1]]
        out, stats, pieces = _device(one, n)
        assert out == _host(one, n)[0] and stats == {"recoded": 1, "bytes_in": len(one[0]), "bytes_out": len(out[0])}
        _assert_records_are_the_planners(pieces)
    files = U.batch(W, H, s)
    out, stats, pieces = _device(files, n)
    want, want_stats = _host(files, n)
    assert out == want and stats == want_stats and stats["kept"] == 3
    assert len({len(f) for f in out}) > 8
    _assert_records_are_the_planners(pieces)
    clean = U.batch(W, H, s, with_kept=False)
    out, stats, _ = _device(clean, n)
    assert out == _host(clean, n)[0] and stats.get("kept", 0) == 0 and stats["recoded"] == len(clean)


def test_files_of_several_geometries_in_one_call_and_in_small_chunks():
    files = U.batch(48, 48, "420") + U.batch(40, 24, "422") + [b"no jpeg at all"] + U.batch(48, 48, "420", with_kept=False)
    want, want_stats = _host(files, 2)
    out, stats, pieces = _device(files, 2, chunk=4)
    assert out == want and stats == want_stats
    assert len(pieces) > 4
    _assert_records_are_the_planners(pieces)


def test_a_scan_that_does_not_fit_its_slot_is_coded_again_at_the_bound(monkeypatch):
    """Slots of 16 bytes hold no scan: every frame goes through the retry, here one frame at a time, and comes out whole."""
    from tstar_amd import jpeg_recode as JR
    monkeypatch.setattr(JR, "RETRY_BYTES", 1)
    files = U.batch(48, 48, "420")
    out, stats, pieces = _device(files, 1, slot_bytes=16)
    want, want_stats = _host(files, 1)
    assert out == want and stats == want_stats
    assert len(pieces) == len(files) - 2                             # grayscale and progressive never reach the device path
    _assert_records_are_the_planners(pieces)


@pytest.mark.parametrize("n", [1, 7])
def test_frames_longer_than_a_copy_piece_and_a_marker_step(n):
    """160x120 noise at quality 100: scans of several 16 KiB copy pieces and many 4 KiB steps of the marker pass, 300 intervals at
    n = 1 whose markers fall on every lane and step boundary; frames of different lengths start at every alignment."""
    files = [U.source(160, 120, "444", "noise100", seed)[1] for seed in range(5)]
    files.insert(2, U.source(160, 120, "444", "progressive")[1])
    files.insert(4, U.source(160, 120, "444", "category11")[1])
    assert min(len(f) for f in files[:2]) > 3 * 16384
    out, stats, pieces = _device(files, n)
    want, want_stats = _host(files, n)
    assert out == want and stats == want_stats and stats["kept"] == 2
    _assert_records_are_the_planners(pieces)


def test_a_coefficient_the_standard_tables_cannot_code_keeps_the_frame_on_the_device():
    """The decoder refuses category 11 itself, so the encoder-walk rule is driven directly: one frame's coefficients in HBM get an AC
    value of 1024 behind the entropy stage.  That frame comes out as its source bytes and is counted as kept; its neighbours are the
    host twin's files; the records are the planner's."""
    from tstar_amd import jpeg_recode as JR
    files = U.batch(24, 40, "444", with_kept=False)[:5]
    geom = JR.covered(files[0])
    run = JR.runner_for(files, geom, "cuda")
    ticket = run.submit(0, run.read(0), torch.cuda.current_stream())
    assert run.collect(ticket) == []
    run.d_coef[3, 1] = 1024
    alloc, stats = GuardedAlloc(), {}
    pieces = JR.DeviceRecoder(geom, "cuda", 2, stats, alloc).recode_chunk(ticket[1], run.d_buf, run.d_coef, [])
    alloc.check()
    (p,) = pieces
    host = p.d_bytes.cpu().numpy()
    out = [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(p.plan.offsets, p.lens)]
    want = _host(files, 2)[0]
    assert out[3] == files[3] and p.kept.tolist() == [False, False, False, True, False]
    assert [out[i] for i in (0, 1, 2, 4)] == [want[i] for i in (0, 1, 2, 4)]
    assert stats["kept"] == 1 and stats["recoded"] == 4
    _assert_records_are_the_planners([(files, p)])


def test_the_plain_assemble_entry_is_the_pitch_taking_one_at_1024():
    """tstar_jpeg_recode_assemble forwards to tstar_jpeg_recode_assemble_opt with rows of 1024 bytes: a one-frame piece through both,
    called directly, gives the same bytes (the host twin's file) and records; its own condition, an interval of at least 1, keeps
    its name and launches nothing."""
    from tstar_amd import _lib, jpeg_recode as JR
    files = [U.source(24, 40, "444", "q75")[1]]
    geom = JR.covered(files[0])
    run = JR.runner_for(files, geom, "cuda")
    ticket = run.submit(0, run.read(0), torch.cuda.current_stream())
    assert run.collect(ticket) == []
    batch, rec = ticket[1], JR.DeviceRecoder(geom, "cuda", 2)
    slot = rec.max_slot
    bufs = rec._buffers(1, slot)
    assert rec._scan(run.d_coef, 0, 1, slot, bufs, True) is None
    meta = bufs.meta[:, :1].cpu().numpy()
    assert meta[1, 0] == 0
    pd = JR.PieceDesc(batch.plan, [len(files[0])], 0, 1, np.zeros(1, bool), meta[0].view(np.uint32).astype(np.int64), geom, 2)
    assert pd.pitch == JR.HEADER_PITCH == 1024
    nrec, _ = JR.recode_layout(1, pd.n_segments)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()      # noqa: E731
    d_desc, d_headers, d_hlen = up(pd.desc), up(pd.headers), up(pd.header_len)
    base, parts, plan = run.d_buf.data_ptr(), batch.parts, batch.plan

    def call(entry, pitch, restart):
        alloc = GuardedAlloc()
        d_out, d_rec = alloc(max(16, pd.total)), alloc(nrec)
        _lib.check(getattr(_lib.load(), entry)(
            pd.desc.ctypes.data, d_desc.data_ptr(), 1, pd.n_segments, d_headers.data_ptr(), *pitch, d_hlen.data_ptr(), len(pd.header_len),
            bufs.out.data_ptr(), slot, bufs.meta[0].data_ptr(), restart, pd.n_mcu, base, batch.total, base + parts["quant"][0],
            base + parts["frames"][0], base + parts["segments"][0], len(plan.frames), len(plan.segments), d_rec.data_ptr(), nrec,
            d_out.data_ptr(), pd.total, int(pd.out_len.max()), _lib.stream_ptr()), entry)
        alloc.check()
        return d_out[:pd.total].cpu().numpy().tobytes(), d_rec.cpu().numpy().tobytes()

    plain = call("tstar_jpeg_recode_assemble", (), 2)
    assert plain == call("tstar_jpeg_recode_assemble_opt", (1024,), 2)
    assert plain[0] == _host(files, 2)[0][0]
    with pytest.raises(_lib.TStarHipError, match="tstar_jpeg_recode_assemble: restart interval outside 1..65535"):
        call("tstar_jpeg_recode_assemble", (), 0)


def test_the_recoder_refuses_a_geometry_it_does_not_code():
    from tstar_amd import jpeg_recode as JR
    for geom in ((64, 48, 1, 1, 1), (64, 48, 3, 4, 1)):
        assert not JR.recodable(geom)
        with pytest.raises(ValueError, match="kept"):
            JR.DeviceRecoder(geom, "cuda", 8)


@pytest.mark.parametrize("colour_behind", [False, True])
def test_a_clip_whose_covered_frames_are_grayscale_is_kept_whole(tmp_path, monkeypatch, colour_behind):
    """The first covered frame fixes the open's geometry: grayscale here, which is not re-coded.  Every frame is kept (colour frames
    behind it are another geometry and go to the host, as in the plain open); the store equals the plain resident open."""
    from PIL import Image
    from tstar_amd.video import open_video
    monkeypatch.delenv("TSTAR_JPEG_RECODE", raising=False)
    files = []
    for i in range(8):
        im = Image.fromarray(JU.noise_picture(48, 64, seed=90 + i))
        files.append(U._save(im, quality=95, subsampling=0) if colour_behind and i >= 5 else U._save(im.convert("L"), quality=95))
    path = str(tmp_path / "gray.mjpeg")
    JU.write_mjpeg(path, files)
    plain = open_video(path, fps=1.0, resident="jpeg", pool_frames=3)
    secs = list(range(8))
    want = plain.host_frames(secs)
    for kw in (dict(recode_blocks=8), dict()):
        if not kw:
            monkeypatch.setenv("TSTAR_JPEG_RECODE", "8")
        st = open_video(path, fps=1.0, resident="jpeg", pool_frames=3, **kw)
        assert st.recode_stats == {"recoded": 0, "kept": 8, "bytes_in": sum(map(len, files)), "bytes_out": sum(map(len, files))}
        assert np.array_equal(st.host_frames(secs), want) and st.fetch_errors() == 0
        assert st.source_frames(secs) == files and st.pool_stats()["arena_bytes"] == plain.pool_stats()["arena_bytes"]
        assert st.entropy_split_stats == plain.entropy_split_stats and st.decode_stats == plain.decode_stats
        U.assert_arenas_equal(st.arena, plain.arena)


def test_an_interval_longer_than_the_split_threshold_is_cut_at_fetch(tmp_path, monkeypatch):
    """recode_blocks=65535 on frames above TSTAR_JPEG_SPLIT_BYTES: DRI and no marker, so every re-coded frame is one long interval
    that a fetch cuts.  The store counts them, queues the default number of rounds (no open has seen these scans converge), and
    serves the plain store's frames."""
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    monkeypatch.delenv("TSTAR_JPEG_RECODE", raising=False)
    monkeypatch.delenv("TSTAR_JPEG_SPLIT_BYTES", raising=False)
    files = [U.source(64, 48, "444", "noise100", seed)[1] for seed in range(6)]
    assert min(map(len, files)) > jpeg.SPLIT_MIN_BYTES + 700
    path = str(tmp_path / "long.mjpeg")
    JU.write_mjpeg(path, files)
    plain = open_video(path, fps=1.0, resident="jpeg", pool_frames=4)
    st = open_video(path, fps=1.0, resident="jpeg", pool_frames=4, recode_blocks=65535)
    assert st.recode_stats["recoded"] == 6 and st.recode_stats["kept"] == 0
    assert (st.arena.frames["n_segments"] == 1).all()
    assert st.entropy_split_stats == {"split": 6, "abandoned": 0, "rounds_max": 0} and st._max_rounds == jpeg.SPLIT_MAX_ROUNDS
    secs = [5, 0, 3, 1, 4, 2]
    assert np.array_equal(st.host_frames(secs), plain.host_frames(secs)) and st.fetch_errors() == 0
    assert st.source_frames([2]) == _host(files[2:3], 65535)[0]


N_CLIP, CLIP_W, CLIP_H, GRAY_AT, PROGRESSIVE_AT = 22, 64, 48, 5, 11


def _clip(tmp_path):
    from PIL import Image
    files = []
    for i in range(N_CLIP):
        pic = JU.noise_picture(CLIP_H, CLIP_W, seed=50 + i)
        im = Image.fromarray(pic)
        if i == GRAY_AT:
            files.append(U._save(im.convert("L"), quality=90))
        elif i == PROGRESSIVE_AT:
            files.append(U._save(im, quality=90, subsampling=0, progressive=True))
        else:
            files.append(U._save(im, quality=100 if i % 2 else 97, subsampling=0))     # two table sets; scans above the split threshold
    path = str(tmp_path / "clip.mjpeg")
    JU.write_mjpeg(path, files)
    return path, files


@pytest.mark.parametrize("scale", [1, 2])
def test_recoded_resident_store_serves_the_same_frames(tmp_path, monkeypatch, scale):
    """22 frames of 64x48 without markers, one grayscale and one progressive among them: every frame read through lease and
    host_frames equals the plain resident open and the decoded open; no segment of a re-coded frame is cut; recode_stats accounts for
    every frame; the arena holds the host twin's files and the planner's records."""
    from tstar_amd import jpeg, jpeg_recode as JR
    from tstar_amd.video import JpegFrameStore, open_video
    monkeypatch.delenv("TSTAR_JPEG_RECODE", raising=False)
    path, files = _clip(tmp_path)
    decoded = open_video(path, fps=1.0, jpeg_entropy="device", jpeg_scale=scale)
    plain = open_video(path, fps=1.0, resident="jpeg", pool_frames=6, jpeg_scale=scale)
    st = open_video(path, fps=1.0, resident="jpeg", pool_frames=6, jpeg_scale=scale, recode_blocks=8)
    assert isinstance(st, JpegFrameStore) and st.shape == plain.shape == tuple(decoded.frames.shape)
    want = decoded.frames.cpu().numpy()
    secs = list(range(N_CLIP))
    assert np.array_equal(st.host_frames(secs), want) and np.array_equal(plain.host_frames(secs), want)
    for some in ([3, GRAY_AT, 21, 3], [PROGRESSIVE_AT, 0, 10, 20, 12]):
        lease = st.lease(some)
        got = lease.frames[lease.idx.long()].cpu().numpy()
        lease.done()
        assert np.array_equal(got, want[some])
    assert st.fetch_errors() == 0 and st.decode_stats == plain.decode_stats and st.entropy_stats == plain.entropy_stats
    assert plain.recode_stats is None
    assert plain.entropy_split_stats["split"] == N_CLIP - 2            # every marker-free scan was cut at the plain open
    assert st.entropy_split_stats == {"split": 0, "abandoned": 0, "rounds_max": 0}
    out, host_stats = _host(files, 8)
    assert st.recode_stats == {"recoded": N_CLIP - 2, "kept": 2, "bytes_in": sum(map(len, files)), "bytes_out": sum(map(len, out))}
    assert st.pool_stats()["arena_bytes"] == st.recode_stats["bytes_out"] and host_stats == st.recode_stats
    arena = st.d_arena.cpu().numpy()
    got = [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(st.arena.off, st.arena.len)]
    assert got == out and got[GRAY_AT] == files[GRAY_AT] and got[PROGRESSIVE_AT] == files[PROGRESSIVE_AT]
    geom = JR.covered(files[0])
    U.assert_arenas_equal(st.arena, U.arena_of_plans([(jpeg.plan_segments(out, geom), [len(f) for f in out])]))
    assert (st.arena.frames["n_segments"][[0, 1]] == 6).all()          # 8 x 6 MCUs at 8 per interval
    if scale == 1:
        monkeypatch.setenv("TSTAR_JPEG_RECODE", "8")
        env = open_video(path, fps=1.0, resident="jpeg", pool_frames=6)
        assert env.recode_stats == st.recode_stats and np.array_equal(env.host_frames(secs), want)
