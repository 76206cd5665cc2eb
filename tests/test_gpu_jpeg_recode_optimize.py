"""GPU: lossless JPEG re-coding with optimised Huffman tables -- the device path against the host twin byte for byte in both modes
(tables per frame, tables shared by a group), the group reduction and the indirected bits kernel alone through the stages of
tstar_jpeg_encode_scan_grp, the retry at the worst-case slot, and open_video(resident="jpeg", recode_blocks=8, recode_optimize=True)
against the plain resident and the decoded store bit for bit.  Every comparison is an equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_recode_optimize_util as OU  # noqa: E402
import jpeg_recode_util as U  # noqa: E402
import jpeg_util as JU  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64
SUB = {"420": "4:2:0", "422": "4:2:2", "444": "4:4:4"}


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
    out = JR.recode_device(files, n, stats=stats, alloc=alloc, pieces_out=pieces, optimize=True, **kw)
    alloc.check()
    return out, stats, pieces


def _host(files, n, **kw):
    from tstar_amd import jpeg_recode as JR
    stats = {}
    return JR.recode_host(files, n, stats, optimize=True, **kw), stats


def _assert_records_are_the_planners(pieces):
    """The device-built records of every piece, collected as an open collects them, against jpeg_plan_segments over the downloaded
    re-coded bytes (table sets included: one per distinct tables and quantisation set)."""
    from tstar_amd import jpeg, jpeg_recode as JR
    got, want = [], []
    for _, p in pieces:
        host = p.d_bytes.cpu().numpy()
        files = [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(p.plan.offsets, p.lens)]
        geom = next(g for g in map(JR.covered, files) if g is not None)
        got.append((p.plan, p.lens))
        want.append((jpeg.plan_segments(files, geom, cap_sets=64), [len(f) for f in files]))
    U.assert_arenas_equal(U.arena_of_plans(got), U.arena_of_plans(want))


# ------------------------------------------------------------------------------------------------ 1. device = twin, both modes
@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_device_recode_equals_the_host_twin_in_both_modes(case):
    """n = 1 frame and a batch whose frames have different lengths with kept frames among them; tables per frame, and tables shared
    by groups of 3 cut inside chunks of 4 (a last group of one among them)."""
    W, H, s, n = case
    for name in ("noise100", "qtables"):
        one = [U.source(W, H, s, name)[1]]
        for kw in (dict(), dict(shared=True)):
            out, stats, pieces = _device(one, n, **kw)
            want, want_stats = _host(one, n, **kw)
            assert out == want and stats == want_stats and stats["optimized"] == 1
            _assert_records_are_the_planners(pieces)
        assert out == _host(one, n)[0]                                    # a group of one frame is the frame's own tables
    files = U.batch(W, H, s)
    out, stats, pieces = _device(files, n)
    want, want_stats = _host(files, n)
    assert out == want and stats == want_stats and stats["kept"] == 3 and stats["optimized"] == 10
    assert len({len(f) for f in out}) > 8
    _assert_records_are_the_planners(pieces)
    kw = dict(shared=True, group_frames=3, chunk=4)
    out, stats, pieces = _device(files, n, **kw)
    want, want_stats = _host(files, n, **kw)
    assert out == want and stats == want_stats and stats["kept"] == 3 and stats["table_sets"] >= 5
    assert len(pieces) == 3
    _assert_records_are_the_planners(pieces)
    for a, b in zip(out, files):
        assert np.array_equal(OU.pixels(a), OU.pixels(b))


def test_the_per_frame_mode_is_the_shared_mode_with_groups_of_one():
    """The device half of the host test of this name: tables per frame and tables shared by groups of one frame give the same
    files, each other's and the host twin's, and the same stats but for the two keys that count tables."""
    for files, n, want, want_stats in OU.groups_of_one_cases():
        own, own_stats, pieces = _device(files, n)
        _assert_records_are_the_planners(pieces)
        shared, shared_stats, pieces = _device(files, n, shared=True, group_frames=1)
        _assert_records_are_the_planners(pieces)
        assert own == shared == want and own_stats == want_stats
        assert OU.without(shared_stats, "table_sets") == OU.without(own_stats, "table_bytes")
        assert shared_stats["table_sets"] == own_stats["optimized"] and "table_bytes" not in shared_stats and "table_sets" not in own_stats


def test_files_of_two_geometries_in_one_call():
    files = U.batch(48, 48, "420") + U.batch(40, 24, "422") + [b"no jpeg at all"] + U.batch(48, 48, "420", with_kept=False)
    for kw in (dict(chunk=4), dict(shared=True, group_frames=5, chunk=7), dict(shared=True)):
        want, want_stats = _host(files, 2, **kw)
        out, stats, pieces = _device(files, 2, **kw)
        assert out == want and stats == want_stats
        _assert_records_are_the_planners(pieces)
    assert len(pieces) == 2 and stats["table_sets"] == 4 + 4               # one group per geometry, four quantisation sets each


# ------------------------------------------------------------------------------------------------ 2. the new kernels alone
def _coefficients(W, H, s, n, seed=0):
    from tstar_amd import jpeg_encode as JE
    frames = np.stack([JU.noise_picture(H, W, seed=seed + i) if i % 2 else U.picture(W, H, "q75", seed + i) for i in range(n)])
    coef, _ = JE.blocks_host(frames, 90, SUB[s])
    return coef


class GroupRun:
    """One call of tstar_jpeg_encode_scan_grp on host coefficients: every device buffer of exact size between sentinels."""

    def __init__(self, coef, W, H, s, restart, group, stages, counts=None, slot=None):
        from tstar_amd import _lib, jpeg_encode as JE
        hs, vs = JE.sampling(SUB[s])
        m = coef.shape[0]
        group = np.ascontiguousarray(group, dtype=np.int32)
        k = int(group.max()) + 1
        one = JE.Plan(W, H, hs, vs, 1, restart=restart, optimize=True)
        self.slot = slot = (one.max_scan_bytes + 15) // 16 * 16 if slot is None else slot
        p = JE.Plan(W, H, hs, vs, m, slot, restart, True)
        span = np.zeros((k, 2), dtype=np.int32)
        lib = _lib.load()
        _lib.check(lib.tstar_jpeg_encode_group_spans(group.ctypes.data, m, k, W, H, hs, vs, span.ctypes.data), "tstar_jpeg_encode_group_spans")
        alloc = GuardedAlloc()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()       # noqa: E731
        d_coef, d_group, d_span = up(coef), up(group), up(span)
        d_hist, d_specs, d_out = alloc(k * 4 * JE.HIST_BINS * 4), alloc(k * 4 * JE.SPEC_BYTES), alloc(m * slot)
        d_meta, d_work = alloc(2 * m * 4), alloc(p.workspace_bytes)
        if counts is not None:
            d_hist.copy_(up(np.asarray(counts, dtype=np.uint32)))
        _lib.check(lib.tstar_jpeg_encode_scan_grp(d_coef.data_ptr(), m, W, H, hs, vs, restart, group.ctypes.data, span.ctypes.data, d_group.data_ptr(),
                                                  d_span.data_ptr(), k, stages, d_hist.data_ptr(), d_specs.data_ptr(), d_out.data_ptr(), slot,
                                                  d_meta.data_ptr(), d_meta.data_ptr() + 4 * m, d_work.data_ptr(), p.workspace_bytes, _lib.stream_ptr()),
                   "tstar_jpeg_encode_scan_grp")
        alloc.check()
        self.hist = d_hist.cpu().numpy().view(np.uint32).reshape(k, 4, JE.HIST_BINS)
        self.specs = d_specs.cpu().numpy().view(JE.SPEC_DTYPE).reshape(k, 4)
        self.codes = d_work[p.off_codes:p.off_codes + k * 4 * 768].cpu().numpy().reshape(k * 4, 768)
        meta = d_meta.cpu().numpy().view(np.int32).reshape(2, m)
        self.lengths, self.status = meta[0].view(np.uint32), meta[1]
        self.out = d_out.cpu().numpy().reshape(m, slot)


@pytest.mark.parametrize("geom", [(48, 48, "420", 2), (160, 120, "444", 7), (176, 144, "444", 0)], ids=["48x48", "160x120", "176x144"])
def test_group_counts_are_the_sums_of_the_frames_counts(geom):
    """Stage 1 alone: groups of 1, 2 and 5 frames with a frame outside every group between them; 176x144 at 4:4:4 (1188 blocks) has
    more than one histogram workgroup per frame."""
    from tstar_amd import jpeg_encode as JE
    W, H, s, restart = geom
    group = np.array([0, -1, 1, 1, -1, -1, 2, 2, 2, -1, 2, 2], dtype=np.int32)
    coef = _coefficients(W, H, s, len(group))
    tables = {}
    JE.scan_host(coef, W, H, SUB[s], restart_blocks=restart, optimize=True, tables=tables)
    run = GroupRun(coef, W, H, s, restart, group, 1)
    for g in range(3):
        assert np.array_equal(run.hist[g], tables["hist"][group == g].sum(axis=0)), g
    assert run.hist[:, [0, 2]].sum() == 8 * (-(-W // 16) * -(-H // 16) * 6 if s == "420" else (W // 8) * (H // 8) * 3)      # a DC symbol per block


def test_group_tables_on_crafted_counts():
    """Stage 2 alone on counts put into the groups' histograms: ties, all 256 symbols, one symbol, code sizes above 16 (the limiting
    loop) and above 32 (the overflow) -> the specs and codes of the table function of the twin."""
    from tstar_amd import jpeg_encode as JE
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from jpeg_optimize_util import fibonacci_counts
    rs = np.random.RandomState(5)
    cases = [rs.randint(0, 1 << rs.randint(1, 20), 256) * (rs.rand(256) < rs.rand()) for _ in range(5)]
    cases = [c if c.any() else np.arange(256) for c in cases]
    cases += [rs.randint(1, 1000, 256), np.full(256, 9), np.eye(256, dtype=np.int64)[0xF0] * 7, np.arange(256)[::-1] + 1]
    cases += [fibonacci_counts(n) for n in (18, 30, 33)]
    k = len(cases) // 4
    counts = np.zeros((k, 4, JE.HIST_BINS), dtype=np.uint32)
    counts[:, :, :256] = np.stack(cases).reshape(k, 4, 256)
    group = np.array([0, 0, -1, 1, 2], dtype=np.int32)
    run = GroupRun(np.zeros((5, 6 * 64), dtype=np.int16), 16, 16, "420", 0, group, 2, counts, slot=4096)
    assert np.array_equal(run.hist, counts)
    statuses = []
    for q, f in enumerate(cases):
        want, got = JE.huff_optimal(f), run.specs.reshape(-1)[q]
        assert (got["bits"].tolist(), got["vals"][:int(got["nvals"])].tobytes(), int(got["status"])) == \
            (want["bits"].tolist(), want["vals"], want["status"]), q
        assert run.codes[q, :512].view(np.uint16).tolist() == want["code"].tolist() and run.codes[q, 512:].tolist() == want["len"].tolist(), q
        statuses.append(want["status"])
    assert statuses.count(JE.HUFF_CLEN_OVERFLOW) == 1 and statuses[-1] == JE.HUFF_CLEN_OVERFLOW


@pytest.mark.parametrize("restart", [0, 2])
def test_the_scans_with_group_tables_and_an_overflowing_group(restart):
    """All stages against the twin's group-coding function; then counts of the test's own (stages 2 + 4): every frame of the group
    whose table overflows has status 3 and an untouched slot, the other groups are coded with the crafted tables."""
    from tstar_amd import jpeg_encode as JE, jpeg_recode as JR
    W, H, s = 48, 48, "420"
    group = np.array([0, 0, -1, 1, 1, 1, 2], dtype=np.int32)
    coef = _coefficients(W, H, s, len(group), seed=3)
    coef[4, 64 * 3 + 9] = -32768                                          # category 16: status 2, counted, no bin outside the histogram
    geom = (W, H, 3, 2, 2)
    for counts in (None, OU.fibonacci_hist(3, 1, 2, 33)):
        scans, status, specs, hist = JR.code_host_shared(coef, geom, restart, group, 3, counts)
        run = GroupRun(coef, W, H, s, restart, group, 7 if counts is None else 6, counts)
        assert run.status.tolist() == status.tolist() and np.array_equal(run.hist, hist) and run.specs.tobytes() == specs.tobytes()
        for i, sc in enumerate(scans):
            n = 0 if sc is None else len(sc)
            assert (sc is None) == (run.status[i] != 0) and (sc is None or run.lengths[i] == n)
            assert run.out[i, :n].tobytes() == (sc or b"") and (run.out[i, n:] == 0xA5).all()
    assert status.tolist() == [0, 0, 3, 3, 2, 3, 0]


# ------------------------------------------------------------------------------------------------ 3. slot retry
@pytest.mark.parametrize("n", [1, 7, 0, 65535])
@pytest.mark.parametrize("shared", [False, True], ids=["frame", "group"])
def test_a_scan_that_does_not_fit_its_slot_is_coded_again_at_the_bound(monkeypatch, n, shared):
    """Slots of 16 bytes hold no scan: every frame goes through the retry, one frame at a time, with the tables of the first pass.
    160x120 noise at quality 100: several 16 KiB copy pieces, 300 intervals at n = 1 whose markers fall on every lane and step
    boundary; n = 0 and an interval beyond the frame leave no marker at all."""
    from tstar_amd import jpeg_recode as JR
    monkeypatch.setattr(JR, "RETRY_BYTES", 1)
    files = [U.source(160, 120, "444", "noise100", seed)[1] for seed in range(4)]
    files.insert(2, U.source(160, 120, "444", "progressive")[1])
    assert min(len(f) for f in files[:2]) > 3 * 16384
    kw = dict(shared=True, group_frames=3) if shared else {}
    out, stats, pieces = _device(files, n, slot_bytes=16, **kw)
    want, want_stats = _host(files, n, **kw)
    assert out == want and stats == want_stats and stats["kept"] == 1 and stats["optimized"] == 4
    assert len(pieces) == 4                                              # the progressive frame never reaches the device path
    _assert_records_are_the_planners(pieces)
    assert OU.markers(out[0]) == (n, [k % 8 for k in range((300 - 1) // n)] if n else [])


# ------------------------------------------------------------------------------------------------ 4. the store
N_CLIP, CLIP_W, CLIP_H, GRAY_AT, PROGRESSIVE_AT = 22, 64, 48, 5, 11


def _clip(tmp_path):
    from PIL import Image
    files = []
    for i in range(N_CLIP):
        im = Image.fromarray(JU.noise_picture(CLIP_H, CLIP_W, seed=50 + i))
        if i == GRAY_AT:
            files.append(U._save(im.convert("L"), quality=90))
        elif i == PROGRESSIVE_AT:
            files.append(U._save(im, quality=90, subsampling=0, progressive=True))
        else:
            files.append(U._save(im, quality=100 if i % 2 else 97, subsampling=0))     # two quantisation sets
    path = str(tmp_path / "clip.mjpeg")
    JU.write_mjpeg(path, files)
    return path, files


@pytest.mark.parametrize("scale", [1, 2])
def test_optimised_resident_store_serves_the_same_frames(tmp_path, monkeypatch, scale):
    from tstar_amd import jpeg, jpeg_recode as JR, jpeg_resident
    from tstar_amd.video import JpegFrameStore, open_video
    monkeypatch.delenv("TSTAR_JPEG_RECODE", raising=False)
    monkeypatch.delenv("TSTAR_JPEG_RECODE_OPTIMIZE", raising=False)
    path, files = _clip(tmp_path)
    decoded = open_video(path, fps=1.0, jpeg_entropy="device", jpeg_scale=scale)
    plain = open_video(path, fps=1.0, resident="jpeg", pool_frames=6, jpeg_scale=scale)
    std = open_video(path, fps=1.0, resident="jpeg", pool_frames=6, jpeg_scale=scale, recode_blocks=8)
    st = open_video(path, fps=1.0, resident="jpeg", pool_frames=6, jpeg_scale=scale, recode_blocks=8, recode_optimize=True)
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
    assert st.entropy_split_stats == {"split": 0, "abandoned": 0, "rounds_max": 0}          # no segment of a re-coded frame is cut
    geom = JR.covered(files[0])
    host_stats = JR.new_stats(True)
    out = JR.recode_host_chunk(files, geom, 8, None, host_stats)
    assert st.recode_stats == host_stats == {"recoded": N_CLIP - 2, "kept": 2, "bytes_in": sum(map(len, files)), "bytes_out": sum(map(len, out)),
                                             "optimized": N_CLIP - 2, "table_sets": 2}        # one group x two quantisation sets
    assert st.pool_stats()["arena_bytes"] == st.recode_stats["bytes_out"] < std.recode_stats["bytes_out"]
    arena = st.d_arena.cpu().numpy()
    got = [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(st.arena.off, st.arena.len)]
    assert got == out and got[GRAY_AT] == files[GRAY_AT] and got[PROGRESSIVE_AT] == files[PROGRESSIVE_AT]
    U.assert_arenas_equal(st.arena, U.arena_of_plans([(jpeg.plan_segments(out, geom), [len(f) for f in out])]))
    assert (st.arena.frames["n_segments"][[0, 1]] == 6).all()
    if scale == 1:
        monkeypatch.setenv("TSTAR_JPEG_RECODE", "8")
        monkeypatch.setenv("TSTAR_JPEG_RECODE_OPTIMIZE", "1")
        env = open_video(path, fps=1.0, resident="jpeg", pool_frames=6)
        assert env.recode_stats == st.recode_stats and np.array_equal(env.host_frames(secs), want)
        off = open_video(path, fps=1.0, resident="jpeg", pool_frames=6, recode_optimize=False)
        assert off.recode_stats == std.recode_stats
        monkeypatch.delenv("TSTAR_JPEG_RECODE")
        monkeypatch.delenv("TSTAR_JPEG_RECODE_OPTIMIZE")
        # groups of 7: three groups, each with frames of both quantisation sets
        src = jpeg.open_source(path, 1.0)
        try:
            small = jpeg_resident.load_resident(src, "cuda", 6, recode_blocks=8, recode_optimize=True, group_frames=7)
        finally:
            src.close()
        hs = JR.new_stats(True)
        out7 = JR.recode_host_chunk(files, geom, 8, 7, hs)
        assert small.recode_stats == hs and hs["table_sets"] == 6 and np.array_equal(small.host_frames(secs), want)
        arena = small.d_arena.cpu().numpy()
        assert [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(small.arena.off, small.arena.len)] == out7


# ------------------------------------------------------------------------------------------------ 5. the default
def test_the_default_open_and_recode_write_the_standard_tables(tmp_path, monkeypatch):
    from tstar_amd import jpeg_encode as JE, jpeg_recode as JR
    from tstar_amd.video import open_video
    monkeypatch.delenv("TSTAR_JPEG_RECODE", raising=False)
    monkeypatch.delenv("TSTAR_JPEG_RECODE_OPTIMIZE", raising=False)
    path, files = _clip(tmp_path)
    st = open_video(path, fps=1.0, resident="jpeg", pool_frames=6, recode_blocks=8)
    stats = {}
    out = JR.recode_host(files, 8, stats)
    assert st.recode_stats == stats == {"recoded": N_CLIP - 2, "kept": 2, "bytes_in": sum(map(len, files)), "bytes_out": sum(map(len, out))}
    arena = st.d_arena.cpu().numpy()
    assert [arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(st.arena.off, st.arena.len)] == out
    dstats = {}
    assert JE.recode_frames(files, 8, stats=dstats, optimize=False) == out and dstats == stats
    ostats = {}
    assert JE.recode_frames(files, 8, stats=ostats, optimize=True) == JE.recode_frames(files, 8, device=False, optimize=True)
    assert set(ostats) == set(stats) | {"optimized", "table_bytes"}
