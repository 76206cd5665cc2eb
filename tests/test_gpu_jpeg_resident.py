"""GPU: the compressed-resident JPEG store -- open_video(resident="jpeg") against the decoded store, byte for byte; the gather kernel
against its host mirror, word for word; tstar_jpeg_reconstruct_slots against tstar_jpeg_reconstruct; leases on two streams; whole
searches on both stores; the refusals.  Every comparison is an equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_resident_util as RU  # noqa: E402
import jpeg_util as JU  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_CLIP = 40


def _clip(tmp_path, mix, n=N_CLIP):
    datas = RU.mix_frames(mix, n)
    path = str(tmp_path / f"{mix}.mjpeg")
    JU.write_mjpeg(path, datas)
    return path, datas


@pytest.mark.parametrize("mix", sorted(RU.MIXES))
def test_resident_store_equals_the_decoded_store(tmp_path, mix):
    """A pool of 4 slots over 40 frames: requests of 1 to 4 seconds, shuffled, with repeats, until every slot has been evicted and
    refilled many times -- host_frames, jpeg_frames and source_frames against the decoded store and the file."""
    from tstar_amd.video import JpegFrameStore, open_video
    path, datas = _clip(tmp_path, mix)
    plain = open_video(path, fps=1.0, jpeg_entropy="device")
    st = open_video(path, fps=1.0, resident="jpeg", pool_frames=4)
    assert isinstance(st, JpegFrameStore) and st.shape == plain.shape == (N_CLIP, *RU.MIXES[mix][:2], 3)
    assert (st.num_seconds, st.raw_fps, st.raw_total_frames, st.fmt, st.lease_frames) == (N_CLIP, 1.0, N_CLIP, "rgb", 4)
    assert st.decode_stats == plain.decode_stats and st.entropy_stats == plain.entropy_stats
    assert st.entropy_split_stats == plain.entropy_split_stats
    want = plain.frames.cpu().numpy()
    n_exc = 1 if mix == "progressive" else 0
    assert st.pool_stats()["exceptions"] == n_exc and st.pool_stats()["arena_bytes"] == sum(len(d) for d in datas)
    assert st.pool_stats()["pool_bytes"] == (4 + n_exc) * want[0].size
    rs = np.random.RandomState(7)
    for call in range(48):
        k = 1 + call % 4
        secs = [int(v) for v in rs.choice(N_CLIP, size=k, replace=False)]
        if call % 3 == 0:
            secs = (secs + secs[:1])[:4] if k < 4 else secs[:2] + secs[:2]          # a second named twice
        got = st.host_frames(secs)
        assert np.array_equal(got, want[secs]), f"call {call}: seconds {secs}"
    ps = st.pool_stats()
    assert ps["evictions"] >= 40 and ps["misses"] == ps["evictions"] + 4 and st.fetch_errors() == 0
    if mix == "long-noise":
        # a fetch queues the rounds the open saw the file need (noise needs many) and every cut segment still converges: none falls to one lane
        assert 1 <= st._max_rounds == plain.entropy_split_stats["rounds_max"] <= 48 and plain.entropy_split_stats["abandoned"] == 0
        st.flush()
        st.host_frames([5, 6, 7])
        info = st._d_status[st._cap_segments:st._cap_segments + 3].cpu().numpy()
        assert (info > 0).all() and info.max() <= st._max_rounds, info
    assert np.array_equal(st.host_frames(list(range(N_CLIP))), want)                # more seconds than slots: served in pieces
    assert np.array_equal(st.host_frames([]), want[:0])
    some = [3, RU.PROGRESSIVE_AT, 39, 3, 17, 0, 21]
    assert st.source_frames(some) == [datas[s] for s in some]
    assert st.jpeg_frames(some, quality=80) == plain.jpeg_frames(some, quality=80)
    assert st.fetch_errors() == 0


def test_seconds_of_one_byte_range_share_an_arena_entry(tmp_path):
    """At half a frame per second two seconds name each raw frame: one arena entry, one slot, one decode."""
    from tstar_amd.video import open_video
    path, datas = _clip(tmp_path, "72x128-422", 12)
    plain = open_video(path, fps=0.5, jpeg_entropy="device")
    st = open_video(path, fps=0.5, resident="jpeg", pool_frames=3)
    assert st.num_seconds == plain.num_seconds == 24 and st.arena.n_entries == 12
    assert st.pool_stats()["arena_bytes"] == sum(len(d) for d in datas)
    assert st.decode_stats == plain.decode_stats and st.entropy_stats == plain.entropy_stats
    lease = st.lease([4, 5, 4, 6])
    assert lease.idx.tolist()[0] == lease.idx.tolist()[1] == lease.idx.tolist()[2] != lease.idx.tolist()[3]
    lease.done()
    assert st.pool_stats()["misses"] == 2
    assert np.array_equal(st.host_frames(list(range(24))), plain.frames.cpu().numpy())


def _upload(arena, dev):
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to(dev)       # noqa: E731
    return dict(bytes=up(arena.bytes, np.uint8), off=up(arena.off, np.int64), len=up(arena.len, np.int32), quant=up(arena.quant, np.int16),
                frames=up(arena.frames, np.int32), segments=up(arena.segments, np.int32))


def _gather_device(arena, d, ids, guard=64):
    """tstar_jpeg_gather into a buffer between ``guard`` sentinel bytes -> the batch as numpy."""
    from tstar_amd import _lib, jpeg_resident as JR
    desc, total, nseg = JR.gather_descriptor(ids, arena.len, arena.frames["n_segments"])
    nbytes = JR.gather_layout(total, len(desc), nseg)[0]
    dev = d["bytes"].device
    buf = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    d_desc = torch.from_numpy(desc.view(np.int32).copy()).to(dev)
    _lib.check(_lib.load().tstar_jpeg_gather(d["bytes"].data_ptr(), d["bytes"].numel(), d["off"].data_ptr(), d["len"].data_ptr(),
                                            d["quant"].data_ptr(), d["frames"].data_ptr(), d["segments"].data_ptr(), arena.n_entries,
                                            len(arena.segments), desc.ctypes.data, d_desc.data_ptr(), len(desc), total, nseg,
                                            buf.data_ptr() + guard, nbytes, _lib.stream_ptr()), "tstar_jpeg_gather")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:guard] == 0xA5).all() and (out[-guard:] == 0xA5).all(), "a write outside the batch buffer"
    return out[guard:-guard]


def test_gather_kernel_equals_its_mirror_on_a_crafted_arena():
    """Frames of 0 .. 20 000 bytes starting at every offset mod 16 (aligned vectors, shifted pairs, byte heads and tails; more than one
    workgroup per frame), shuffled with repeats: the kernel's buffer is the mirror's, word for word, between untouched sentinels."""
    arena = RU.crafted_arena(seed=3)
    d = _upload(arena, "cuda")
    rs = np.random.RandomState(1)
    E = arena.n_entries
    lists = [list(range(E)), [0, 19, 0], [17], [16, 16, 17, 16]] + [[int(v) for v in rs.randint(0, E, size=n)] for n in (1, 2, 7, 33)]
    for ids in lists:
        want, _ = arena.gather_host(ids)
        got = _gather_device(arena, d, ids)
        diff = np.nonzero(got != want)[0]
        assert len(diff) == 0, f"ids {ids}: {len(diff)} bytes differ, first at {int(diff[0])}"


def test_gather_kernel_checks_the_device_words_itself():
    """The launcher checks the host's copy of the descriptor; the kernel reads the device's.  Where the two differ -- an id outside
    the arena, a length that is not the arena's, a destination outside the batch -- the kernel copies nothing for that frame and
    stays inside the buffer; the launcher refuses a bad host copy before any launch."""
    from tstar_amd import _lib, jpeg_resident as JR
    lib = _lib.load()
    arena = RU.crafted_arena(seed=4)
    d = _upload(arena, "cuda")
    ids = [15, 13, 16]
    desc, total, nseg = JR.gather_descriptor(ids, arena.len, arena.frames["n_segments"])
    nbytes, q_at, f_at, s_at = JR.gather_layout(total, 3, nseg)
    want, _ = arena.gather_host(ids)

    def run(h_desc, dev_desc):
        buf = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device="cuda")
        d_desc = torch.from_numpy(dev_desc.view(np.int32).copy()).cuda()
        rc = lib.tstar_jpeg_gather(d["bytes"].data_ptr(), d["bytes"].numel(), d["off"].data_ptr(), d["len"].data_ptr(), d["quant"].data_ptr(),
                                   d["frames"].data_ptr(), d["segments"].data_ptr(), arena.n_entries, len(arena.segments), h_desc.ctypes.data,
                                   d_desc.data_ptr(), 3, total, nseg, buf.data_ptr() + 64, nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:64] == 0xA5).all() and (out[-64:] == 0xA5).all(), "a write outside the batch buffer"
        return rc, out[64:-64]

    for field, value in (("id", arena.n_entries), ("len", int(desc["len"][1]) - 1), ("dst", total), ("first_segment", nseg), ("dst", 8)):
        bad = desc.copy()
        bad[field][1] = value
        rc, got = run(desc, bad)
        assert rc == 0
        fr = got[f_at:f_at + 48].view(np.int32).reshape(3, 4)
        assert fr[1, 0] == -1 and fr[0, 0] == arena.frames["table_set"][15] and fr[2, 0] == arena.frames["table_set"][16], field
        o0, o2 = int(desc["dst"][0]), int(desc["dst"][2])
        assert np.array_equal(got[o0:o0 + 4097], want[o0:o0 + 4097]) and np.array_equal(got[o2:o2 + 16384], want[o2:o2 + 16384]), field
        o1, n1 = int(desc["dst"][1]), (int(desc["len"][1]) + 15) & ~15
        assert (got[o1:o1 + n1] == (0 if field in ("id", "len") else 0xA5)).all(), field       # zeros, or never written at all
        if field != "len":                                          # the arena's lengths are the device's to know
            rc, got = run(bad, desc)
            assert rc != 0 and (got == 0xA5).all(), f"{field}: a bad host descriptor must be refused before any launch"


@pytest.mark.parametrize("size,sampling", [((17, 33), "420"), ((72, 128), "422"), ((17, 33), "gray")])
def test_reconstruct_slots_equals_reconstruct(size, sampling):
    """Slots out of order, one skipped below and one above the pool, 64 sentinel bytes on both sides of the pool.  17 x 33: a frame is
    1683 bytes, the byte-store form; 72 x 128: the dword form."""
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    H, W = size
    datas = [JU.encode(JU.noise_picture(H, W, seed=50 + i), sampling, 85) for i in range(5)]
    geom = RU.geometry(datas)
    coef, quant, status = RU.host_coefficients(datas, geom)
    assert not status.any()
    blocks, plane_bytes = jpeg._sizes(geom)
    d_coef, d_quant = torch.from_numpy(coef).cuda(), torch.from_numpy(quant.view(np.int16)).cuda()
    planes = torch.empty(5 * plane_bytes, dtype=torch.uint8, device="cuda")
    ref = torch.empty((5, H, W, 3), dtype=torch.uint8, device="cuda")
    _lib.check(lib.tstar_jpeg_reconstruct(d_coef.data_ptr(), d_quant.data_ptr(), 5, *geom, planes.data_ptr(), ref.data_ptr(), _lib.stream_ptr()),
               "tstar_jpeg_reconstruct")
    ref = ref.cpu().numpy()
    P, per = 6, H * W * 3
    slots = [4, -1, 0, 6, 2]
    buf = torch.full((64 + P * per + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_slots = torch.tensor(slots, dtype=torch.int32, device="cuda")
    _lib.check(lib.tstar_jpeg_reconstruct_slots(d_coef.data_ptr(), d_quant.data_ptr(), 5, *geom, planes.data_ptr(), buf.data_ptr() + 64, P,
                                                d_slots.data_ptr(), _lib.stream_ptr()), "tstar_jpeg_reconstruct_slots")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:64] == 0xA5).all() and (out[-64:] == 0xA5).all(), "a write outside the pool"
    pool = out[64:-64].reshape(P, H, W, 3)
    for j, s in enumerate(slots):
        if 0 <= s < P:
            assert np.array_equal(pool[s], ref[j]), f"frame {j} in slot {s}"
    for s in (1, 3, 5):
        assert (pool[s] == 0xA5).all(), f"slot {s} was written"
    if JU.turbo():
        assert np.array_equal(ref[0], JU.pillow_rgb(datas[0]))


def test_a_lease_on_one_stream_survives_fetches_on_another(tmp_path):
    """Pool of 4.  Stream A leases seconds 0, 1 and keeps them; stream B fills the rest of the pool, is done, and fetches again: it
    gets B's old slots, never A's.  After A is done, a fetch of four frames on B reuses A's slots behind A's reads."""
    from tstar_amd.video import open_video
    path, _ = _clip(tmp_path, "72x128-420")
    want = open_video(path, fps=1.0, jpeg_entropy="device").frames
    st = open_video(path, fps=1.0, resident="jpeg", pool_frames=4)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(a):
        l1 = st.lease([0, 1])
        held = set(l1.idx.tolist())
    with torch.cuda.stream(b):
        l2 = st.lease([2, 3])
        got2 = l2.frames.index_select(0, l2.idx.long())
        l2.done()
        with pytest.raises(ValueError, match="pool_frames=4"):
            st.lease([4, 5, 6])                                     # two slots are A's
        l3 = st.lease([4, 5])
        assert not held & set(l3.idx.tolist())
        got3 = l3.frames.index_select(0, l3.idx.long())
        l3.done()
    with torch.cuda.stream(a):
        got1 = l1.frames.index_select(0, l1.idx.long())             # read under the first lease, after B's fetches were queued
        l1.done()
    with torch.cuda.stream(b):
        l4 = st.lease([6, 7, 8, 9])                                  # every slot, A's two included: B waits for A's reads
        assert held <= set(l4.idx.tolist())
        got4 = l4.frames.index_select(0, l4.idx.long())
        l4.done()
    torch.cuda.synchronize()
    assert torch.equal(got1, want[[0, 1]]) and torch.equal(got2, want[[2, 3]]) and torch.equal(got3, want[[4, 5]])
    assert torch.equal(got4, want[[6, 7, 8, 9]]) and st.fetch_errors() == 0
    assert st.pool_stats()["misses"] == 10 and st.pool_stats()["hits"] == 0


# ---- whole searches ------------------------------------------------------------------------------------------------------------
N_SEARCH, GRID, KEYS = 120, 4, 4
QUESTIONS = [(["couch"], ["tv", "chair"], 11), (["dog", "lamp"], ["road"], 12), (["cup"], ["table"], 13)]


@pytest.fixture(scope="module")
def search_avi(tmp_path_factory):
    """120 frames of the synthetic video at 72 x 128 as a Motion-JPEG AVI, one frame per second."""
    from tstar_amd.video import synthetic_frames_numpy
    frames = synthetic_frames_numpy(range(N_SEARCH), N_SEARCH, 72, 128, seed=3)
    path = str(tmp_path_factory.mktemp("resident") / "search.avi")
    JU.write_avi(path, [JU.encode(f, "420", 90) for f in frames], 128, 72, rate=1)
    return path


def _searcher(h, store, q):
    from tstar_amd.interface_searcher import TStarSearcher
    targets, cues, seed = q
    return TStarSearcher(store, h, list(targets), list(cues), search_nframes=KEYS, image_grid_shape=(GRID, GRID), search_budget=0.5,
                         confidence_threshold=0.6, rng=np.random.RandomState(seed), keep_visual_history=True)


def _record(s, frames, ts):
    return dict(frames=torch.as_tensor(np.asarray(frames)), ts=list(ts), sd=torch.as_tensor(np.array(s.score_distribution)),
                scores=[torch.as_tensor(np.asarray(v)) for v in s.Score_history], P=[torch.as_tensor(np.asarray(v)) for v in s.P_history],
                boxes=[torch.as_tensor(np.asarray(x)) for it in s.detect_bbox_iters for d in it for x in (d.xyxy, d.confidence, d.class_id)],
                iterations=s.iterations, frames_scored=s.frames_scored)


def _assert_same(a, b, what):
    assert a["ts"] == b["ts"] and torch.equal(a["frames"], b["frames"]) and torch.equal(a["sd"], b["sd"]), what
    for key in ("scores", "P", "boxes"):
        assert len(a[key]) == len(b[key]) and all(torch.equal(x, y) for x, y in zip(a[key], b[key])), f"{what}: {key}"
    assert (a["iterations"], a["frames_scored"]) == (b["iterations"], b["frames_scored"]), what


@pytest.mark.parametrize("cache", [0, 16])
@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_searches_on_the_resident_store_equal_the_decoded_store(search_avi, mode, cache, monkeypatch):
    """TStarSearcher alone and in a lock-step group of 3 over one store, pool_frames=32 at a 4 x 4 grid: keyframes, timestamps, score
    distribution, score and P history and the visual history's boxes are those of the decoded store, bit for bit."""
    from tstar_amd import lockstep
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.video import open_video
    monkeypatch.setattr(lockstep, "_AHEAD_ALWAYS", True)
    runs = {}
    for kind in ("plain", "resident"):
        store = open_video(search_avi, jpeg_entropy="device") if kind == "plain" else open_video(search_avi, resident="jpeg", pool_frames=32)
        h = OWLInterface(synthetic_seed=0, max_batch=16, weights_dtype=mode, input_size=(64, 96), feature_cache_frames=cache)
        s = _searcher(h, store, QUESTIONS[0])
        solo = _record(s, *s.search())
        group = [_searcher(h, store, q) for q in QUESTIONS]
        res = lockstep.search_lockstep(group)
        runs[kind] = [solo] + [_record(g, fr, ts) for g, (fr, ts) in zip(group, res)]
        h.scorer.close()
        if kind == "resident":
            ps = store.pool_stats()
            assert store.fetch_errors() == 0 and ps["misses"] > 32 and ps["evictions"] > 0 and ps["hits"] > 0
    assert runs["plain"][0]["iterations"] >= 2 and len(runs["plain"][0]["boxes"]) > 0
    for i, (a, b) in enumerate(zip(runs["resident"], runs["plain"])):
        _assert_same(a, b, "solo search" if i == 0 else f"lock-step item {i - 1}")


def test_refusals(tmp_path):
    from tstar_amd.video import open_video
    path, _ = _clip(tmp_path, "17x33-444", 8)
    st = open_video(path, fps=1.0, resident="jpeg", pool_frames=4)
    with pytest.raises(ValueError, match="pool_frames=4"):
        st.lease([0, 1, 2, 3, 4])
    assert st.pool_stats()["misses"] == 0
    lease = st.lease([0, 1, 2, 3, 3, 0])                              # four distinct frames fit
    lease.done()
    with pytest.raises(IndexError):
        st.lease([8])
    with pytest.raises(AttributeError, match="lease"):
        st.frames
    with pytest.raises(ValueError, match="synthetic://n=8"):
        open_video("synthetic://n=8,h=72,w=128", resident="jpeg")
    with pytest.raises(ValueError, match="GPU store"):
        open_video(path, fps=1.0, device="cpu", resident="jpeg")
