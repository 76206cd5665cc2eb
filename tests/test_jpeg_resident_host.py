"""CPU: the compressed-resident JPEG store without a GPU -- the gather's host mirror (tstar_jpeg_gather_host) over arena records,
the pool's bookkeeping (jpeg_resident.SlotPool), the stand-alone sanitizer program, and the lease of a decoded store."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_resident_util as RU  # noqa: E402
import jpeg_util as JU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decode_batch(buf, plan, geom):
    """A gathered batch through both host decoders -> coefficients (the two must agree, every segment OK)."""
    from tstar_amd import jpeg
    coef, status = jpeg.entropy_segments_host(buf, plan, geom)
    coef2, status2, info = jpeg.entropy_split_host(buf, plan, geom)
    assert not status.any() and not status2.any(), (status, status2)
    assert np.array_equal(coef, coef2)
    return coef, info


def reconstruct(coef, quant, geom):
    from tstar_amd import _lib
    out = np.empty((len(coef), geom[1], geom[0], 3), dtype=np.uint8)
    _lib.check(_lib.load().tstar_jpeg_reconstruct_host(coef.ctypes.data, np.ascontiguousarray(quant).ctypes.data, len(coef), *geom,
                                                       out.ctypes.data, 0), "tstar_jpeg_reconstruct_host")
    return out


@pytest.mark.parametrize("mix", sorted(RU.MIXES))
def test_gathered_batch_decodes_to_the_frames(mix):
    """A batch the mirror builds from arena records for a shuffled id list with repeats decodes, through tstar_jpeg_entropy_split_host
    and tstar_jpeg_entropy_segments_host, to the coefficients tstar_jpeg_entropy_batch gives for those frames, and reconstructs to
    Pillow's bytes.  The arena is planned in chunks of 4 with filler between them, so frames start at odd offsets and table sets
    and segments are numbered over the whole file."""
    from tstar_amd import jpeg
    datas = RU.mix_frames(mix, 7)
    geom = RU.geometry(datas)
    arena, route = RU.build_arena(datas, geom, chunk=4, gap=3)
    want_c, want_q, want_s = RU.host_coefficients(datas, geom)
    ok = [i for i in range(len(datas)) if route[i] == jpeg.ROUTE_DEVICE]
    if mix == "progressive":
        assert ok == [i for i in range(len(datas)) if i != RU.PROGRESSIVE_AT] and want_s[RU.PROGRESSIVE_AT] == jpeg.UNCOVERED
        assert arena.frames["table_set"][RU.PROGRESSIVE_AT] == -1 and arena.frames["n_segments"][RU.PROGRESSIVE_AT] == 0
    else:
        assert len(ok) == len(datas)
    if mix == "optimize":
        assert len(arena.table_sets) == len(datas)                    # a set per frame, none lost or merged across chunks
    if mix == "restart3":
        assert (arena.frames["n_segments"] > 8).all()
    for e in ok:                                                      # segments count from the frame's first byte
        fr = arena.frames[e]
        seg = arena.segments[fr["first_segment"]:fr["first_segment"] + fr["n_segments"]]
        assert (seg["frame"] == e).all() and (seg["end"] + 2 <= arena.len[e]).all() and (seg["begin"] <= seg["end"]).all()
    ids = RU.shuffled_ids(ok, seed=len(mix))
    buf, plan = arena.gather_host(ids)
    assert (plan.offsets % 16 == 0).all() and (plan.frames["first_segment"] == np.cumsum(plan.frames["n_segments"]) - plan.frames["n_segments"]).all()
    for j, e in enumerate(ids):                                       # the bytes are the files', the padding zeros
        o, n = int(plan.offsets[j]), len(datas[e])
        assert buf[o:o + n].tobytes() == datas[e] and not buf[o + n:(o + n + 15) & ~15].any()
    coef, info = decode_batch(buf, plan, geom)
    if mix == "long-noise":
        assert min(len(d) for d in datas) > jpeg.SPLIT_MIN_BYTES and (info > 0).all()       # the split path did the work
    assert np.array_equal(coef, want_c[ids]) and np.array_equal(plan.quant, want_q[ids])
    if not JU.turbo():
        pytest.skip("Pillow on this machine is not built on libjpeg-turbo: its bytes are not the yardstick of the byte-equality")
    rgb = reconstruct(coef, plan.quant, geom)
    for j, e in enumerate(ids):
        assert np.array_equal(rgb[j], JU.pillow_rgb(datas[e])), f"frame {e} at position {j}"


def test_mirror_refuses_bad_descriptors():
    """Ids outside the arena, a short buffer and a batch of 2^32 bytes are errors before anything is written."""
    from tstar_amd import _lib, jpeg_resident as JR
    datas = RU.mix_frames("17x33-420", 3)
    geom = RU.geometry(datas)
    arena, _ = RU.build_arena(datas, geom)
    with pytest.raises(ValueError, match="outside the arena"):
        arena.gather_host([0, 3])
    with pytest.raises(ValueError, match="outside the arena"):
        arena.gather_host([-1])
    buf = np.full(64, 0xA5, dtype=np.uint8)
    with pytest.raises(_lib.TStarHipError, match="shorter than tstar_jpeg_gather_bytes"):
        arena.gather_host([0, 1], buf=buf)
    assert (buf == 0xA5).all()
    with pytest.raises(ValueError, match="32 bits"):
        JR.gather_descriptor([0] * 5, np.array([1 << 30], dtype=np.uint32), np.array([1], dtype=np.int32))
    assert _lib.load().tstar_jpeg_gather_bytes(1 << 32, 1, 1, None) == 0 and _lib.load().tstar_jpeg_gather_bytes(24, 1, 1, None) == 0
    assert JR.gather_layout(32, 2, 3) == (32 + 2 * 384 + 2 * 16 + 80, 32, 32 + 768, 32 + 768 + 32)


def test_frame_beyond_4_gib_of_arena():
    """One frame at arena offset 2^32 + 5 (a lazily allocated host buffer: only the frame's pages are touched) gathers and decodes
    like the same frame at offset 0: the offsets are 64-bit all the way."""
    from tstar_amd import jpeg, jpeg_resident as JR
    data = RU.mix_frames("72x128-420", 1)[0]
    geom = RU.geometry([data])
    at = (1 << 32) + 5
    try:
        big = np.zeros(at + len(data), dtype=np.uint8)
    except MemoryError:
        pytest.skip("no 4 GiB of address space for the arena")
    big[at:] = np.frombuffer(data, dtype=np.uint8)
    b = JR.ArenaBuilder()
    b.add(jpeg.plan_segments([data], geom), [len(data)], base=at)
    arena = b.finish(big)
    assert int(arena.off[0]) == at and arena.off.dtype == np.uint64
    buf, plan = arena.gather_host([0, 0])
    coef, _ = decode_batch(buf, plan, geom)
    want, _, _ = RU.host_coefficients([data], geom)
    assert np.array_equal(coef[0], want[0]) and np.array_equal(coef[1], want[0])
    # an arena that ends before the frame does: nothing is read, the frame is zeros and its segments name no frame
    buf, plan = arena.gather_host([0], arena_bytes=at + 10)
    assert not buf[:len(data)].any() and plan.frames["table_set"][0] == -1 and (plan.segments["frame"] == 0xFFFFFFFF).all()
    _, status = jpeg.entropy_segments_host(buf, plan, geom)
    assert (status == jpeg.MALFORMED).all()


def test_slot_pool_bookkeeping():
    """Hits, LRU order, repeated entries, leased slots, the pool_frames refusal and permanent exception slots."""
    from tstar_amd.jpeg_resident import SlotPool
    p = SlotPool(3, exceptions=[7, 9])
    slots, fill, waits = p.acquire([5, 7, 5, 6, 9], key="A")
    assert slots[0] == slots[2] and slots[1] == 3 and slots[4] == 4 and len({slots[0], slots[3]}) == 2 and max(slots[0], slots[3]) < 3
    assert fill == [(5, slots[0]), (6, slots[3])] and waits == [] and (p.hits, p.misses, p.evictions) == (0, 2, 0)
    p.filled([s for _, s in fill], "A", "fillA")
    # a leased slot is not handed out again before done: one slot is free, two new frames do not fit, and nothing changed
    with pytest.raises(ValueError, match="pool_frames=3"):
        p.acquire([1, 2], key="A")
    assert (p.hits, p.misses) == (0, 2) and p.slot_of == {5: slots[0], 6: slots[3]}
    s2, fill2, waits2 = p.acquire([1, 5], key="B")                     # a hit from another stream waits for the fill
    assert s2[1] == slots[0] and fill2 == [(1, s2[0])] and s2[0] not in (slots[0], slots[3]) and waits2 == ["fillA"]
    p.filled([s2[0]], "B", "fillB")
    p.release(slots, "A", "doneA")                                     # 5 is still held by the second lease, 6 is idle now
    assert list(p.idle) == [slots[3]]
    p.release(s2, "B", "doneB")
    assert list(p.idle) == [slots[3], s2[0], slots[0]]                 # least recently released first
    # LRU: the next miss takes 6's slot and waits for its reader on the other stream and for its fill; exceptions never move
    s3, fill3, waits3 = p.acquire([8, 9], key="B")
    assert fill3 == [(8, slots[3])] and s3 == [slots[3], 4] and sorted(waits3) == ["doneA", "fillA"] and p.evictions == 1 and 6 not in p.slot_of
    p.release(s3, "B", "doneB2")
    s4, fill4, waits4 = p.acquire([1, 5, 8], key="B")                  # all resident: hits only, same-stream fills need no wait
    assert fill4 == [] and waits4 == ["fillA"] and (p.hits, p.misses) == (4, 4)
    p.release(s4, "B", "doneB3")
    # every slot is evicted and refilled in release order; permanent slots are not counted against the pool
    s5, fill5, _ = p.acquire([10, 11, 12, 7, 9], key="A")
    assert [s for _, s in fill5] == s4 and s5[3:] == [3, 4] and p.evictions == 4
    with pytest.raises(ValueError, match="pool_frames=3"):
        p.acquire([13], key="A")
    p.forget(fill5)
    p.release(s5)
    assert p.slot_of == {} and len(p.idle) == 3
    # flush forgets what no lease holds; the slots still wait for their last readers
    one = SlotPool(1)
    s6, fill6, _ = one.acquire([20], key="A")
    one.filled(s6, "A", "fill6")
    assert one.flush() == 0                                             # held by a lease: stays
    one.release(s6, "A", "done6")
    assert one.flush() == 1 and one.slot_of == {}
    s7, fill7, waits7 = one.acquire([20], key="B")
    assert fill7 == [(20, 0)] and sorted(waits7) == ["done6", "fill6"] and one.evictions == 0


def test_resident_sanitizer_program(tmp_path):
    """csrc/jpeg_resident_check_main.cpp with the mirror, built with -fsanitize=address,undefined (a stand-alone CPU program; nothing
    is loaded into python, nothing of the GPU is involved): descriptors with out-of-range ids, short capacities, zero-length
    frames and arenas whose records point outside them, on exact-size heap blocks.  The mirror must refuse or stay in bounds."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_resident_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_resident_host.cpp"), os.path.join(csrc, "jpeg_resident_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for seed in ("1", "2", "3"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert r.stdout.strip() == "cases=70 refused=21 zeroed=9 differ=0", r.stdout


def test_plain_store_lease_is_the_store():
    """A decoded store leases its own tensor, the seconds as positions, and done() changes nothing."""
    import torch
    from tstar_amd.video import FrameStore
    t = torch.arange(5 * 2 * 3 * 3, dtype=torch.uint8).reshape(5, 2, 3, 3)
    st = FrameStore(t, 1.0)
    assert st.device == t.device and st.lease_frames is None
    lease = st.lease([4, 0, 4])
    assert lease.frames is t and lease.N == 5 and lease.idx.dtype == torch.int32 and lease.idx.tolist() == [4, 0, 4]
    lease.done()
    lease.done()
    given = torch.tensor([1, 2], dtype=torch.int32)
    assert st.lease([1, 2], given).idx is given
    assert np.array_equal(st.host_frames([3, 3, 1]), t[[3, 3, 1]].numpy()) and st.host_frames([]).shape == (0, 2, 3, 3)


def test_resident_options(monkeypatch):
    from tstar_amd import jpeg_resident as JR
    monkeypatch.delenv("TSTAR_JPEG_RESIDENT", raising=False)
    monkeypatch.delenv("TSTAR_JPEG_POOL", raising=False)
    assert JR.resident_mode() is None and JR.resident_mode("jpeg") == "jpeg" and JR.pool_size() == 512 and JR.pool_size(7) == 7
    monkeypatch.setenv("TSTAR_JPEG_RESIDENT", "1")
    monkeypatch.setenv("TSTAR_JPEG_POOL", "40")
    assert JR.resident_mode() == "jpeg" and JR.pool_size() == 40 and JR.pool_size(8) == 8
    monkeypatch.setenv("TSTAR_JPEG_RESIDENT", "0")
    assert JR.resident_mode() is None
    with pytest.raises(ValueError, match="resident='nv12'"):
        JR.resident_mode("nv12")
    with pytest.raises(ValueError, match="pool_frames=0"):
        JR.pool_size(0)
