"""CPU: the device entropy stage without a GPU -- the segment planner and the kernel's decode core run on the host
(tstar_jpeg_plan_segments + tstar_jpeg_entropy_segments_host) against the sequential host decoder
(tstar_jpeg_entropy_batch), which is the yardstick: same coefficients, same quantisation rows, same statuses."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_decode(datas, geom):
    """The yardstick: (coef int16 [n, blocks * 64], quant uint16 [n, 192], status int32 [n])."""
    from tstar_amd import jpeg
    blocks = jpeg._sizes(geom)[0]
    coef = np.zeros((len(datas), blocks * 64), dtype=np.int16)
    quant = np.zeros((len(datas), 192), dtype=np.uint16)
    status, _ = jpeg.entropy_batch(datas, geom, coef, quant)
    return coef, quant, status


def segments_decode(datas, geom, guard=4096):
    """plan + the decode core on the CPU, every output between sentinels -> (plan, coef, seg_status)."""
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    plan = jpeg.plan_segments(datas, geom)
    n, nseg = len(datas), len(plan.segments)
    blocks = jpeg._sizes(geom)[0]
    buf = np.frombuffer(b"".join(datas), dtype=np.uint8)
    assert plan.total_bytes == len(buf)
    coef = np.full(n * blocks * 64 + 2 * guard, 0x5A5A, dtype=np.int16)
    status = np.full(nseg + 2 * guard, 0x5A5A5A5A, dtype=np.int32)
    if nseg:
        rc = lib.tstar_jpeg_entropy_segments_host(buf.ctypes.data, len(buf), plan.segments.ctypes.data, plan.table_sets.ctypes.data,
                                                  len(plan.table_sets), plan.frames.ctypes.data, n, nseg, *geom,
                                                  coef[guard:].ctypes.data, status[guard:].ctypes.data)
        assert rc == 0
    for arr, fill in ((coef, 0x5A5A), (status, 0x5A5A5A5A)):
        assert (arr[:guard] == fill).all() and (arr[-guard:] == fill).all(), "a write outside the output buffers"
    return plan, coef[guard:-guard].reshape(n, blocks * 64), status[guard:guard + nseg]


def check_streams(datas, geom):
    """Every stream of the batch: routed to the host only when the sequential decoder does not accept it; else the status of its
    first segment that is not OK is that decoder's status; coefficients and tables of accepted frames identical (so no other
    frame of the batch wrote into their region either).  Returns the number of device-routed streams."""
    from tstar_amd import jpeg
    want_c, want_q, want_s = host_decode(datas, geom)
    plan, coef, seg_status = segments_decode(datas, geom)
    got = plan.frame_status(seg_status)
    for i in range(len(datas)):
        if plan.route[i] == jpeg.ROUTE_HOST:
            assert want_s[i] != jpeg.OK, f"stream {i}: the sequential decoder accepts it, the planner does not"
            assert plan.frames["table_set"][i] == -1 and plan.frames["n_segments"][i] == 0 and not plan.quant[i].any()
            continue
        assert got[i] == want_s[i], f"stream {i}: segments say {got[i]}, the sequential decoder {want_s[i]}"
        if want_s[i] == jpeg.OK:
            assert np.array_equal(coef[i], want_c[i]) and np.array_equal(plan.quant[i], want_q[i]), f"stream {i}"
    return int((plan.route == jpeg.ROUTE_DEVICE).sum())


@pytest.mark.parametrize("quality", JU.QUALITIES)
@pytest.mark.parametrize("sampling", JU.SAMPLINGS)
@pytest.mark.parametrize("size", JU.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_segments_equal_the_sequential_decoder(size, sampling, quality):
    """The whole matrix, one batch per cell (default, optimised and restart tables; synthetic and noise).  Every well-formed file
    takes the device route: the allowed host-routed share is 0."""
    from tstar_amd import jpeg
    H, W = size
    files = JU.matrix_files(H, W, sampling, quality)
    datas = [d for _, d in files] + [JU.strip_dht(d) for lab, d in files if lab.endswith("default")]
    rc, geom, _ = jpeg.probe(datas[0])
    assert rc == jpeg.OK
    want_c, want_q, want_s = host_decode(datas, geom)
    assert not want_s.any()
    plan, coef, seg_status = segments_decode(datas, geom)
    assert (plan.route == jpeg.ROUTE_DEVICE).all(), [files[i][0] for i in np.nonzero(plan.route)[0] if i < len(files)]
    assert not seg_status.any() and not plan.frame_status(seg_status).any()
    assert np.array_equal(plan.quant, want_q)
    assert np.array_equal(coef, want_c)
    # the records themselves: segments tile every frame's MCUs in order, offsets stay inside the frame's bytes
    offsets, total = jpeg.pack_offsets(datas)
    mcus = ((W + 8 * geom[3] - 1) // (8 * geom[3])) * ((H + 8 * geom[4] - 1) // (8 * geom[4]))
    for i, d in enumerate(datas):
        fr = plan.frames[i]
        segs = plan.segments[fr["first_segment"]:fr["first_segment"] + fr["n_segments"]]
        assert (segs["frame"] == i).all() and list(segs["last"]) == [0] * (len(segs) - 1) + [1]
        assert segs["first_mcu"][0] == 0 and np.array_equal(segs["first_mcu"][1:], np.cumsum(segs["n_mcu"])[:-1]) and segs["n_mcu"].sum() == mcus
        assert (segs["begin"] <= segs["end"]).all() and segs["begin"][0] >= offsets[i] and segs["end"][-1] + 2 <= offsets[i] + len(d)
    # default tables with and without DHT, and the restart files, share their tables; the optimised files bring their own
    assert 1 <= len(plan.table_sets) <= 3


MUTATION_FILES = [("420", "default"), ("422", "restart"), ("444", "optimize"), ("gray", "default"), ("420", "restart")]


@pytest.mark.parametrize("sampling,tables", MUTATION_FILES)
def test_truncated_streams_have_the_sequential_decoders_status(sampling, tables):
    from tstar_amd import jpeg
    data = JU.encode(JU.noise_picture(97, 301, seed=3), sampling, 75, tables)
    geom = jpeg.probe(data)[1]
    datas = [data] + [data[:n] for n in range(0, len(data), 97)] + [data[:-1], data[:-2]]
    assert len(datas) > 50
    assert check_streams(datas, geom) >= 1
    # nothing truncated is accepted by either side
    plan, _, seg_status = segments_decode(datas, geom)
    assert plan.route[0] == jpeg.ROUTE_DEVICE and plan.frame_status(seg_status)[0] == jpeg.OK
    assert (plan.frame_status(seg_status)[1:] != jpeg.OK).all()


@pytest.mark.parametrize("sampling,tables", MUTATION_FILES)
def test_flipped_bytes_have_the_sequential_decoders_status(sampling, tables):
    """Inverted bytes in the entropy data: ones that make a marker (the planner must send those to the host) and an even spread
    (many of which are valid streams of another picture: those must decode to the same coefficients on both sides)."""
    from tstar_amd import jpeg
    data = JU.encode(JU.noise_picture(97, 301, seed=4), sampling, 75, tables)
    geom = jpeg.probe(data)[1]
    _, start = JU.segments(data)
    end = len(data) - 2
    sure = [p for p in range(start, end - 64)
            if data[p] == 0x00 and not (data[p + 1] in (0x00, 0xFF) or 0xD0 <= data[p + 1] <= 0xD9)][:40]
    spread = list(range(start, end, max(1, (end - start) // 200)))
    datas = []
    for p in sure + spread:
        m = bytearray(data)
        m[p] ^= 0xFF
        datas.append(bytes(m))
    routed = check_streams(datas, geom)
    plan = jpeg.plan_segments(datas[:len(sure)], geom)
    assert (plan.route == jpeg.ROUTE_HOST).all(), "a marker in the middle of a scan is not the framing the kernel may see"
    print(f"{sampling}/{tables}: {routed} of {len(datas)} flipped streams keep their framing and are decoded segment by segment")


def test_frames_the_decoder_does_not_vouch_for_keep_their_status():
    """Stray bytes in front of EOI, a missing EOI, a block beyond the energy bound, fill bytes in front of markers, a restart
    marker out of order, one too many and one too few."""
    from tstar_amd import jpeg
    pic = JU.noise_picture(40, 50, seed=9)
    good = JU.encode(pic, "420", 75)
    rst = JU.encode(pic, "420", 75, "restart")
    geom = jpeg.probe(good)[1]
    stray = good[:-2] + b"\x12\x34\x56" + good[-2:]
    segs, _ = JU.segments(good)
    a = next(a for m, a, _ in segs if m == 0xDB)
    loud = bytearray(good)
    for k in range(64):
        loud[a + 5 + k] = min(255, 8 * loud[a + 5 + k])
    _, start = JU.segments(rst)
    marks = [p for p in range(start, len(rst) - 2) if rst[p] == 0xFF and 0xD0 <= rst[p + 1] <= 0xD7]
    assert len(marks) >= 3
    filled = rst[:marks[1]] + b"\xff\xff" + rst[marks[1]:-2] + b"\xff" + rst[-2:]            # fill bytes are allowed
    swapped = bytearray(rst)
    swapped[marks[0] + 1], swapped[marks[1] + 1] = swapped[marks[1] + 1], swapped[marks[0] + 1]
    extra = rst[:-2] + b"\xff\xd7" + rst[-2:]
    fewer = rst[:marks[-1]] + rst[-2:]
    datas = [good, stray, bytes(loud), good[:-2], good[:-1], rst, filled, bytes(swapped), extra, fewer,
             JU.encode(pic, "444", 75), JU.encode(pic, "420", 75, progressive=True), b"", b"\xff\xd8"]
    check_streams(datas, geom)
    want = host_decode(datas, geom)[2]
    assert list(want[:7]) == [jpeg.OK, jpeg.UNCOVERED, jpeg.UNCOVERED, jpeg.UNCOVERED, jpeg.UNCOVERED, jpeg.OK, jpeg.OK]
    plan, _, seg_status = segments_decode(datas, geom)
    # stray bytes and the loud block are seen by the decode core itself (device route); broken framing never reaches it
    assert list(plan.route) == [0, 0, 0, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    assert list(plan.frame_status(seg_status)[:3]) == [jpeg.OK, jpeg.UNCOVERED, jpeg.UNCOVERED]


def test_a_segment_record_that_points_outside_the_batch_touches_nothing():
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    data = JU.encode(JU.noise_picture(33, 17, seed=1), "420", 75, "restart")
    geom = jpeg.probe(data)[1]
    plan = jpeg.plan_segments([data, data], geom)
    blocks = jpeg._sizes(geom)[0]
    buf = np.frombuffer(data + data, dtype=np.uint8)
    nseg = len(plan.segments)
    assert nseg >= 4
    bad = plan.segments.copy()
    bad["frame"][0] = 2                          # no such frame
    bad["end"][1] = len(buf) + 1                 # past the bytes
    bad["n_mcu"][2] = 1 << 30                    # more MCUs than a frame has
    bad["begin"][3] = bad["end"][3] + 1          # begin behind end
    frames = plan.frames.copy()
    frames["table_set"][1] = 7                   # no such table set: every segment of frame 1
    guard = 1024
    coef = np.full(2 * blocks * 64 + 2 * guard, 0x5A5A, dtype=np.int16)
    status = np.full(nseg, -1, dtype=np.int32)
    rc = lib.tstar_jpeg_entropy_segments_host(buf.ctypes.data, len(buf), bad.ctypes.data, plan.table_sets.ctypes.data, len(plan.table_sets),
                                              frames.ctypes.data, 2, nseg, *geom, coef[guard:].ctypes.data, status.ctypes.data)
    assert rc == 0
    assert list(status[:4]) == [jpeg.MALFORMED] * 4
    assert (status[plan.segments["frame"] == 1] == jpeg.MALFORMED).all()
    assert (coef[:guard] == 0x5A5A).all() and (coef[-guard:] == 0x5A5A).all()
    assert not coef[guard + blocks * 64:-guard].any(), "frame 1 was written although none of its segments is usable"
    # arguments are refused outright
    assert lib.tstar_jpeg_entropy_segments_host(None, len(buf), bad.ctypes.data, plan.table_sets.ctypes.data, 1, frames.ctypes.data, 2, nseg,
                                                *geom, coef.ctypes.data, status.ctypes.data) == 1
    assert lib.tstar_jpeg_entropy_segments_host(buf.ctypes.data, len(buf), bad.ctypes.data, plan.table_sets.ctypes.data, 1, frames.ctypes.data, 2,
                                                nseg, 50, 40, 3, 3, 1, coef.ctypes.data, status.ctypes.data) == 1


def test_plan_reports_the_sizes_it_needs():
    from tstar_amd import _lib, jpeg
    import ctypes as C
    lib = _lib.load()
    pic = JU.noise_picture(33, 17, seed=1)
    datas = [JU.encode(pic, "420", 75, "restart"), JU.encode(pic, "420", 75, "optimize")]
    geom = jpeg.probe(datas[0])[1]
    full = jpeg.plan_segments(datas, geom)
    assert len(full.table_sets) == 2 and len(full.segments) == 3
    small = jpeg.plan_segments(datas, geom, cap_sets=1, cap_segments=1)         # grows and calls again
    assert np.array_equal(small.segments, full.segments) and np.array_equal(small.table_sets, full.table_sets)
    ptrs = (C.c_char_p * 2)(*datas)
    lens = (C.c_size_t * 2)(*[len(d) for d in datas])
    offsets = np.array([0, len(datas[0])], dtype=np.uint64)
    route, frames, quant = np.empty(2, np.int32), np.empty(2, jpeg.FRAME_DTYPE), np.empty((2, 192), np.uint16)
    out5 = (C.c_size_t * 5)()
    rc = lib.tstar_jpeg_plan_segments(ptrs, lens, offsets.ctypes.data, 2, *geom, route.ctypes.data, frames.ctypes.data, quant.ctypes.data,
                                      None, 0, None, 0, out5)
    assert rc == 4 and list(out5) == [2, 3, jpeg.TABLE_SET_BYTES, jpeg.SEGMENT_DTYPE.itemsize, jpeg.FRAME_DTYPE.itemsize]
    offsets[1] = (1 << 32) - 10                                                   # beyond a segment's 32-bit offsets
    sets, segs = np.empty((2, jpeg.TABLE_SET_BYTES), np.uint8), np.empty(3, jpeg.SEGMENT_DTYPE)
    rc = lib.tstar_jpeg_plan_segments(ptrs, lens, offsets.ctypes.data, 2, *geom, route.ctypes.data, frames.ctypes.data, quant.ctypes.data,
                                      sets.ctypes.data, 2, segs.ctypes.data, 3, out5)
    assert rc == 1 and b"32-bit" in lib.tstar_last_error()


def test_chunk_policy():
    """Frames per chunk of the device path: as many as 512 MiB of device coefficients hold, at most 1024 and at most the frames
    there are; an explicit chunk wins over the budget."""
    from tstar_amd.jpeg import device_entropy_chunk as chunk
    b360, b1080 = 5520, 48960                      # blocks of a 360x640 / 1080x1920 4:2:0 frame (padded to whole MCUs)
    table = [
        ((b360, 3600), {}, 759),                   # (512 << 20) // (5520 * 128)
        ((b1080, 600), {}, 85),
        ((b360, 100), {}, 100),                    # not more than there are
        ((6, 100000), {}, 1024),                   # tiny frames: the frame cap
        ((1 << 24, 10), {}, 1),                    # one frame above the budget still goes
        ((b360, 3600), {"chunk": 64}, 64),
        ((b360, 10), {"chunk": 64}, 10),
        ((b360, 3600), {"coef_budget": 64 << 20}, 94),
        ((b360, 3600), {"max_frames": 256}, 256),
    ]
    for args, kw, want in table:
        assert chunk(*args, **kw) == want, (args, kw)
    for bad in ((0, 10), (10, 0)):
        with pytest.raises(ValueError):
            chunk(*bad)
    # and by compressed bytes: whole files go up, and a segment addresses the upload with 32 bits
    from tstar_amd.jpeg import device_entropy_take as take
    for lens, kw, want in (([10, 20, 30], {}, 3), ([], {}, 1), ([600 << 20, 400 << 20, 100 << 20], {}, 2), ([2 << 30, 5], {}, 1),
                           ([4, 4, 4, 4], {"byte_budget": 8}, 2), ([4, 4, 4, 4], {"byte_budget": 7}, 1), ([9, 1], {"byte_budget": 8}, 1)):
        assert take(lens, **kw) == want, (lens, kw)


def test_a_restart_coded_batch_is_planned_in_one_call(monkeypatch):
    """The default segment capacity comes from the first frame, so a chunk of restart-coded frames is not walked twice."""
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    datas = [JU.encode(JU.noise_picture(97, 301, seed=i), "420", 75, "restart") for i in range(4)]
    geom = jpeg.probe(datas[0])[1]
    calls = []
    real = lib.tstar_jpeg_plan_segments

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def tstar_jpeg_plan_segments(self, *a):
            rc = real(*a)
            calls.append((a[3], rc))
            return rc

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    plan = jpeg.plan_segments(datas, geom)
    assert len(plan.segments) == 4 * 45
    assert calls == [(1, 0), (4, 0)], calls                                       # the first frame alone, then the batch once


def test_entropy_mode_keyword_and_environment(monkeypatch):
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    monkeypatch.delenv("TSTAR_JPEG_ENTROPY", raising=False)
    assert jpeg.entropy_mode() == "host" and jpeg.entropy_mode("device") == "device"
    monkeypatch.setenv("TSTAR_JPEG_ENTROPY", "device")
    assert jpeg.entropy_mode() == "device" and jpeg.entropy_mode("host") == "host"
    with pytest.raises(ValueError, match="entropy mode"):
        jpeg.entropy_mode("gpu")
    datas = [JU.encode(JU.synthetic_picture(40, 50, frame=i), "420") for i in range(3)]
    with pytest.raises(ValueError, match="entropy='device' needs a GPU store"):
        open_video(datas, device="cpu", jpeg_entropy="device")                  # only the explicit keyword is an error
    for kw in ({}, {"jpeg_entropy": "host"}):                                   # the variable leaves a CPU store on the host path
        st = open_video(datas, device="cpu", **kw)
        assert st.decode_stats == {"device": 0, "host": 3, "pillow": 0} and st.entropy_stats == {"device": 0, "host": 3}


def test_segment_core_under_address_and_ub_sanitizers(tmp_path):
    """Planner + decode core built with -fsanitize=address,undefined (a stand-alone CPU program; nothing is loaded into python,
    nothing of the GPU is involved) and driven by csrc/jpeg_segments_check_main.cpp over intact, truncated, flipped,
    header-mutated, stray-byte and EOI-less streams on exact-size heap copies.  An out-of-bounds access or undefined operation
    aborts the tool; it also compares every stream with the sequential decoder."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_segments_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_host.cpp"), os.path.join(csrc, "jpeg_segments_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    pics = {"s": JU.synthetic_picture(40, 50), "n": JU.noise_picture(33, 17, seed=2)}
    for kind, pic in pics.items():
        for sampling, tables in MUTATION_FILES:
            p = tmp_path / f"{kind}_{sampling}_{tables}.jpg"
            p.write_bytes(JU.encode(pic, sampling, 75, tables))
            files.append(str(p))
    for name, data in (("nodht", JU.strip_dht(JU.encode(pics["n"], "420", 75))),
                       ("long_codes", JU.encode(JU.noise_picture(97, 301, seed=3), "420", 100, "optimize")),
                       ("wrap", JU.encode(JU.noise_picture(97, 301, seed=3), "420", 75, "restart"))):
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(data)
        files.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files) and all(" intact=0 " in ln and ln.endswith(" differ=0") for ln in lines), r.stdout
