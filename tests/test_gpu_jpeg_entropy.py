"""GPU: the JPEG entropy stage on the device -- tstar_jpeg_entropy_device == the sequential host decoder bit for bit
(coefficients, quantisation rows, statuses), the store == Pillow (libjpeg-turbo) byte for byte, wave edges, mixed table
sets, the error paths, and open_video with jpeg_entropy="device"."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (17, 33), (97, 301), (360, 640)]
QUALITIES = [30, 100]
GUARD = 4096
COEF_SENTINEL, STATUS_SENTINEL, RGB_SENTINEL = 0x7FC0, 0x7FC00000, 0xA5        # NaN-like patterns no decoder writes by itself


def _need_turbo():
    if not JU.turbo():
        pytest.skip("Pillow on this machine is not built on libjpeg-turbo: its bytes are not the yardstick the byte-equality "
                    "is defined against (the comparison is not loosened instead)")


def host_decode(datas, geom):
    from tstar_amd import jpeg
    blocks = jpeg._sizes(geom)[0]
    coef = np.zeros((len(datas), blocks * 64), dtype=np.int16)
    quant = np.zeros((len(datas), 192), dtype=np.uint16)
    status, _ = jpeg.entropy_batch(datas, geom, coef, quant)
    return coef, quant, status


def device_decode(datas, geom, reconstruct=False):
    """One upload, one launch; every output has a sentinel tail that must come back untouched.
    -> (plan, coef int16 [n, blocks * 64], seg_status, rgb uint8 [n, H, W, 3] or None)."""
    import torch
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    batch = jpeg.DeviceBatch(datas, geom)
    n, nseg = len(datas), len(batch.plan.segments)
    assert nseg > 0
    blocks, plane_bytes = jpeg._sizes(geom)
    host = np.zeros(batch.nbytes, dtype=np.uint8)
    batch.fill(host)
    d_buf = torch.from_numpy(host).cuda()
    d_coef = torch.full((n * blocks * 64 + GUARD,), COEF_SENTINEL, dtype=torch.int16, device="cuda")
    d_status = torch.full((nseg + GUARD,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    batch.launch(d_buf, d_coef, d_status, geom, _lib.stream_ptr())
    rgb = None
    if reconstruct:
        W, H = geom[0], geom[1]
        d_planes = torch.empty(n * plane_bytes, dtype=torch.uint8, device="cuda")
        d_rgb = torch.full((n * H * W * 3 + GUARD,), RGB_SENTINEL, dtype=torch.uint8, device="cuda")
        _lib.check(lib.tstar_jpeg_reconstruct(d_coef.data_ptr(), d_buf.data_ptr() + batch.parts["quant"][0], n, *geom, d_planes.data_ptr(),
                                              d_rgb.data_ptr(), _lib.stream_ptr()), "tstar_jpeg_reconstruct")
        out = d_rgb.cpu().numpy()
        assert (out[-GUARD:] == RGB_SENTINEL).all()
        rgb = out[:-GUARD].reshape(n, H, W, 3)
    torch.cuda.synchronize()
    coef, status = d_coef.cpu().numpy(), d_status.cpu().numpy()
    assert (coef[-GUARD:] == COEF_SENTINEL).all(), "the kernel wrote behind the coefficient buffer"
    assert (status[-GUARD:] == STATUS_SENTINEL).all(), "the kernel wrote behind the status array"
    assert np.array_equal(d_buf.cpu().numpy(), host), "the kernel wrote into its input"
    return batch.plan, coef[:-GUARD].reshape(n, blocks * 64), status[:nseg], rgb


def _long_code_lengths(data):
    """Code lengths above 9 bits that the file's Huffman tables define (with optimised tables every defined code is used)."""
    out = 0
    for m, a, b in JU.segments(data)[0]:
        if m == 0xC4:
            q = a + 4
            while q < b:
                counts = data[q + 1:q + 17]
                out += sum(counts[9:])
                q += 17 + sum(counts)
    return out


@pytest.fixture(scope="module")
def hard_stream():
    """Noise at quality 100 with optimised tables: codes longer than the 9-bit fast table and stuffed FF bytes."""
    data = JU.encode(JU.noise_picture(97, 301, seed=97 + 301 + 100), "420", 100, "optimize")
    _, start = JU.segments(data)
    assert _long_code_lengths(data) >= 1, "no code longer than 9 bits: the long-code path would go untested"
    assert b"\xff\x00" in data[start:], "no FF00: the unstuffing would go untested"
    return data


@pytest.fixture(scope="module")
def wrap_stream():
    """97x301 4:2:0 with a restart interval of 3 MCUs: 19 x 7 = 133 MCUs -> 45 segments (RSTn wraps five times), the last of
    one MCU."""
    from tstar_amd import jpeg
    data = JU.encode(JU.noise_picture(97, 301, seed=5), "420", 75, "restart")
    plan = jpeg.plan_segments([data], jpeg.probe(data)[1])
    assert len(plan.segments) > 8 and plan.segments["n_mcu"][-1] < plan.segments["n_mcu"][0]
    return data


def test_long_codes_stuffing_and_marker_wrap(hard_stream, wrap_stream):
    from tstar_amd import jpeg
    _need_turbo()
    datas = [hard_stream, wrap_stream]
    geom = jpeg.probe(datas[0])[1]
    want_c, want_q, want_s = host_decode(datas, geom)
    assert not want_s.any()
    plan, coef, seg_status, rgb = device_decode(datas, geom, reconstruct=True)
    assert not seg_status.any() and np.array_equal(coef, want_c) and np.array_equal(plan.quant, want_q)
    for i, d in enumerate(datas):
        assert np.array_equal(rgb[i], JU.pillow_rgb(d))


@pytest.mark.parametrize("sampling", JU.SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_entropy_equals_host_and_pillow(size, sampling):
    """{synthetic, noise} x {default, optimised, restart tables} x qualities {30, 100} of one geometry in one launch: several
    table sets per workgroup at the small sizes, hundreds of restart segments at the large ones."""
    from tstar_amd import jpeg
    _need_turbo()
    H, W = size
    datas = [d for q in QUALITIES for _, d in JU.matrix_files(H, W, sampling, q)]
    geom = jpeg.probe(datas[0])[1]
    want_c, want_q, want_s = host_decode(datas, geom)
    assert not want_s.any()
    plan, coef, seg_status, rgb = device_decode(datas, geom, reconstruct=True)
    assert (plan.route == jpeg.ROUTE_DEVICE).all() and len(plan.table_sets) >= 4
    assert not seg_status.any()
    assert np.array_equal(plan.quant, want_q)
    bad = np.nonzero((coef != want_c).any(axis=1))[0]
    assert len(bad) == 0, f"frames {bad.tolist()} differ from the host decoder's coefficients"
    for i, d in enumerate(datas):
        assert np.array_equal(rgb[i], JU.pillow_rgb(d)), f"frame {i} differs from Pillow"


@pytest.fixture(scope="module")
def one_segment_frames():
    """130 frames of one segment each (17x33 4:2:0, default tables: one table set, so the workgroups stage it in LDS) and what
    the host decodes from them."""
    from tstar_amd import jpeg
    datas = [JU.encode(JU.noise_picture(17, 33, seed=i), "420", 75) for i in range(130)]
    geom = jpeg.probe(datas[0])[1]
    return datas, geom, host_decode(datas, geom)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_segment_counts_around_wave_edges(one_segment_frames, n):
    datas, geom, (want_c, want_q, want_s) = one_segment_frames
    plan, coef, seg_status, _ = device_decode(datas[:n], geom)
    assert len(plan.segments) == n and len(plan.table_sets) == 1
    assert not seg_status.any() and np.array_equal(coef, want_c[:n]) and np.array_equal(plan.quant, want_q[:n])


def test_mixed_table_sets_in_one_workgroup():
    """Default, optimised and restart frames interleaved, fewer than 64 segments: one workgroup whose lanes name different table
    sets (tables from global memory), against a batch of the restart frame alone (one set: tables from LDS)."""
    from tstar_amd import jpeg
    pics = [JU.noise_picture(17, 33, seed=40 + i) for i in range(9)]
    datas = [JU.encode(p, "420", 90, ("default", "optimize", "restart")[i % 3]) for i, p in enumerate(pics)]
    geom = jpeg.probe(datas[0])[1]
    want_c, want_q, _ = host_decode(datas, geom)
    plan, coef, seg_status, _ = device_decode(datas, geom)
    assert len(plan.table_sets) >= 3 and len(plan.segments) < 64 and len(set(plan.frames["table_set"][:3])) > 1
    assert not seg_status.any() and np.array_equal(coef, want_c) and np.array_equal(plan.quant, want_q)
    plan, coef, seg_status, _ = device_decode([datas[2]], geom)
    assert len(plan.table_sets) == 1 and len(plan.segments) == 2
    assert not seg_status.any() and np.array_equal(coef[0], want_c[2])


def test_error_paths_equal_the_decode_core_on_the_host():
    """Truncated, flipped, stray-byte and loud streams.  Each batch first runs through the same decode core on the CPU
    (entropy_segments_host); the device must then return the same status for every segment, and the same coefficients for
    every frame whose segments are all OK.  Streams whose framing is broken never reach either: the planner routes them away."""
    from tstar_amd import jpeg
    data = JU.encode(JU.noise_picture(97, 301, seed=3), "420", 75, "restart")
    plain = JU.encode(JU.noise_picture(97, 301, seed=3), "420", 75)
    geom = jpeg.probe(data)[1]
    _, start = JU.segments(data)
    datas = [data, plain, plain[:-2] + b"\x12\x34\x56" + plain[-2:]]
    segs, _ = JU.segments(plain)
    a = next(a for m, a, _ in segs if m == 0xDB)
    loud = bytearray(plain)
    for k in range(64):
        loud[a + 5 + k] = min(255, 8 * loud[a + 5 + k])
    datas.append(bytes(loud))
    datas += [data[:n] for n in range(0, len(data), 97)]
    for src in (data, plain):
        s0 = JU.segments(src)[1]
        for p in range(s0, len(src) - 2, max(1, (len(src) - 2 - s0) // 60)):
            m = bytearray(src)
            m[p] ^= 0xFF
            datas.append(bytes(m))
    plan = jpeg.plan_segments(datas, geom)
    buf = np.frombuffer(b"".join(datas), dtype=np.uint8)
    core_coef, core_status = jpeg.entropy_segments_host(buf, plan, geom)
    core_frames = plan.frame_status(core_status)
    want_s = host_decode(datas, geom)[2]
    routed = plan.route == jpeg.ROUTE_DEVICE
    assert np.array_equal(core_frames[routed], want_s[routed])                   # the core ran clean on these bytes, and agrees
    assert {jpeg.OK, jpeg.MALFORMED, jpeg.UNCOVERED} <= set(core_frames[routed].tolist())
    plan_d, coef, seg_status, _ = device_decode(datas, geom)
    assert np.array_equal(plan_d.segments, plan.segments)
    assert np.array_equal(seg_status, core_status)
    ok = core_frames == jpeg.OK
    assert ok.sum() >= 3 and np.array_equal(coef[ok], core_coef[ok])


def test_launcher_refuses_bad_arguments():
    import torch
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    data = JU.encode(JU.noise_picture(17, 33, seed=1), "420", 75)
    geom = jpeg.probe(data)[1]
    batch = jpeg.DeviceBatch([data], geom)
    host = np.zeros(batch.nbytes, dtype=np.uint8)
    batch.fill(host)
    d_buf = torch.from_numpy(host).cuda()
    blocks = jpeg._sizes(geom)[0]
    d_coef = torch.full((blocks * 64,), COEF_SENTINEL, dtype=torch.int16, device="cuda")
    d_status = torch.full((1,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    base, parts, s = d_buf.data_ptr(), batch.parts, _lib.stream_ptr()
    good = [base, batch.total, base + parts["segments"][0], base + parts["table_sets"][0], 1, base + parts["frames"][0], 1, 1, *geom,
            d_coef.data_ptr(), d_status.data_ptr(), s]
    for at, value in ((0, None), (2, None), (3, None), (5, None), (13, None), (14, None), (4, 0), (6, 0), (7, 0), (1, 0), (1, 1 << 32),
                      (8, 0), (11, 3), (2, base + parts["segments"][0] + 1)):
        args = list(good)
        args[at] = value
        assert lib.tstar_jpeg_entropy_device(*args) == 1, (at, value)
    torch.cuda.synchronize()
    assert (d_coef.cpu().numpy() == COEF_SENTINEL).all() and int(d_status.cpu()[0]) == STATUS_SENTINEL      # nothing was launched
    assert lib.tstar_jpeg_entropy_device(*good) == 0
    torch.cuda.synchronize()
    assert int(d_status.cpu()[0]) == jpeg.OK


# ------------------------------------------------------------------------------------------------ open_video
@pytest.fixture(scope="module")
def clip():
    from tstar_amd.video import synthetic_frames_numpy
    frames = synthetic_frames_numpy(range(95), 95, 72, 128, seed=7)
    # every fourth frame default tables, the others restart-coded: the frames a 25 / 30 fps container hands out (0, 25, 50 /
    # 0, 30, 60) then hold both kinds
    return [JU.encode(f, "420", 85, "restart" if i % 4 else "default") for i, f in enumerate(frames)]


@pytest.mark.parametrize("container", ["folder", "mjpeg", "avi"])
def test_open_video_device_entropy_equals_host_mode(tmp_path, clip, container, monkeypatch):
    import torch
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    _need_turbo()
    monkeypatch.delenv("TSTAR_JPEG_ENTROPY", raising=False)
    wanted = {"folder": range(12), "mjpeg": (0, 25, 50), "avi": (0, 30, 60)}[container]
    geom = jpeg.probe(clip[0])[1]
    counts = {len(jpeg.plan_segments([clip[i]], geom).segments) for i in wanted}
    assert 1 in counts and max(counts) > 1, "the container's frames must hold single- and multi-segment frames"
    if container == "folder":
        path = tmp_path / "frames"
        path.mkdir()
        for i, d in enumerate(clip[:12]):
            (path / f"f{i}.jpg").write_bytes(d)
        n = 12
    elif container == "mjpeg":
        path = tmp_path / "clip.mjpeg"
        JU.write_mjpeg(str(path), clip, pad=3)
        n = 3
    else:
        path = tmp_path / "clip.avi"
        JU.write_avi(str(path), clip, 128, 72, rate=30)
        n = 3
    host = open_video(str(path))
    dev = open_video(str(path), jpeg_entropy="device")
    assert host.decode_stats == dev.decode_stats == {"device": n, "host": 0, "pillow": 0}
    assert host.entropy_stats == {"device": 0, "host": n} and dev.entropy_stats == {"device": n, "host": 0}
    assert torch.equal(host.frames, dev.frames)
    assert (dev.raw_fps, dev.raw_total_frames, dev.num_seconds) == (host.raw_fps, host.raw_total_frames, host.num_seconds)


@pytest.mark.parametrize("chunk", [None, 4])
def test_planted_frames_are_counted_and_exact(clip, chunk, monkeypatch):
    """A progressive frame (routed to the host by the planner) and a stray-byte frame (refused by the kernel) among good ones:
    both go through the host decoder, which hands them to Pillow; the counts say so and every byte is Pillow's."""
    from tstar_amd import jpeg
    from tstar_amd.video import synthetic_frames_numpy
    _need_turbo()
    monkeypatch.delenv("TSTAR_JPEG_ENTROPY", raising=False)
    datas = list(clip[:10])
    datas[3] = JU.encode(synthetic_frames_numpy([3], 95, 72, 128, seed=7)[0], "420", 85, progressive=True)
    datas[6] = datas[6][:-2] + b"\x12\x34\x56" + datas[6][-2:]
    ref = np.stack([JU.pillow_rgb(d) for d in datas])
    st = jpeg.load_jpeg(jpeg.JpegList(datas), device="cuda", chunk=chunk, entropy="device")
    assert st.decode_stats == {"device": 8, "host": 0, "pillow": 2}
    assert st.entropy_stats == {"device": 8, "host": 2}
    assert np.array_equal(st.frames.cpu().numpy(), ref)
    # the default mode: what it always was, plus the new attribute
    st = jpeg.load_jpeg(jpeg.JpegList(datas), device="cuda", chunk=chunk)
    assert st.decode_stats == {"device": 8, "host": 0, "pillow": 2} and list(st.decode_stats) == ["device", "host", "pillow"]
    assert st.entropy_stats == {"device": 0, "host": 10}
    assert np.array_equal(st.frames.cpu().numpy(), ref)
    # a broken frame is the same error in both modes
    datas[8] = datas[8][:len(datas[8]) // 2]
    for mode in ("host", "device"):
        with pytest.raises(ValueError, match=r"Cannot open video file: <jpeg list>\[8\] \("):
            jpeg.load_jpeg(jpeg.JpegList(datas), device="cuda", chunk=chunk, entropy=mode)


def test_environment_selects_the_device_mode(clip, monkeypatch):
    from tstar_amd.video import open_video
    monkeypatch.setenv("TSTAR_JPEG_ENTROPY", "device")
    st = open_video(clip[:5])
    assert st.entropy_stats == {"device": 5, "host": 0}
    st = open_video(clip[:5], jpeg_entropy="host")
    assert st.entropy_stats == {"device": 0, "host": 5}
