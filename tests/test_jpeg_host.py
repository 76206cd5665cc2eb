"""CPU: the JPEG decode front end without a GPU -- host entropy stage + scalar reference of the kernels against Pillow
(libjpeg-turbo) BYTE FOR BYTE, the container readers, and malformed input."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, SAMPLINGS, QUALITIES = JU.SIZES, JU.SAMPLINGS, JU.QUALITIES


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_path_equals_pillow(size, sampling, quality):
    """Equality of bytes with np.asarray(Image.open(f).convert("RGB")): both sides run the same integer algorithm.  The
    files with default tables are decoded a second time with their DHT segments removed (Annex K tables implied)."""
    from tstar_amd import jpeg
    assert JU.turbo(), "Pillow here is not built on libjpeg-turbo: the byte-equality yardstick does not apply"
    H, W = size
    files = JU.matrix_files(H, W, sampling, quality)
    stripped = [(lab + "/no-DHT", JU.strip_dht(d)) for lab, d in files if not lab.endswith("optimize")]
    got = jpeg.decode_host([d for _, d in files + stripped])
    refs = [JU.pillow_rgb(d) for _, d in files]
    refs += [r for (lab, _), r in zip(files, refs) if not lab.endswith("optimize")]
    for (lab, _), g, r in zip(files + stripped, got, refs):
        assert r.shape == (H, W, 3)
        diff = np.nonzero(g != r)
        assert len(diff[0]) == 0, f"{lab}: {len(diff[0])} bytes differ, first at {[int(a[0]) for a in diff]}"


def test_probe_reports_geometry_and_coverage():
    from tstar_amd import jpeg
    pic = JU.synthetic_picture(40, 50)
    for sampling, want in (("420", (50, 40, 3, 2, 2)), ("422", (50, 40, 3, 2, 1)), ("444", (50, 40, 3, 1, 1)), ("gray", (50, 40, 1, 1, 1))):
        rc, info, _ = jpeg.probe(JU.encode(pic, sampling))
        assert rc == jpeg.OK and info == want
    rc, info, msg = jpeg.probe(JU.encode(pic, "420", progressive=True))
    assert rc == jpeg.UNCOVERED and info[:2] == (50, 40) and "progressive" in msg
    from PIL import Image
    import io
    b = io.BytesIO()
    Image.fromarray(pic).convert("CMYK").save(b, "JPEG")
    assert jpeg.probe(b.getvalue())[0] == jpeg.UNCOVERED


# ------------------------------------------------------------------------------------------------ containers
def _video_frames(n, H=72, W=128):
    from tstar_amd.video import synthetic_frames_numpy
    return synthetic_frames_numpy(range(n), n, H, W, seed=7)


@pytest.fixture(scope="module")
def clip():
    """95 frames of 72x128 synthetic video at 30 fps (3 logical seconds: raw frames 0, 30, 60), their JPEGs and what Pillow
    decodes from them."""
    frames = _video_frames(95)
    jpegs = [JU.encode(f, "420", 85) for f in frames]
    return jpegs, np.stack([JU.pillow_rgb(d) for d in jpegs])


@pytest.mark.parametrize("kw", [dict(index=True), dict(index=False), dict(index=True, absolute_index=True),
                                dict(index=True, audio=True), dict(index=False, audio=True)],
                         ids=["idx1", "no-idx1", "idx1-absolute", "audio-first-idx1", "audio-first-walk"])
def test_avi_reader(tmp_path, clip, kw):
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    jpegs, ref = clip
    path = str(tmp_path / "clip.avi")
    JU.write_avi(path, jpegs, 128, 72, rate=30, **kw)
    src = jpeg.avi_mjpeg(path)
    try:
        assert src.n_frames == 95 and src.fps == 30.0
        assert jpeg.wanted_frames(src.n_frames, src.fps) == [0, 30, 60]
        assert [src.read(i) for i in (0, 1, 94)] == [jpegs[0], jpegs[1], jpegs[94]]
    finally:
        src.close()
    st = open_video(path, device="cpu")
    assert st.raw_fps == 30.0 and st.raw_total_frames == 95 and st.num_seconds == 3
    assert st.decode_stats == {"device": 0, "host": 3, "pillow": 0}
    assert np.array_equal(st.frames.numpy(), ref[[0, 30, 60]])


def test_avi_rate_from_scale_and_dropped_frame(tmp_path, clip):
    from tstar_amd import jpeg
    jpegs, _ = clip
    path = str(tmp_path / "ntsc.avi")
    JU.write_avi(path, [jpegs[0], b"", jpegs[2]], 128, 72, rate=30000, scale=1001)
    src = jpeg.avi_mjpeg(path)
    try:
        assert abs(src.fps - 30000 / 1001) < 1e-12 and src.n_frames == 3
        assert src.read(1) == jpegs[0]                 # a zero-length chunk repeats the previous picture
    finally:
        src.close()


def test_avi_other_codec_and_opendml_are_refused_by_name(tmp_path, clip):
    from tstar_amd.video import open_video
    jpegs, _ = clip
    path = str(tmp_path / "x.avi")
    JU.write_avi(path, jpegs[:2], 128, 72, fourcc=b"XVID")
    with pytest.raises(ValueError, match=r"Cannot open video file: .*XVID"):
        open_video(path, device="cpu")
    JU.write_avi(path, jpegs[:40], 128, 72, avix=True)
    with pytest.raises(ValueError, match=r"Cannot open video file: .*AVIX"):
        open_video(path, device="cpu")
    with open(path, "wb") as f:
        f.write(b"RIFF\x04\x00\x00\x00WAVE")
    with pytest.raises(ValueError, match="Cannot open video file"):
        open_video(path, device="cpu")


def test_mjpeg_stream(tmp_path, clip):
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    jpegs, ref = clip
    # a frame with a thumbnail-like JPEG inside an APP1 segment: an FFD8 / FFD9 search would split it in two
    inner = JU.encode(JU.synthetic_picture(8, 8), "444", 50)
    app1 = b"\xff\xe1" + struct.pack(">H", 2 + len(inner)) + inner
    with_thumb = jpegs[0][:2] + app1 + jpegs[0][2:]
    path = str(tmp_path / "clip.mjpeg")
    JU.write_mjpeg(path, [with_thumb] + jpegs[1:60], pad=3)
    src = jpeg.mjpeg_stream(path, 25.0)
    try:
        assert src.n_frames == 60 and src.fps == 25.0 and src.read(0) == with_thumb and src.read(59) == jpegs[59]
    finally:
        src.close()
    st = open_video(path, device="cpu")                                    # default 25 fps: seconds 0, 1 -> frames 0, 25
    assert (st.raw_fps, st.raw_total_frames, st.num_seconds) == (25.0, 60, 2)
    assert np.array_equal(st.frames.numpy(), ref[[0, 25]])
    st = open_video(path, device="cpu", fps=10)
    assert st.num_seconds == 6 and np.array_equal(st.frames.numpy(), ref[[0, 10, 20, 30, 40, 50]])
    with open(path, "ab") as f:
        f.write(jpegs[0][:len(jpegs[0]) // 2])                             # a torn last frame
    with pytest.raises(ValueError, match="frame 60 .*broken or truncated"):
        open_video(path, device="cpu")


def test_folder_natural_order_and_list_of_bytes(tmp_path, clip):
    from tstar_amd.video import load_video_frames, open_video
    jpegs, ref = clip
    d = tmp_path / "frames"
    d.mkdir()
    order = {"f2.jpg": 0, "f10.jpg": 1, "f1.JPEG": 2, "f100.jpg": 3}       # natural order: f1, f2, f10, f100
    for name, i in order.items():
        (d / name).write_bytes(jpegs[i])
    (d / "notes.txt").write_text("not a frame")
    st = open_video(str(d), device="cpu")
    assert (st.raw_fps, st.raw_total_frames, st.num_seconds) == (1.0, 4, 4)
    assert np.array_equal(st.frames.numpy(), ref[[2, 0, 1, 3]])
    st = open_video(str(d), device="cpu", fps=2.0)                         # two files per logical second
    assert st.num_seconds == 2 and np.array_equal(st.frames.numpy(), ref[[2, 1]])
    st = open_video(jpegs[:5], device="cpu")
    assert st.num_seconds == 5 and np.array_equal(st.frames.numpy(), ref[:5])
    st = open_video([str(d / "f10.jpg"), jpegs[7]], device="cpu")
    assert np.array_equal(st.frames.numpy(), ref[[1, 7]])
    with pytest.raises(ValueError, match="holds no .jpg"):
        empty = tmp_path / "empty"
        empty.mkdir()
        open_video(str(empty), device="cpu")
    with pytest.raises(ValueError, match="fps= applies"):
        open_video("synthetic://n=4", fps=2.0)


def test_fallback_frames_are_counted_and_exact(tmp_path):
    """Frames the device path does not cover (progressive here) go through Pillow, and so does a covered frame whose sampling
    differs from the batch's; both are counted, and every frame must have the first one's size."""
    from tstar_amd.video import open_video
    pics = [JU.synthetic_picture(40, 50, frame=i) for i in range(4)]
    datas = [JU.encode(pics[0], "420"), JU.encode(pics[1], "420", progressive=True), JU.encode(pics[2], "444"),
             JU.encode(pics[3], "420", tables="optimize")]
    ref = np.stack([JU.pillow_rgb(d) for d in datas])
    st = open_video(datas, device="cpu")
    assert st.decode_stats == {"device": 0, "host": 2, "pillow": 2}
    assert np.array_equal(st.frames.numpy(), ref)
    st = open_video([datas[1], datas[1], datas[0]], device="cpu")          # the stream may open with uncovered frames
    assert st.decode_stats == {"device": 0, "host": 1, "pillow": 2}
    assert np.array_equal(st.frames.numpy(), ref[[1, 1, 0]])
    other = JU.encode(JU.synthetic_picture(48, 50), "420")
    with pytest.raises(ValueError, match=r"\[2\] is 50x48, the first frame is 50x40"):
        open_video([datas[0], datas[3], other], device="cpu")


def _rgb_coded(pic, ids=(1, 2, 3)):
    """A JPEG whose three components ARE R, G, B (Pillow keep_rgb: no JFIF marker, Adobe marker with transform 0), with the
    component ids rewritten so that nothing but the markers says so."""
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(pic).save(b, "JPEG", quality=90, keep_rgb=True)
    d = bytearray(b.getvalue())
    for m, a, _ in JU.segments(bytes(d))[0]:
        if m == 0xC0:
            for c in range(3):
                d[a + 4 + 6 + 3 * c] = ids[c]
        elif m == 0xDA:
            for c in range(3):
                d[a + 4 + 1 + 2 * c] = ids[c]
    return bytes(d)


def _swap_app0(data, replacement):
    """data with its JFIF APP0 segment replaced by `replacement` (bytes of whole segments, may be empty)."""
    for m, a, b in JU.segments(data)[0]:
        if m == 0xE0:
            return data[:a] + replacement + data[b:]
    raise AssertionError("no APP0")


def test_colour_space_follows_the_markers_as_libjpeg_reads_them():
    """libjpeg takes three components as YCbCr when a JFIF marker is present; else as RGB when an Adobe marker says transform
    0, whatever the component ids; else by the ids.  RGB-coded frames are not ours: Pillow decodes them, and they are counted."""
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    pic = JU.synthetic_picture(16, 16)
    for ids in ((1, 2, 3), (ord("R"), ord("G"), ord("B")), (0, 1, 2)):
        d = _rgb_coded(pic, ids)
        rc, info, msg = jpeg.probe(d)
        assert rc == jpeg.UNCOVERED and "RGB" in msg, ids
        st = open_video([d, d], device="cpu")
        assert st.decode_stats == {"device": 0, "host": 0, "pillow": 2}
        assert np.array_equal(st.frames.numpy()[1], JU.pillow_rgb(d))
    ycc = JU.encode(pic, "420", 90)
    adobe = lambda t: b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t])
    for name, d, covered in (("no JFIF, no Adobe, ids 1 2 3", _swap_app0(ycc, b""), True),
                             ("no JFIF, Adobe transform 1", _swap_app0(ycc, adobe(1)), True),
                             ("no JFIF, Adobe transform 0", _swap_app0(ycc, adobe(0)), False),
                             ("JFIF and Adobe transform 0", ycc[:2] + adobe(0) + ycc[2:], True)):
        rc = jpeg.probe(d)[0]
        assert rc == (jpeg.OK if covered else jpeg.UNCOVERED), name
        st = open_video([d], device="cpu")
        assert st.decode_stats["pillow"] == (0 if covered else 1), name
        assert np.array_equal(st.frames.numpy()[0], JU.pillow_rgb(d)), name


@pytest.mark.parametrize("size", [(4, 4), (9, 1), (3, 3), (5, 4), (8, 3), (16, 2), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pictures_too_narrow_for_the_triangle_filter_go_to_pillow(size):
    """Subsampled chroma at most two samples wide (W <= 4): libjpeg replicates instead of filtering, so such frames are not
    covered; full-resolution chroma and grayscale of the same size are."""
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    H, W = size
    pic = JU.noise_picture(H, W, seed=H * 31 + W)
    for sampling in JU.SAMPLINGS:
        d = JU.encode(pic, sampling, 90)
        covered = sampling in ("444", "gray")
        assert jpeg.probe(d)[0] == (jpeg.OK if covered else jpeg.UNCOVERED), sampling
        st = open_video([d], device="cpu")
        assert st.decode_stats == {"device": 0, "host": int(covered), "pillow": int(not covered)}, sampling
        assert np.array_equal(st.frames.numpy()[0], JU.pillow_rgb(d)), sampling


@pytest.mark.parametrize("size", [(3, 5), (9, 6), (1, 7), (2, 8), (16, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_narrowest_covered_pictures_equal_pillow(size):
    from tstar_amd import jpeg
    H, W = size
    pic = JU.noise_picture(H, W, seed=H * 17 + W)
    for sampling in JU.SAMPLINGS:
        d = JU.encode(pic, sampling, 90)
        assert np.array_equal(jpeg.decode_host([d])[0], JU.pillow_rgb(d)), sampling


def test_frames_the_decoder_does_not_vouch_for_are_pillows_call():
    """Stray bytes between the last block and EOI, or a block beyond the energy bound: not an error of the whole video but a
    frame for the general decoder -- what Pillow reads is stored and counted, what Pillow refuses is the error."""
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    pic = JU.noise_picture(40, 50, seed=9)
    good = JU.encode(pic, "420", 75)
    stray = good[:-2] + b"\x12\x34\x56" + good[-2:]
    # the same coefficients under a quantisation table eight times as coarse: every block far beyond what 8-bit samples give
    segs, _ = JU.segments(good)
    a = next(a for m, a, _ in segs if m == 0xDB)
    loud = bytearray(good)
    for k in range(64):
        loud[a + 5 + k] = min(255, 8 * loud[a + 5 + k])
    loud = bytes(loud)
    rc, geom, _ = jpeg.probe(good)
    blocks = jpeg._sizes(geom)[0]
    status, _ = jpeg.entropy_batch([good, stray, loud, good[:-2]], geom, np.empty((4, blocks * 64), np.int16), np.empty((4, 192), np.uint16))
    assert list(status) == [jpeg.OK, jpeg.UNCOVERED, jpeg.UNCOVERED, jpeg.UNCOVERED]
    st = open_video([good, stray, loud], device="cpu")
    assert st.decode_stats == {"device": 0, "host": 1, "pillow": 2}
    assert np.array_equal(st.frames.numpy(), np.stack([JU.pillow_rgb(d) for d in (good, stray, loud)]))
    with pytest.raises(ValueError, match=r"\[1\].*truncated"):          # no EOI: Pillow refuses it too
        open_video([good, good[:-2]], device="cpu")


# ------------------------------------------------------------------------------------------------ malformed input
def _rejected(data):
    from tstar_amd import jpeg
    try:
        jpeg.decode_host([bytes(data)])
    except ValueError:
        return True
    return False


@pytest.mark.parametrize("sampling,tables", [("420", "default"), ("422", "restart"), ("444", "optimize"), ("gray", "default")])
def test_truncated_at_every_97th_offset_is_an_error(sampling, tables):
    data = JU.encode(JU.noise_picture(97, 301, seed=3), sampling, 75, tables)
    assert not _rejected(data)
    offsets = list(range(0, len(data), 97))
    assert len(offsets) > 50
    for n in offsets:
        assert _rejected(data[:n]), f"the first {n} of {len(data)} bytes decoded"
    assert _rejected(data[:-1]) and _rejected(data[:-2])


@pytest.mark.parametrize("sampling,tables", [("420", "default"), ("422", "restart"), ("444", "optimize"), ("gray", "default")])
def test_flipped_bytes_in_the_entropy_data(sampling, tables):
    """Inverted bytes (b ^ 0xFF) in the entropy-coded segment.

    Which flips MUST be an error follows from the format, not from the decoder: a zero byte becomes FF, and FF followed by
    anything but 00 / FF / RSTn is a marker in the middle of a scan whose MCUs are not complete, so at least the eight bits
    that byte carried are missing.  Every such position of the file is tried and each is an error.

    An arbitrary flip cannot be required to fail: Huffman codes resynchronise, and a damaged stream is quite often a VALID
    stream of another picture (with the strict end-of-scan check and the block-energy bound here, 133 to 159 of about 200
    evenly spaced flips per file are rejected; the test prints the count).  For those the requirement is the one
    that can hold: never a crash, and either an error or exactly the bytes Pillow decodes from the same damaged file --
    nothing is decoded approximately."""
    from tstar_amd import jpeg
    data = JU.encode(JU.noise_picture(97, 301, seed=4), sampling, 75, tables)
    _, start = JU.segments(data)
    end = len(data) - 2
    sure = [p for p in range(start, end - 64)
            if data[p] == 0x00 and not (data[p + 1] in (0x00, 0xFF) or 0xD0 <= data[p + 1] <= 0xD7)]
    assert len(sure) >= 20
    for p in sure:
        m = bytearray(data)
        m[p] ^= 0xFF
        assert _rejected(m), f"marker made at offset {p} went unnoticed"
    rejected = 0
    spread = range(start, end, max(1, (end - start) // 200))
    for p in spread:
        m = bytearray(data)
        m[p] ^= 0xFF
        try:
            got = jpeg.decode_host([bytes(m)])[0]
        except ValueError:
            rejected += 1
            continue
        assert np.array_equal(got, JU.pillow_rgb(bytes(m))), f"flip at {p}: accepted, but not what Pillow reads from the same bytes"
    print(f"{sampling}/{tables}: {rejected} of {len(spread)} spread flips rejected, the rest decode as Pillow decodes them")


def _patched(data, marker, fn):
    """data with the payload of its first `marker` segment rewritten by fn(bytearray payload incl. length) -> bytes."""
    segs, _ = JU.segments(data)
    for m, a, b in segs:
        if m == marker:
            return data[:a + 2] + bytes(fn(bytearray(data[a + 2:b]))) + data[b:]
    raise AssertionError(hex(marker))


def _without(data, marker):
    for m, a, b in JU.segments(data)[0]:
        if m == marker:
            return data[:a] + data[b:]
    raise AssertionError(hex(marker))


def _set(offset, value):
    def fn(seg):
        seg[offset] = value
        return seg
    return fn


def test_bad_headers_are_errors():
    from tstar_amd import jpeg
    data = JU.encode(JU.synthetic_picture(40, 50), "420", 75)
    assert not _rejected(data)
    DQT, DHT, SOF, SOS = 0xDB, 0xC4, 0xC0, 0xDA
    cases = {
        "DQT length too long for its tables": _patched(data, DQT, lambda s: s[:2] + s[2:-1]),          # one byte short of 65
        "DQT length field below 2": _patched(data, DQT, _set(1, 1)),
        "DQT length past the end": _patched(data, DQT, lambda s: b"\xff\xff" + s[2:]),
        "DQT table index 4": _patched(data, DQT, _set(2, 0x04)),
        "DQT precision 2": _patched(data, DQT, _set(2, 0x20)),
        "DHT table index 4": _patched(data, DHT, _set(2, 0x04)),
        "DHT class 2": _patched(data, DHT, _set(2, 0x20)),
        "DHT more codes than symbols": _patched(data, DHT, _set(3 + 15, 200)),
        "DHT over-full code length": _patched(data, DHT, _set(3, 3)),                                   # three 1-bit codes
        "DHT length cut": _patched(data, DHT, lambda s: s[:2] + s[2:10]),
        "SOF length": _patched(data, SOF, _set(1, 12)),
        "SOF zero components": _patched(data, SOF, _set(7, 0)),
        "SOF five components": _patched(data, SOF, _set(7, 5)),
        "SOF zero width": _patched(data, SOF, lambda s: s[:5] + b"\x00\x00" + s[7:]),
        "SOF sampling factor 0": _patched(data, SOF, _set(9, 0x02)),
        "SOF quantisation table 3 (undefined)": _patched(data, SOF, _set(10, 3)),
        "SOF quantisation table index 9": _patched(data, SOF, _set(10, 9)),
        "SOF 12-bit samples": _patched(data, SOF, _set(2, 12)),
        "SOS names Huffman table 3 (undefined)": _patched(data, SOS, _set(4, 0x33)),
        "SOS component count": _patched(data, SOS, _set(2, 7)),
        "no SOI": b"\x00" + data[1:],
        "empty": b"",
        "SOI only": data[:2],
        "scan before frame header": _without(data, SOF),
        "no quantisation tables": _without(_without(data, DQT), DQT),
    }
    for why, bad in cases.items():
        assert bad != data, why
        assert _rejected(bad), why
    # a taller picture than the data holds: the scan ends early
    taller = _patched(data, SOF, lambda s: s[:3] + struct.pack(">H", 400) + s[5:])
    assert _rejected(taller)
    # 12-bit is reported as broken input by the probe too (no decoder on either side reads it)
    assert jpeg.probe(cases["SOF 12-bit samples"])[0] == jpeg.MALFORMED


def test_entropy_batch_reports_each_frame_and_keeps_to_its_buffers():
    from tstar_amd import jpeg
    pic = JU.noise_picture(33, 17, seed=1)
    good = JU.encode(pic, "420", 75)
    rc, geom, _ = jpeg.probe(good)
    assert rc == 0
    datas = [good, good[:len(good) // 2], JU.encode(pic, "444", 75), JU.encode(pic, "420", 75, progressive=True), good]
    blocks = 3 * 2 * 4 + 2 * 3 * 2                  # 17x33 at 2x2: 2 x 3 MCUs of 4 luma + 2 chroma blocks
    guard = 4096
    coef = np.full(len(datas) * blocks * 64 + guard, 0x5A5A, dtype=np.int16)
    quant = np.full(len(datas) * 192 + guard, 0xA5A5, dtype=np.uint16)
    status, msg = jpeg.entropy_batch(datas, geom, coef, quant, threads=3)
    assert list(status) == [jpeg.OK, jpeg.MALFORMED, jpeg.GEOMETRY, jpeg.UNCOVERED, jpeg.OK]
    assert "frame 1" in msg
    assert (coef[-guard:] == 0x5A5A).all() and (quant[-guard:] == 0xA5A5).all()
    per = blocks * 64
    assert np.array_equal(coef[:per], coef[4 * per:5 * per]) and np.array_equal(quant[:192], quant[4 * 192:5 * 192])


def test_thread_allowance_is_capped():
    from tstar_amd import _lib
    lib = _lib.load()
    allowed = len(os.sched_getaffinity(0))
    assert lib.tstar_jpeg_threads(0) == min(16, allowed)
    assert lib.tstar_jpeg_threads(1) == 1 and lib.tstar_jpeg_threads(1000) == min(16, allowed)


def test_host_stage_under_address_and_ub_sanitizers(tmp_path):
    """The host stage built once with -fsanitize=address,undefined (CPU build; nothing of the GPU is involved) and driven over
    intact, truncated (every 97th offset), flipped and header-mutated files by csrc/jpeg_check_main.cpp.  Any out-of-bounds
    access or undefined operation aborts the tool; it must also reject every truncated file."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_host.cpp"), os.path.join(csrc, "jpeg_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    pics = {"s": JU.synthetic_picture(40, 50), "n": JU.noise_picture(33, 17, seed=2)}
    for kind, pic in pics.items():
        for sampling, tables in (("420", "default"), ("422", "restart"), ("444", "optimize"), ("gray", "default")):
            p = tmp_path / f"{kind}_{sampling}_{tables}.jpg"
            p.write_bytes(JU.encode(pic, sampling, 75, tables))
            files.append(str(p))
    nodht = tmp_path / "nodht.jpg"
    nodht.write_bytes(JU.strip_dht(JU.encode(pics["n"], "420", 75)))
    files.append(str(nodht))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files) and all(" intact=0 truncated_decoded=0/" in ln for ln in lines), r.stdout
