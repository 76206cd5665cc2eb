"""CPU: lossless JPEG re-coding with a restart interval -- the host twin (jpeg_encode.recode_frames(device=False)) against Pillow as
the independent yardstick, the header from a file's own tables, the frames that are kept, the host mirror of the device assembly
against the planner, the containers, the refusals and the stand-alone sanitizer program.  Every comparison is an equality."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_recode_util as U  # noqa: E402
import jpeg_util as JU  # noqa: E402


def _recode(files, n, **kw):
    from tstar_amd import jpeg_encode as JE
    stats = {}
    out = JE.recode_frames(files, restart_blocks=n, device=False, stats=stats, **kw)
    return out, stats


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
@pytest.mark.parametrize("name", sorted(U.PILLOW_SOURCES))
def test_recoded_file_is_pillows_file_with_the_interval(case, name):
    """A source Pillow wrote at quality q (with default or optimised tables), re-coded at interval N, is byte for byte what Pillow
    writes for the same pixels with restart_marker_blocks=N."""
    W, H, s, n = case
    rgb, data = U.source(W, H, s, name)
    (out,), stats = _recode([data], n)
    assert out == U.pillow_with_interval(rgb, s, U.PILLOW_SOURCES[name], n)
    assert stats == {"recoded": 1, "bytes_in": len(data), "bytes_out": len(out)}


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
@pytest.mark.parametrize("name", U.SOURCES)
def test_recoding_changes_no_pixel_no_coefficient_no_table(case, name):
    """Pillow decodes the same pixels from both files; the project's host decoder returns identical coefficients and quant rows; the
    DQT payload is the source's; the file carries DRI = N and exactly the markers of that interval, in order."""
    W, H, s, n = case
    _, data = U.source(W, H, s, name)
    (out,), stats = _recode([data], n)
    assert stats.get("kept", 0) == 0 and stats["recoded"] == 1
    assert np.array_equal(JU.pillow_rgb(out), JU.pillow_rgb(data))
    g0, c0, q0 = U.host_coefficients(data)
    g1, c1, q1 = U.host_coefficients(out)
    assert g0 == g1 and np.array_equal(c0, c1) and np.array_equal(q0, q1)
    assert U.dqt_payloads(out) == U.dqt_payloads(data)
    segs, scan_at = JU.segments(out)
    dri = [out[a + 4:b] for m, a, b in segs if m == 0xDD]
    assert dri == [bytes([n >> 8, n & 255])]
    hs, vs = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}[s]
    mcus = (-(-W // (8 * hs))) * (-(-H // (8 * vs)))
    scan = out[scan_at:]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + k % 8 for k in range((mcus - 1) // n)]


@pytest.mark.parametrize("name", U.KEPT_SOURCES)
def test_frames_the_recoder_does_not_take_come_back_as_they_are(name):
    """Grayscale, progressive, and a crafted frame whose AC coefficient has size category 11: the source bytes, counted as kept."""
    _, data = U.source(48, 48, "420", name)
    (out,), stats = _recode([data], 1)
    assert out == data and stats == {"kept": 1, "bytes_in": len(data), "bytes_out": len(data)}


def test_a_coefficient_the_standard_tables_cannot_code_keeps_the_frame():
    """The decoder in front refuses category 11 itself, so the encoder-walk rule is driven directly: the coding half of the twin
    (jpeg_recode.code_host) on hand-made coefficients.  An AC value of 1024 (category 11) and a DC difference of 2048 (category 12)
    give None -- the frame is kept; 1023 and 2047 are coded, and the file with 1023 decodes back to the same coefficients (a DC of
    2047 at a table of ones is beyond the decoder's energy bound, so that file is only checked to be there)."""
    from tstar_amd import jpeg_recode as JR
    geom = (8, 8, 3, 1, 1)
    quant = np.ones(192, dtype=np.uint16)
    for at, bad, good in ((1, 1024, 1023), (1, -1024, -1023), (0, 2048, 2047), (64, -2048, -2047)):
        coef = np.zeros((1, 3 * 64), dtype=np.int16)
        coef[0, at] = bad
        assert JR.code_host(coef, quant, geom, 1) is None
        coef[0, at] = good
        out = JR.code_host(coef, quant, geom, 1)
        assert out is not None and out[:2] == b"\xff\xd8" and out[-2:] == b"\xff\xd9"
        if abs(good) == 1023:
            g, c, q = U.host_coefficients(out)
            assert g == geom and np.array_equal(c, coef[0]) and np.array_equal(q, quant)


def test_a_batch_of_files_of_several_geometries_and_kinds():
    files = U.batch(48, 48, "420") + U.batch(24, 40, "444") + [b"no jpeg at all"]
    out, stats = _recode(files, 2)
    kept = U.n_kept(files)
    assert kept == 7 and stats["kept"] == kept and stats["recoded"] == len(files) - kept
    assert stats["bytes_in"] == sum(map(len, files)) and stats["bytes_out"] == sum(map(len, out))
    for a, b in zip(files, out):
        assert (a == b) == (U.n_kept([a]) == 1)
    again, stats2 = _recode(out, 2)                                    # a file that has the interval already comes out as it is
    assert again == out and stats2["kept"] == kept


@pytest.mark.parametrize("restart", [0, 5])
@pytest.mark.parametrize("quality", [1, 30, 75, 100])
def test_header_from_a_quality_s_tables_is_the_quality_s_header(quality, restart):
    from tstar_amd import jpeg_encode as JE
    frame = JU.synthetic_picture(24, 40)
    _, quant = JE.blocks_host(frame[None], quality, "4:2:2")
    want = JE.header(40, 24, quality, "4:2:2", restart_blocks=restart)
    assert JE.header_from_tables(40, 24, quant, "4:2:2", restart) == want
    assert len(want) == 623 + (6 if restart else 0)


def test_header_with_wide_and_with_three_tables():
    """A value above 255: 16-bit entries (Pq = 1) and SOF1, as libjpeg writes it; different chroma rows: a third table for Cr.  The
    project's parser reads the rows back."""
    from tstar_amd import jpeg_encode as JE
    rs = np.random.RandomState(3)
    quant = rs.randint(1, 12, size=(3, 64))
    quant[1, 5] = 300
    quant[2, 63] = 65535
    head = JE.header_from_tables(16, 16, quant, "4:2:0", 4)
    segs, _ = JU.segments(head)
    dqt = [head[a + 4:b] for m, a, b in segs if m == 0xDB]
    assert [len(p) for p in dqt] == [65, 129, 129] and [p[0] for p in dqt] == [0x00, 0x11, 0x12]
    assert [m for m, _, _ in segs if 0xC0 <= m <= 0xC3] == [0xC1]
    coef = np.zeros((1, 6, 64), dtype=np.int16)
    coef[:, :, :6] = rs.randint(-3, 4, size=(1, 6, 6))               # few and small: inside the decoder's energy bound
    coef = coef.reshape(1, 6 * 64)
    scans, _, status = JE.scan_host(coef, 16, 16, "4:2:0", restart_blocks=4)
    assert status[0] == 0
    _, c, q = U.host_coefficients(head + scans[0])
    assert np.array_equal(q.reshape(3, 64), quant) and np.array_equal(c, coef[0])
    two = JE.header_from_tables(16, 16, quant[[0, 1, 1]], "4:2:0", 0)
    assert [m for m, _, _ in JU.segments(two)[0]].count(0xDB) == 2
    for bad in (np.zeros((3, 64)), np.full((3, 64), 65536), np.ones((2, 64))):
        with pytest.raises(ValueError):
            JE.header_from_tables(16, 16, bad, "4:2:0", 0)


@pytest.mark.parametrize("case", [U.CASES[2], U.CASES[4], U.CASES[6], U.CASES[7]], ids=[U.CASE_IDS[i] for i in (2, 4, 6, 7)])
def test_assembly_mirror_gives_the_twin_s_files_and_the_planner_s_records(case):
    """The host mirror of the device assembly over a batch of different lengths with kept frames in it: the output bytes are the
    twin's files end to end, and off / len / quant / frame records / segments / table sets are, field for field, what
    jpeg_plan_segments says about those bytes (through ArenaBuilder, as an open collects them)."""
    from tstar_amd import jpeg, jpeg_encode as JE, jpeg_recode as JR
    W, H, s, n = case
    files = U.batch(W, H, s)
    geom = JR.covered(files[0])
    batch = jpeg.DeviceBatch(files, geom)
    buf = np.zeros(batch.nbytes, dtype=np.uint8)
    batch.fill(buf)
    coef, seg_status = jpeg.entropy_segments_host(buf, batch.plan, geom)
    bad = batch.plan.frame_status(seg_status) != 0
    assert bad.sum() == 3
    one = JE.Plan(W, H, geom[3], geom[4], 1, restart=n)
    slot = (one.max_scan_bytes + 15) // 16 * 16
    scans, lengths, status = JE.scan_host(coef, W, H, JR._SUBSAMPLING[geom[3:]], slot_bytes=slot, restart_blocks=n)
    slots = np.full((len(files), slot), 0xA5, dtype=np.uint8)
    for i, sc in enumerate(scans):
        if sc is not None:
            slots[i, :len(sc)] = np.frombuffer(sc, dtype=np.uint8)
    want_files, _ = _recode(files, n)
    pieces = []
    for a, b in ((0, 5), (5, len(files))):                              # two pieces of one source batch
        kept = bad[a:b] | (status[a:b] == JE.STATUS_BAD_COEF)
        pd = JR.PieceDesc(batch.plan, [len(f) for f in files], a, b, kept, lengths[a:b], geom, n)
        out, rec = JR.assemble_host(pd, slots[a:b], lengths[a:b], buf, batch.plan)
        assert out.tobytes() == b"".join(want_files[a:b])
        pieces.append((pd.plan_of(rec), pd.out_len, want_files[a:b]))
    got = U.arena_of_plans([(p, lens) for p, lens, _ in pieces])
    want = U.arena_of_plans([(jpeg.plan_segments(fs, geom), [len(f) for f in fs]) for _, _, fs in pieces])
    U.assert_arenas_equal(got, want)
    new = got.frames["n_segments"][~bad]
    hs, vs = geom[3:]
    assert (new == -(-((-(-W // (8 * hs))) * (-(-H // (8 * vs)))) // n)).all()


def test_assembly_refuses_a_descriptor_that_does_not_tile():
    from tstar_amd import _lib, jpeg, jpeg_encode as JE, jpeg_recode as JR
    files = U.batch(24, 40, "444", with_kept=False)[:3]
    geom = JR.covered(files[0])
    batch = jpeg.DeviceBatch(files, geom)
    buf = np.zeros(batch.nbytes, dtype=np.uint8)
    batch.fill(buf)
    coef, _ = jpeg.entropy_segments_host(buf, batch.plan, geom)
    scans, lengths, _ = JE.scan_host(coef, 24, 40, "4:4:4", slot_bytes=8192, restart_blocks=2)
    slots = np.zeros((3, 8192), dtype=np.uint8)
    for i, sc in enumerate(scans):
        slots[i, :len(sc)] = np.frombuffer(sc, dtype=np.uint8)
    for field, value in (("first_segment", 1), ("n_segments", 3), ("hdr", 7), ("src", 3), ("kind", 2), ("table_set", -1)):
        pd = JR.PieceDesc(batch.plan, [len(f) for f in files], 0, 3, np.zeros(3, bool), lengths, geom, 2)
        pd.desc[field][1] = value
        with pytest.raises(_lib.TStarHipError):
            JR.assemble_host(pd, slots, lengths, buf, batch.plan)


def test_the_plain_assembly_entry_is_the_pitch_taking_one_at_1024():
    """tstar_jpeg_recode_assemble_host forwards to tstar_jpeg_recode_assemble_host_opt with rows of 1024 bytes: a one-frame piece
    through both, called directly, gives the same bytes and records; its own condition, an interval of at least 1, keeps its name."""
    from tstar_amd import _lib, jpeg, jpeg_encode as JE, jpeg_recode as JR
    files = [U.source(24, 40, "444", "q75")[1]]
    geom = JR.covered(files[0])
    batch = jpeg.DeviceBatch(files, geom)
    buf = np.zeros(batch.nbytes, dtype=np.uint8)
    batch.fill(buf)
    coef, _ = jpeg.entropy_segments_host(buf, batch.plan, geom)
    scans, lengths, _ = JE.scan_host(coef, 24, 40, "4:4:4", slot_bytes=8192, restart_blocks=2)
    slots = JR._aligned16(np.zeros((1, 8192), dtype=np.uint8))
    slots[0, :len(scans[0])] = np.frombuffer(scans[0], dtype=np.uint8)
    pd = JR.PieceDesc(batch.plan, [len(files[0])], 0, 1, np.zeros(1, bool), lengths, geom, 2)
    assert pd.pitch == JR.HEADER_PITCH == 1024
    nrec, _ = JR.recode_layout(1, pd.n_segments)
    headers, quant, plan = JR._aligned16(pd.headers), JR._aligned16(batch.plan.quant), batch.plan

    def call(entry, pitch, restart):
        rec, out = JR._aligned16(np.zeros(nrec, dtype=np.uint8)), np.zeros(max(16, pd.total), dtype=np.uint8)
        _lib.check(getattr(_lib.load(), entry)(
            pd.desc.ctypes.data, 1, pd.n_segments, headers.ctypes.data, *pitch, pd.header_len.ctypes.data, len(pd.header_len),
            slots.ctypes.data, slots.shape[1], lengths.ctypes.data, restart, pd.n_mcu, buf.ctypes.data, plan.total_bytes, quant.ctypes.data,
            plan.frames.ctypes.data, plan.segments.ctypes.data, len(plan.frames), len(plan.segments), rec.ctypes.data, rec.size,
            out.ctypes.data, pd.total), entry)
        return out.tobytes(), rec.tobytes()

    plain = call("tstar_jpeg_recode_assemble_host", (), 2)
    assert plain == call("tstar_jpeg_recode_assemble_host_opt", (1024,), 2)
    assert plain[0][:pd.total] == _recode(files, 2)[0][0]
    with pytest.raises(_lib.TStarHipError, match="tstar_jpeg_recode_assemble_host: restart interval outside 1..65535"):
        call("tstar_jpeg_recode_assemble_host", (), 0)


def test_recode_mjpeg_carries_every_frame_and_the_rate(tmp_path, monkeypatch):
    from tstar_amd import jpeg, jpeg_encode as JE
    files = [U.source(48, 48, "420", name, seed)[1] for seed in (0, 1) for name in ("q75", "noise100", "gray")]
    src = str(tmp_path / "src.avi")
    JU.write_avi(src, files, 48, 48, rate=30000, scale=1001)
    want, _ = _recode(files, 3)
    stats = {}
    for dst in ("out.avi", "out.mjpeg"):
        path = str(tmp_path / dst)
        assert JE.recode_mjpeg(src, path, restart_blocks=3, device=False, stats=stats) == len(files)
        back = jpeg.open_source(path)
        try:
            assert [back.read(i) for i in range(back.n_frames)] == want
            if dst.endswith(".avi"):
                assert back.fps == 30000 / 1001
        finally:
            back.close()
    assert stats["kept"] == 4 and stats["recoded"] == 8
    folder = tmp_path / "frames"
    folder.mkdir()
    for i, f in enumerate(files):
        (folder / f"f{i}.jpg").write_bytes(f)
    assert JE.recode_mjpeg(str(folder), str(tmp_path / "folder.mjpeg"), restart_blocks=3, device=False) == len(files)
    assert (tmp_path / "folder.mjpeg").read_bytes() == b"".join(want)
    monkeypatch.setattr(JE, "AVI_LIMIT", 4096)
    with pytest.raises(ValueError, match="1 GiB"):
        JE.recode_mjpeg(src, str(tmp_path / "big.avi"), restart_blocks=3, device=False)
    with pytest.raises(ValueError, match="expected .avi"):
        JE.recode_mjpeg(src, str(tmp_path / "out.mp4"), restart_blocks=3, device=False)
    with pytest.raises(ValueError, match="recode_mjpeg"):
        JE.recode_mjpeg(str(tmp_path / "nothing.bin"), str(tmp_path / "x.avi"), device=False)
    broken = tmp_path / "broken"
    broken.mkdir()
    (broken / "f0.jpg").write_bytes(b"\xff\xd8 not a picture")
    (broken / "f1.jpg").write_bytes(files[0])
    with pytest.raises(ValueError, match="recode_mjpeg.*f0.jpg"):      # the container's picture size comes from the first frame's header
        JE.recode_mjpeg(str(broken), str(tmp_path / "broken.avi"), device=False)
    assert not (tmp_path / "broken.avi").exists()


@pytest.mark.parametrize("n", [0, -1, 65536, 1.5, True, "8"])
def test_intervals_outside_what_dri_holds_are_refused(n):
    from tstar_amd import jpeg_encode as JE
    with pytest.raises(ValueError):
        JE.recode_frames([U.source(16, 16, "420", "q75")[1]], restart_blocks=n, device=False)


def test_recode_blocks_needs_the_resident_store(tmp_path, monkeypatch):
    from tstar_amd import jpeg_recode as JR
    from tstar_amd.video import open_video
    monkeypatch.delenv("TSTAR_JPEG_RESIDENT", raising=False)
    path = str(tmp_path / "clip.mjpeg")
    JU.write_mjpeg(path, [U.source(16, 16, "420", "q75")[1]] * 2)
    with pytest.raises(ValueError, match='resident="jpeg"'):
        open_video(path, device="cpu", fps=1.0, recode_blocks=8)
    with pytest.raises(ValueError, match="recode_blocks"):
        open_video("synthetic://n=4,h=16,w=16", device="cpu", resident="jpeg", recode_blocks=8)
    monkeypatch.setenv("TSTAR_JPEG_RECODE", "12")
    assert JR.recode_mode() == 12 and JR.recode_mode(3) == 3
    monkeypatch.setenv("TSTAR_JPEG_RECODE", "0")
    assert JR.recode_mode() == 0
    monkeypatch.setenv("TSTAR_JPEG_RECODE", "many")
    with pytest.raises(ValueError, match="TSTAR_JPEG_RECODE"):
        JR.recode_mode()
    # the variable alone leaves a store that is not compressed-resident as it is
    monkeypatch.setenv("TSTAR_JPEG_RECODE", "8")
    st = open_video(path, device="cpu", fps=1.0)
    assert st.num_seconds == 2 and not hasattr(st, "recode_stats")


def test_recode_sanitizer_program(tmp_path):
    """csrc/jpeg_recode_check_main.cpp with the assembly's mirror and the header writer, built with -fsanitize=address,undefined (a
    stand-alone CPU program; nothing is loaded into Python): pieces in exact-size heap blocks, kept and re-coded frames, refused
    descriptors, short capacities."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_recode_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_recode_host.cpp"), os.path.join(csrc, "jpeg_enc_host.cpp"), os.path.join(csrc, "jpeg_host.cpp"),
           os.path.join(csrc, "jpeg_recode_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the compiler lacks the sanitizer runtime: " + r.stderr.strip().splitlines()[-1][:200])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok" in run.stdout
