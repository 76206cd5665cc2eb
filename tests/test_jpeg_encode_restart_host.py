"""Restart intervals in the JPEG encoder's host twin (csrc/jpeg_enc_host.cpp) against Pillow, byte for byte; no GPU needed.

``restart_rows=`` / ``restart_blocks=`` must give the bytes of ``Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=s,
restart_marker_rows=r, restart_marker_blocks=b)``.  tests/test_gpu_jpeg_encode_restart.py pins the kernels against the twin on
the same matrix.
"""
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from jpeg_encode_util import new_counters, pillow_bytes, sos_end
from jpeg_restart_util import (GEOMETRIES, INTERVALS, KINDS, QUALITIES, interval_of, markers_of, mcus, new_restart_counters,
                               pillow_restart_bytes, rst_picture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}")
def test_whole_files_equal_pillow(geom):
    from tstar_amd import jpeg_encode as JE
    H, W, s = geom
    mx, my = mcus(H, W, s)
    for kind in KINDS:
        a = rst_picture(kind, H, W, s)
        for q in QUALITIES:
            plain = pillow_bytes(a, q, s)
            for kw in INTERVALS:
                want = pillow_restart_bytes(a, q, s, **kw)
                c = new_restart_counters()
                out, lengths, status = JE.encode_host(a, q, s, restart_counters=c, **kw)
                assert status[0] == 0 and out[0, :lengths[0]].tobytes() == want, (geom, kind, q, kw)
                assert JE.encode_frames(a, q, s, device=False, **kw) == [want]
                # what the file must hold whatever the picture
                R = interval_of(H, W, s, **kw)
                n = (mx * my - 1) // R
                marks = markers_of(want[sos_end(want):])
                assert marks == [0xD0 + (i & 7) for i in range(n)] and int(c[0]) == n, (geom, kw)
                assert int(c[1]) + int(c[2]) <= n
                if n == 0:                            # DRI and no marker: the marker-free scan behind six bytes more of header
                    assert want[629:] == plain[623:]


def test_rows_win_and_zero_means_none():
    from tstar_amd import jpeg_encode as JE
    H, W, s = GEOMETRIES[0]
    a = rst_picture("noise", H, W, s)
    both = JE.encode_frames(a, 75, s, device=False, restart_rows=2, restart_blocks=3)
    assert both == JE.encode_frames(a, 75, s, device=False, restart_rows=2) == JE.encode_frames(a, 75, s, device=False, restart_blocks=10)
    assert JE.encode_frames(a, 75, s, device=False, restart_rows=0, restart_blocks=4) == JE.encode_frames(a, 75, s, device=False, restart_blocks=4)
    assert JE.encode_frames(a, 75, s, device=False, restart_rows=0, restart_blocks=4) == [pillow_restart_bytes(a, 75, s, 0, 4)]
    plain = [pillow_bytes(a, 75, s)]
    assert JE.encode_frames(a, 75, s, device=False, restart_rows=0, restart_blocks=0) == plain
    assert JE.encode_frames(a, 75, s, device=False, restart_rows=None, restart_blocks=None) == plain
    assert JE.restart_interval(W, H, s, 2, 3) == 10 and JE.restart_interval(W, H, s, None, 3) == 3 and JE.restart_interval(W, H, s) == 0


def test_interval_zero_through_the_new_entries_is_the_existing_entries():
    """tstar_jpeg_encode_*_rst with interval 0 == the entries without an interval: files, scans, lengths, header, plan, counters.
    jpeg_encode reaches the _rst entries alone, so the entries without an interval are called here as the ABI has them."""
    import ctypes as C
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    lib = _lib.load()
    for H, W, s in GEOMETRIES:
        hs, vs = JE.sampling(s)
        batch = np.stack([rst_picture("noise", H, W, s), rst_picture("smooth", H, W, s)])
        idx = np.arange(2, dtype=np.int32)
        for q in (30, 100):
            c_old, c_new, r_new = new_counters(), new_counters(), new_restart_counters()
            p = JE.Plan(W, H, hs, vs, 2)
            slot = p.header_bytes + p.max_scan_bytes
            old = (np.empty((2, slot), dtype=np.uint8), np.zeros(2, dtype=np.uint32), np.full(2, -1, dtype=np.int32))
            _lib.check(lib.tstar_jpeg_encode_host(batch.ctypes.data, 2, H, W, idx.ctypes.data, 2, q, hs, vs, old[0].ctypes.data, slot,
                                                  old[1].ctypes.data, old[2].ctypes.data, 0, c_old.ctypes.data))
            new = JE.encode_host(batch, q, s, counters=c_new, restart_counters=r_new)          # goes through tstar_jpeg_encode_host_rst
            assert np.array_equal(old[1], new[1]) and np.array_equal(old[2], new[2]) and np.array_equal(c_old, c_new)
            assert all(old[0][i, :old[1][i]].tobytes() == new[0][i, :new[1][i]].tobytes() == pillow_bytes(batch[i], q, s) for i in range(2))
            assert r_new.tolist() == [0, 0, 0]
            coef, _ = JE.blocks_host(batch, q, s)
            r2 = new_restart_counters()
            a_out, a_len, a_st = np.empty((2, p.max_scan_bytes), dtype=np.uint8), np.zeros(2, dtype=np.uint32), np.full(2, -1, dtype=np.int32)
            _lib.check(lib.tstar_jpeg_encode_scan_host(coef.ctypes.data, 2, W, H, hs, vs, a_out.ctypes.data, p.max_scan_bytes, a_len.ctypes.data,
                                                       a_st.ctypes.data, 0, None))
            a = ([a_out[i, :a_len[i]].tobytes() if a_st[i] == 0 else None for i in range(2)], a_len, a_st)
            b = JE.scan_host(coef, W, H, s, restart_counters=r2)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and r2.tolist() == [0, 0, 0]
            buf, plain = np.zeros(1024, dtype=np.uint8), np.zeros(1024, dtype=np.uint8)
            n, n_plain = C.c_size_t(0), C.c_size_t(0)
            _lib.check(lib.tstar_jpeg_encode_header_rst(W, H, q, hs, vs, 0, buf.ctypes.data, buf.size, C.byref(n)))
            _lib.check(lib.tstar_jpeg_encode_header(W, H, q, hs, vs, plain.ctypes.data, plain.size, C.byref(n_plain)))
            assert buf[:n.value].tobytes() == plain[:n_plain.value].tobytes() == JE.header(W, H, q, s) and n.value == n_plain.value == 623
        out8, new8, out2 = (C.c_size_t * 8)(), (C.c_size_t * 8)(), (C.c_size_t * 2)()
        _lib.check(lib.tstar_jpeg_encode_plan(W, H, hs, vs, 3, 4096, out8))
        _lib.check(lib.tstar_jpeg_encode_plan_rst(W, H, hs, vs, 3, 4096, 0, new8, out2))
        assert list(out8) == list(new8) and list(out2) == [0, 0]


def test_the_corpus_reaches_every_path():
    """Conditions on the inputs of the tests here and on the GPU, from the twin's counters: over the corpus a marker is written, an
    interval ends byte-aligned (no padding), a padded byte comes out as 0xFF, and data bytes are stuffed."""
    from tstar_amd import jpeg_encode as JE
    total = dict(rst=0, pad_free=0, pad_ff=0, stuffed=0)
    for H, W, s in GEOMETRIES:
        for kind in KINDS:
            for q in QUALITIES:
                for kw in INTERVALS:
                    c, r = new_counters(), new_restart_counters()
                    JE.encode_host(rst_picture(kind, H, W, s), q, s, counters=c, restart_counters=r, **kw)
                    for k, v in zip(JE.RESTART_COUNTERS, r):
                        total[k] += int(v)
                    total["stuffed"] += int(c[JE.COUNTERS.index("stuffed")])
    print(total)
    assert all(v > 0 for v in total.values()), total
    assert total["pad_free"] + total["pad_ff"] < total["rst"]


def test_header_carries_dri_directly_before_sos():
    from tstar_amd import jpeg_encode as JE
    for H, W, s in GEOMETRIES + [(360, 640, "4:2:0")]:
        hs, vs = JE.sampling(s)
        a = rst_picture("smooth", H, W, s) if H < 100 else np.zeros((H, W, 3), dtype=np.uint8)
        plain = JE.header(W, H, 75, s)
        assert plain == pillow_bytes(a, 75, s)[:623] and b"\xff\xdd" not in plain
        assert JE.header(W, H, 75, s, restart_rows=0, restart_blocks=0) == plain
        for kw in INTERVALS + [dict(restart_blocks=65535), dict(restart_blocks=258)]:
            ref = pillow_restart_bytes(a, 75, s, **kw)
            head = JE.header(W, H, 75, s, **kw)
            R = interval_of(H, W, s, **kw)
            assert head == ref[:sos_end(ref)] and len(head) == 629, (H, W, s, kw)
            assert head[:609] == plain[:609] and head[609:615] == b"\xff\xdd\x00\x04" + struct.pack(">H", R) and head[615:] == plain[609:]
            assert JE.Plan(W, H, hs, vs, restart=R).header_bytes == 629


def test_plan_bounds_hold_the_markers_and_the_padding():
    """max_scan_bytes grows by 4 bytes per marker: the padding in front of a marker adds less than one data byte, which stuffing
    can double; the marker's two bytes are never stuffed.  The workspace grows by the interval tables."""
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    base = JE.Plan(640, 360, 2, 2, 4, 4096)
    for R, markers in ((1, 919), (8, 114), (40, 22), (919, 1), (920, 0), (65535, 0)):
        p = JE.Plan(640, 360, 2, 2, 4, 4096, restart=R)
        assert p.markers == markers == (40 * 23 - 1) // R and p.restart == R
        assert p.max_scan_bytes == base.max_scan_bytes + 4 * markers and p.header_bytes == 629
        assert p.blocks == base.blocks and p.entropy_wgs_x == base.entropy_wgs_x and p.block_wgs == base.block_wgs
        assert base.workspace_bytes + 4 * 4 * (2 * markers + 1) <= p.workspace_bytes <= base.workspace_bytes + 4 * 4 * (2 * markers + 1) + 64
    # the bound is reached from below by the worst the tables allow; a real worst case stays inside it
    H, W, s = GEOMETRIES[2]
    a = rst_picture("noise", H, W, s)
    out, lengths, status = JE.encode_host(a, 100, s, restart_blocks=1)
    assert status[0] == 0 and lengths[0] - 629 <= JE.Plan(W, H, 1, 1, restart=1).max_scan_bytes
    for R in (-1, 65536, 1 << 20):
        with pytest.raises(_lib.TStarHipError, match="65535"):
            JE.Plan(640, 360, 2, 2, 1, 4096, restart=R)


def test_invalid_values_raise_before_anything_is_touched():
    from tstar_amd import jpeg_encode as JE
    a = rst_picture("smooth", 45, 77, "4:2:0")

    class NoStore:                                     # a store whose frames must never be asked for
        fmt, shape = "rgb", (4, 45, 77, 3)

        def __getattr__(self, name):
            raise AssertionError(f"store.{name} touched")

    for kw in (dict(restart_blocks=-1), dict(restart_rows=-1), dict(restart_blocks=2.5), dict(restart_rows=1.0), dict(restart_blocks="4"),
               dict(restart_blocks=True), dict(restart_blocks=65536), dict(restart_rows=13108), dict(restart_rows=-1, restart_blocks=4)):
        for call in (lambda: JE.encode_frames(a, device=False, **kw), lambda: JE.encode_host(a, **kw), lambda: JE.header(77, 45, **kw),
                     lambda: JE.scan_host(np.zeros((1, 15 * 6 * 64), np.int16), 77, 45, **kw), lambda: JE.frames_to_base64(a[None], **kw),
                     lambda: JE.save_mjpeg(a[None], "/nonexistent/never_opened.avi", device=False, **kw),
                     lambda: JE.encode_frames((NoStore(), [0]), **kw), lambda: JE.save_mjpeg(NoStore(), "/nonexistent/never_opened.avi", **kw)):
            with pytest.raises(ValueError, match="restart"):
                call()
    with pytest.raises(ValueError, match="65535"):
        JE.restart_interval(77, 45, "4:2:0", restart_blocks=65536)
    assert JE.restart_interval(77, 45, "4:2:0", restart_blocks=65535) == 65535 and JE.restart_interval(77, 45, "4:2:0", restart_rows=13107) == 65535
    assert JE.restart_interval(77, 45, "4:2:0", restart_blocks=np.int64(4)) == 4


def test_short_slots_report_short_and_write_nothing():
    """Under-sized slots, whole files and scans alone: STATUS_SHORT, the length the frame would take, and not a byte written into
    the slot or behind it (sentinels)."""
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    lib = _lib.load()
    for (H, W, s), q, kw in ((GEOMETRIES[0], 100, dict(restart_blocks=1)), (GEOMETRIES[1], 75, dict(restart_rows=1)),
                             (GEOMETRIES[4], 30, dict(restart_blocks=4)), (GEOMETRIES[3], 75, dict(restart_blocks=1))):
        hs, vs = JE.sampling(s)
        a = rst_picture("noise", H, W, s)
        ref = pillow_restart_bytes(a, q, s, **kw)
        L, pad = len(ref), 64
        for cap, want in ((L, JE.STATUS_OK), (L - 1, JE.STATUS_SHORT), (629, JE.STATUS_SHORT), (0, JE.STATUS_SHORT)):
            buf = np.full(L + pad, 0xA5, dtype=np.uint8)
            out, lengths, status = JE.encode_host(a, q, s, slot_bytes=cap, out=buf, **kw)
            assert status[0] == want and lengths[0] == L, (H, W, s, cap)
            assert buf[:L].tobytes() == ref and (buf[L:] == 0xA5).all() if want == JE.STATUS_OK else (buf == 0xA5).all()
        # the scan stage alone: two frames in slots back to back, then slots one byte, a marker, half a scan short
        coef, _ = JE.blocks_host(np.stack([a, a]), q, s)
        R = interval_of(H, W, s, **kw)
        need = L - 629
        for slot in (need, need - 1, need - 2, need // 2, 2):
            buf = np.full(2 * slot + pad, 0xA5, dtype=np.uint8)
            lengths, status = np.zeros(2, np.uint32), np.full(2, -1, np.int32)
            _lib.check(lib.tstar_jpeg_encode_scan_host_rst(coef.ctypes.data, 2, W, H, hs, vs, R, buf.ctypes.data, slot, lengths.ctypes.data,
                                                           status.ctypes.data, 2, None, None))
            assert lengths.tolist() == [need, need]
            if slot == need:
                assert status.tolist() == [0, 0] and buf[:need].tobytes() == buf[need:2 * need].tobytes() == ref[629:]
                assert (buf[2 * need:] == 0xA5).all()
            else:
                assert status.tolist() == [1, 1] and (buf == 0xA5).all(), slot


def test_pillow_reads_the_files_as_it_reads_the_marker_free_ones():
    """Restart markers change the entropy coding, not the coefficients: Pillow decodes every file of the matrix to the pixels of
    the file without markers; and the scan stage fed what the project's decoder reads out of Pillow's file gives Pillow's scan."""
    from PIL import Image
    from tstar_amd import jpeg
    from tstar_amd import jpeg_encode as JE
    for H, W, s in GEOMETRIES:
        hs, vs = JE.sampling(s)
        for kind in KINDS:
            a = rst_picture(kind, H, W, s)
            plain = np.asarray(Image.open(io.BytesIO(pillow_bytes(a, 75, s))))
            coef, _ = JE.blocks_host(a, 75, s)
            for kw in INTERVALS:
                data = JE.encode_frames(a, 75, s, device=False, **kw)[0]
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), plain), (H, W, s, kind, kw)
                if W // hs > 2:                       # the project's decoder leaves narrower chroma planes to Pillow
                    dcoef = np.zeros((1, coef.shape[1]), dtype=np.int16)
                    dquant = np.zeros((1, 192), dtype=np.uint16)
                    status, msg = jpeg.entropy_batch([data], (W, H, 3, hs, vs), dcoef, dquant)
                    assert status[0] == 0, msg
                    assert np.array_equal(dcoef, coef)
                    scans, _, st = JE.scan_host(dcoef, W, H, s, **kw)
                    assert st[0] == 0 and scans[0] == data[629:]


def test_container_files_carry_the_markers(tmp_path):
    from tstar_amd import jpeg
    from tstar_amd import jpeg_encode as JE
    H, W, s = GEOMETRIES[0]
    frames = np.stack([rst_picture("smooth", H, W, s), rst_picture("noise", H, W, s)])
    want = [pillow_restart_bytes(a, 90, s, restart_blocks=4) for a in frames]
    path = str(tmp_path / "r.avi")
    assert JE.save_mjpeg(frames, path, quality=90, device=False, restart_blocks=4) == 2
    src = jpeg.avi_mjpeg(path)
    try:
        assert [bytes(src.read(i)) for i in range(2)] == want
    finally:
        src.close()
    path = str(tmp_path / "plain.avi")                 # the default stays: no markers
    JE.save_mjpeg(frames, path, quality=90, device=False)
    src = jpeg.avi_mjpeg(path)
    try:
        assert [bytes(src.read(i)) for i in range(2)] == [pillow_bytes(a, 90, s) for a in frames]
    finally:
        src.close()
    import base64
    assert JE.frames_to_base64(frames, quality=90, restart_rows=1) == [base64.b64encode(pillow_restart_bytes(a, 90, s, restart_rows=1)).decode()
                                                                       for a in frames]


def test_host_twin_with_intervals_under_address_and_ub_sanitizers(tmp_path):
    """The twin built with -fsanitize=address,undefined (CPU build; nothing of the GPU is involved) and driven by
    csrc/jpeg_enc_rst_check_main.cpp over tiny geometries, intervals from one MCU to beyond the frame and under-sized slots.  Any
    out-of-bounds access or undefined operation aborts the tool."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_enc_rst_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_enc_host.cpp"), os.path.join(csrc, "jpeg_host.cpp"), os.path.join(csrc, "jpeg_enc_rst_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler lacks the sanitizer runtime: " + r.stderr.strip().splitlines()[-1][:200])
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 8 * 8 and all(" ok=1 " in ln for ln in lines), r.stdout
    assert any(" rst=0 " not in ln for ln in lines)


def test_surface():
    import inspect
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    from tstar_amd.video import FrameStore
    new = {"tstar_jpeg_encode_plan_rst", "tstar_jpeg_encode_header_rst", "tstar_jpeg_encode_scan_rst", "tstar_jpeg_encode_rst",
           "tstar_jpeg_encode_scan_host_rst", "tstar_jpeg_encode_host_rst"}
    with open(os.path.join(ROOT, "include", "tstar_hip.h")) as f:
        declared = set(re.findall(r"\b(tstar_[a-z0-9_]+)\s*\(", f.read()))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new) and lib.tstar_abi_version() == 3
    for fn in (JE.header, JE.scan_host, JE.encode_host, JE.encode_frames, JE.frames_to_base64, JE.save_mjpeg, FrameStore.jpeg_frames,
               FrameStore.save_mjpeg):
        params = inspect.signature(fn).parameters
        assert params["restart_rows"].default is None and params["restart_blocks"].default is None, fn
    # what existing callers read stays what it was
    assert JE.Plan.FIELDS == ("blocks", "coef_bytes", "max_scan_bytes", "header_bytes", "workspace_bytes", "block_wgs", "entropy_wgs_x",
                              "stuff_wgs_x")
    assert JE.COUNTERS == ("zrl", "no_eob", "stuffed", "dummy_right", "dummy_bottom") and JE.RESTART_COUNTERS == ("rst", "pad_free", "pad_ff")
