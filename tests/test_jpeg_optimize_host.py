"""Optimised Huffman tables in the JPEG encoder's host twin (csrc/jpeg_enc_host.cpp, csrc/jpeg_enc_math.h) against Pillow's
``optimize=True``, byte for byte; no GPU needed.

``optimize=True`` must give the bytes of ``Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=s, optimize=True,
restart_marker_rows=r, restart_marker_blocks=b)``.  The table procedure alone is compared with a Python restatement of libjpeg's
jpeg_gen_optimal_table (tests/jpeg_optimize_util.py), which in turn is held to Pillow's own tables.
tests/test_gpu_jpeg_optimize.py pins the kernels against the twin.
"""
import inspect
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from jpeg_encode_util import pillow_bytes, sos_end
from jpeg_optimize_util import (CLEN_OVERFLOW, GEOMETRIES, INTERVALS, KINDS, OK, QUALITIES, batch_of, canonical_codes, deep_table_picture,
                                fibonacci_counts, file_histograms, file_tables, flat_picture, optimal_table, pillow_optimize_bytes, rst_picture)
from jpeg_restart_util import interval_of, pillow_restart_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_table(got, want):
    return (list(got["bits"]), got["vals"], got["status"], got["steps"]) == tuple(want)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}")
def test_whole_files_equal_pillow(geom):
    from tstar_amd import jpeg_encode as JE
    H, W, s = geom
    for kind in KINDS:
        a = rst_picture(kind, H, W, s)
        for q in QUALITIES:
            for kw in INTERVALS:
                want = pillow_optimize_bytes(a, q, s, **kw)
                out, lengths, status = JE.encode_host(a, q, s, optimize=True, **kw)
                assert status[0] == 0 and out[0, :lengths[0]].tobytes() == want, (geom, kind, q, kw)
                assert JE.encode_frames(a, q, s, device=False, optimize=True, **kw) == [want]


def test_flat_pictures_batches_and_reordered_indices():
    from tstar_amd import jpeg_encode as JE
    for H, W, s in GEOMETRIES:
        flat = flat_picture(H, W)
        want = pillow_optimize_bytes(flat, 75, s)
        assert JE.encode_frames(flat, 75, s, device=False, optimize=True) == [want]
        tabs = file_tables(want)                       # four one-symbol tables: 20 bytes each, the symbol at length 1
        assert [t[0] for t in tabs] == [0x00, 0x10, 0x01, 0x11] and all(len(t[3]) == 22 and t[1] == [1] + [0] * 15 for t in tabs)
        pair = np.stack([rst_picture("noise", H, W, s), rst_picture("smooth", H, W, s)])
        for kw in (dict(), dict(restart_blocks=4)):
            assert JE.encode_frames(pair, 30, s, device=False, optimize=True, **kw) == [pillow_optimize_bytes(a, 30, s, **kw) for a in pair]
        store = np.concatenate([batch_of(H, W, s, 3), flat[None]])
        order = [3, 1, 0, 2, 1]
        out, lengths, status = JE.encode_host(store, 75, s, idx=order, optimize=True, threads=2)
        assert status.tolist() == [0] * 5
        assert [out[i, :lengths[i]].tobytes() for i in range(5)] == [pillow_optimize_bytes(store[k], 75, s) for k in order]


def test_the_restatement_gives_pillows_own_tables():
    """What the table function is compared with below is itself held to Pillow: the symbol counts decoded from Pillow's files give,
    through the restatement, the bits and huffval of every DHT segment of those files; and so does the table function."""
    from tstar_amd import jpeg_encode as JE
    n = 0
    for H, W, s in GEOMETRIES:
        hs, vs = JE.sampling(s)
        for kind in KINDS:
            a = rst_picture(kind, H, W, s)
            for q in (30, 100):
                for kw in (dict(), dict(restart_blocks=4)):
                    data = pillow_optimize_bytes(a, q, s, **kw)
                    hist = file_histograms(data, hs, vs, W, H)
                    tabs = file_tables(data)
                    assert [t[0] for t in tabs] == [0x00, 0x10, 0x01, 0x11]
                    for t in range(4):
                        want = optimal_table(hist[t])
                        assert (want[0], want[1], want[2]) == (tabs[t][1], tabs[t][2], OK), (H, W, s, kind, q, kw, t)
                        assert same_table(JE.huff_optimal(hist[t]), want)
                        n += 1
                    # and the twin's own counts are the file's
                    coef, _ = JE.blocks_host(a, q, s)
                    got = {}
                    JE.scan_host(coef, W, H, s, optimize=True, tables=got, **kw)
                    assert np.array_equal(got["hist"][0, :, :256], hist) and not got["hist"][0, :, 256].any()
    assert n == 5 * 2 * 2 * 2 * 4


def test_table_function_on_random_and_extreme_histograms():
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    rs = np.random.RandomState(7)
    cases = []
    for _ in range(60):
        cases.append(rs.randint(0, 1 << rs.randint(1, 20), 256) * (rs.rand(256) < rs.rand()))
    cases.append(rs.randint(1, 1000, 256))                                     # all 256 symbols present
    cases.append(np.arange(1, 257))
    for sym in (0, 5, 0xF0, 255):                                              # one symbol present
        one = np.zeros(256, dtype=np.int64)
        one[sym] = 1 + sym
        cases.append(one)
    for n in (2, 3, 7, 12, 162, 255, 256):                                     # equal counts: every choice is a tie
        eq = np.zeros(256, dtype=np.int64)
        eq[:n] = 9
        cases.append(eq)
        cases.append(eq[::-1].copy())
    cases.append(np.where(np.arange(256) % 3 == 0, 1, 0))                      # ties with the reserved symbol's 1
    for f in cases:
        if not np.any(f):
            continue
        got, want = JE.huff_optimal(f), optimal_table(f)
        assert same_table(got, want), f.tolist()
        code, ln = canonical_codes(want[0], want[1])
        assert got["code"].tolist() == code and got["len"].tolist() == ln
        assert sum(want[0]) == len(want[1]) == int(np.count_nonzero(f))
        assert sum(b * 2.0 ** -(l + 1) for l, b in enumerate(want[0])) < 1.0      # the all-ones code stays free
    one = JE.huff_optimal(cases[62])
    assert one["bits"].tolist() == [1] + [0] * 15 and one["vals"] == b"\x00" and one["len"][0] == 1 and one["code"][0] == 0
    # depths above 16: the limiting path; 1, 2, 3, 5, 8, ... beside the reserved symbol's 1
    for n, steps in ((18, 3), (30, 68)):
        got, want = JE.huff_optimal(fibonacci_counts(n)), optimal_table(fibonacci_counts(n))
        assert same_table(got, want) and want[3] == steps and want[2] == OK and max(got["len"]) == 16
    # 32 symbols reach depth 32, which libjpeg still limits; 33 is its JERR_HUFF_CLEN_OVERFLOW
    assert same_table(JE.huff_optimal(fibonacci_counts(32)), optimal_table(fibonacci_counts(32)))
    assert int(fibonacci_counts(33).sum()) < 2 ** 31
    for n in (33, 40):
        got = JE.huff_optimal(fibonacci_counts(n))
        assert got["status"] == JE.HUFF_CLEN_OVERFLOW == CLEN_OVERFLOW == optimal_table(fibonacci_counts(n))[2]
        assert got["vals"] == b"" and not got["bits"].any() and not got["len"].any()
    assert JE.huff_optimal(np.zeros(256))["status"] == JE.HUFF_EMPTY
    with pytest.raises(ValueError):
        JE.huff_optimal(np.full(256, 10 ** 7))
    with pytest.raises(_lib.TStarHipError):
        bad = np.zeros(1, dtype=JE.SPEC_DTYPE).repeat(4)
        JE.header_from_specs(77, 45, bad)


def test_the_limiting_step_against_pillow():
    """A gray picture whose AC-luma counts are 1, 2, 3, 5, ... (one AC basis function per block): libjpeg itself has to limit the
    table.  The smallest number of block types at which it does, and the 18 types of 1368 x 512 that need 5 steps from depth 19."""
    from tstar_amd import jpeg_encode as JE
    steps = {}
    for types in (15, 16, 18):
        a = deep_table_picture(types)
        for kw in (dict(), dict(restart_marker_blocks=8)):
            rst = dict(restart_blocks=kw.get("restart_marker_blocks", 0))
            want = pillow_optimize_bytes(a, 80, "4:4:4", **rst)
            hist = file_histograms(want, 1, 1, a.shape[1], a.shape[0])
            tabs = file_tables(want)
            table = optimal_table(hist[1])
            assert (table[0], table[1]) == (tabs[1][1], tabs[1][2])
            steps[types] = table[3]
            if types != 15:
                assert JE.encode_frames(a, 80, "4:4:4", device=False, optimize=True, **rst) == [want], (types, kw)
                assert JE.huff_optimal(hist[1])["steps"] == table[3]
    assert deep_table_picture(18).shape == (1368, 512, 3)
    assert steps[15] == 0 and steps[16] >= 1 and steps[18] == 5, steps


def test_header_keyword_and_plan():
    from PIL import Image
    from tstar_amd import jpeg
    from tstar_amd import jpeg_encode as JE
    from tstar_amd.video import FrameStore
    for H, W, s in GEOMETRIES:
        hs, vs = JE.sampling(s)
        a = rst_picture("noise", H, W, s)
        for kw in (dict(), dict(restart_blocks=4)):
            R = interval_of(H, W, s, **kw)
            std = pillow_restart_bytes(a, 75, s, **kw) if kw else pillow_bytes(a, 75, s)
            # optimize=False is the encode as it was
            assert JE.encode_frames(a, 75, s, device=False, optimize=False, **kw) == JE.encode_frames(a, 75, s, device=False, **kw) == [std]
            out, lengths, status = JE.encode_host(a, 75, s, optimize=False, **kw)
            assert out[0, :lengths[0]].tobytes() == std
            want = pillow_optimize_bytes(a, 75, s, **kw)
            assert len(want) < len(std)
            # the four DHT segments, a segment each, in the order DC 0, AC 0, DC 1, AC 1, between SOF0 and DRI / SOS
            head = want[:sos_end(want)]
            plain = JE.header(W, H, 75, s, **kw)
            tabs = file_tables(want)
            assert [t[0] for t in tabs] == [0x00, 0x10, 0x01, 0x11]
            assert head == plain[:177] + b"".join(t[3] for t in tabs) + plain[609:]
            coef, _ = JE.blocks_host(a, 75, s)
            got = {}
            scans, _, st = JE.scan_host(coef, W, H, s, optimize=True, tables=got, **kw)
            assert st[0] == 0 and head + scans[0] == want
            assert JE.header_from_specs(W, H, got["specs"][0], 75, s, restart=R) == head == plain[:177] + JE.dht_segments(got["specs"][0]) + plain[609:]
            # a file reopens through the project's probe and host decoder to Pillow's pixels
            if W // hs > 2:
                rc, info, _ = jpeg.probe(want)
                assert rc == 0 and (int(info[0]), int(info[1])) == (W, H)
                dcoef, dquant = np.zeros((1, coef.shape[1]), dtype=np.int16), np.zeros((1, 192), dtype=np.uint16)
                status, msg = jpeg.entropy_batch([want], (W, H, 3, hs, vs), dcoef, dquant)
                assert status[0] == 0 and np.array_equal(dcoef, coef), msg
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(want))), np.asarray(Image.open(io.BytesIO(std))))
        # the plan: the default is today's, field for field; optimize holds the longer codes, the longest header and the tables
        base, same, opt = JE.Plan(W, H, hs, vs, 3, 4096), JE.Plan(W, H, hs, vs, 3, 4096, optimize=False), JE.Plan(W, H, hs, vs, 3, 4096, optimize=True)
        assert [getattr(base, k) for k in JE.Plan.FIELDS] == [getattr(same, k) for k in JE.Plan.FIELDS] and not same.optimize
        assert base.header_bytes == 623 and opt.header_bytes == 177 + 4 * (2 + 2 + 17 + 256) + 14 == 1299
        assert JE.Plan(W, H, hs, vs, 3, 4096, 4, optimize=True).header_bytes == 1305
        assert opt.max_scan_bytes == 2 * ((opt.blocks * (27 + 63 * 26) + 7) // 8) + 2 > base.max_scan_bytes
        assert opt.workspace_bytes >= base.workspace_bytes + 3 * 4 * (257 * 4 + 768) and opt.off_hist % 16 == 0 and opt.off_codes % 16 == 0
    for fn in (JE.scan_host, JE.encode_host, JE.encode_frames, JE.frames_to_base64, JE.save_mjpeg, FrameStore.jpeg_frames, FrameStore.save_mjpeg):
        assert inspect.signature(fn).parameters["optimize"].default is False, fn
    assert JE.Plan.FIELDS == ("blocks", "coef_bytes", "max_scan_bytes", "header_bytes", "workspace_bytes", "block_wgs", "entropy_wgs_x",
                              "stuff_wgs_x")


def test_short_slots_and_containers(tmp_path):
    import base64
    from tstar_amd import jpeg
    from tstar_amd import jpeg_encode as JE
    H, W, s = GEOMETRIES[0]
    a = rst_picture("noise", H, W, s)
    ref = pillow_optimize_bytes(a, 75, s, restart_blocks=4)
    L = len(ref)
    for cap, want in ((L, JE.STATUS_OK), (L - 1, JE.STATUS_SHORT), (200, JE.STATUS_SHORT), (0, JE.STATUS_SHORT)):
        buf = np.full(L + 64, 0xA5, dtype=np.uint8)
        _, lengths, status = JE.encode_host(a, 75, s, slot_bytes=cap, out=buf, optimize=True, restart_blocks=4)
        assert status[0] == want and lengths[0] == L
        assert buf[:L].tobytes() == ref and (buf[L:] == 0xA5).all() if want == JE.STATUS_OK else (buf == 0xA5).all()
    frames = np.stack([a, rst_picture("smooth", H, W, s)])
    path = str(tmp_path / "o.avi")
    assert JE.save_mjpeg(frames, path, quality=90, device=False, optimize=True, restart_blocks=8) == 2
    src = jpeg.avi_mjpeg(path)
    try:
        assert [bytes(src.read(i)) for i in range(2)] == [pillow_optimize_bytes(f, 90, s, restart_blocks=8) for f in frames]
    finally:
        src.close()
    assert JE.frames_to_base64(frames, optimize=True) == [base64.b64encode(pillow_optimize_bytes(f, 75, s)).decode() for f in frames]


def test_surface():
    from tstar_amd import _lib
    new = {"tstar_jpeg_encode_plan_opt", "tstar_jpeg_huff_optimal", "tstar_jpeg_encode_header_opt", "tstar_jpeg_encode_scan_host_opt",
           "tstar_jpeg_encode_host_opt", "tstar_jpeg_encode_scan_opt"}
    with open(os.path.join(ROOT, "include", "tstar_hip.h")) as f:
        declared = set(re.findall(r"\b(tstar_[a-z0-9_]+)\s*\(", f.read()))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in new)


def test_host_twin_with_optimised_tables_under_address_and_ub_sanitizers(tmp_path):
    """The twin built with -fsanitize=address,undefined (CPU build; nothing of the GPU is involved) and driven by
    csrc/jpeg_enc_opt_check_main.cpp over tiny geometries, exact and short slots and the extreme histograms.  Any out-of-bounds
    access or undefined operation aborts the tool."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_enc_opt_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_enc_host.cpp"), os.path.join(csrc, "jpeg_host.cpp"), os.path.join(csrc, "jpeg_enc_opt_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler lacks the sanitizer runtime: " + r.stderr.strip().splitlines()[-1][:200])
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 8 * 4 + 1 and all(" ok=1" in ln for ln in lines), r.stdout
