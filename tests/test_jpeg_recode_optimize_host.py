"""CPU: lossless JPEG re-coding with optimised Huffman tables, host twin.  Per frame, Pillow is the yardstick byte for byte; the
shared tables of a group are held against the pure table procedure on the sum of per-frame counts; nothing but the entropy coding
changes; the guards (overflow, coefficients without a code, keywords, the environment variable, the default's stats)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_recode_optimize_util as OU  # noqa: E402
import jpeg_recode_util as U  # noqa: E402
import jpeg_util as JU  # noqa: E402

SUB = {"420": "4:2:0", "422": "4:2:2", "444": "4:4:4"}


def _recode(files, n, **kw):
    from tstar_amd import jpeg_encode as JE
    stats = {}
    return JE.recode_frames(files, restart_blocks=n, device=False, stats=stats, **kw), stats


# ------------------------------------------------------------------------------------------------ 1. Pillow, per frame
@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
@pytest.mark.parametrize("name", list(U.PILLOW_SOURCES))
def test_per_frame_recode_is_pillows_optimize_file(case, name):
    W, H, s, n = case
    rgb, data = U.source(W, H, s, name)
    out, stats = _recode([data], n, optimize=True)
    assert out[0] == OU.pillow_optimized(rgb, s, U.PILLOW_SOURCES[name], n)
    assert stats == {"recoded": 1, "bytes_in": len(data), "bytes_out": len(out[0]), "optimized": 1,
                     "table_bytes": sum(21 + len(v) for _, _, v in OU.dht_tables(out[0]))}


@pytest.mark.parametrize("geom", OU.PLAIN_GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}")
def test_recode_without_an_interval_is_pillows_optimize_file(geom):
    W, H, s = geom
    for name, q in U.PILLOW_SOURCES.items():
        rgb, data = U.source(W, H, s, name)
        out, stats = _recode([data], 0, optimize=True)
        assert out[0] == OU.pillow_optimized(rgb, s, q) and OU.markers(out[0]) == (0, [])
        if name == "optimize":
            assert out[0] == data                                         # an optimised source comes back as its own bytes
        assert stats["optimized"] == 1 and "kept" not in stats


def test_header_with_given_quant_rows_and_tables():
    """For the tables of a Pillow quality the new header function gives header_from_specs' bytes; with custom rows it is
    header_from_tables' layout with the four DHT segments replaced."""
    from tstar_amd import jpeg_encode as JE
    rgb, data = U.source(48, 48, "420", "q75")
    geom, coef, quant = U.host_coefficients(data)
    tables = {}
    JE.scan_host(coef[None], 48, 48, "4:2:0", threads=1, restart_blocks=3, optimize=True, tables=tables)
    sp = tables["specs"][0]
    for restart in (0, 3):
        assert JE.header_from_tables_specs(48, 48, quant, sp, "4:2:0", restart) == JE.header_from_specs(48, 48, sp, 75, "4:2:0", restart)
    wide = np.array(U.QTABLES[0] + U.QTABLES[1] + [v + 1 for v in U.QTABLES[1]])
    got, std = JE.header_from_tables_specs(48, 48, wide, sp, "4:2:0", 3), JE.header_from_tables(48, 48, wide, "4:2:0", 3)
    cut = lambda d: [d[a:b] for m, a, b in JU.segments(d)[0] if m != 0xC4]      # noqa: E731
    assert cut(got) == cut(std) and b"\xff\xc1" in got
    assert b"".join(d for d in [got[a:b] for m, a, b in JU.segments(got)[0] if m == 0xC4]) == JE.dht_segments(sp)
    with pytest.raises(ValueError):
        JE.header_from_tables_specs(48, 48, np.zeros(192), sp)


# ------------------------------------------------------------------------------------------------ 2. only the entropy coding changes
@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_nothing_but_the_entropy_coding_changes(case):
    W, H, s, n = case
    hs, vs = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}[s]
    mcus = (-(-W // (8 * hs))) * (-(-H // (8 * vs)))
    for name in U.SOURCES:
        _, data = U.source(W, H, s, name)
        (out,), stats = _recode([data], n, optimize=True)
        (std,), _ = _recode([data], n)
        assert stats.get("kept", 0) == 0 and stats["optimized"] == 1
        assert np.array_equal(OU.pixels(out), OU.pixels(data))
        g0, c0, q0 = U.host_coefficients(data)
        g1, c1, q1 = U.host_coefficients(out)
        assert g0 == g1 and np.array_equal(c0, c1) and np.array_equal(q0, q1)
        assert U.dqt_payloads(out) == U.dqt_payloads(data)
        n_markers = (mcus - 1) // n
        assert OU.markers(out) == (n, [k % 8 for k in range(n_markers)])
        assert len(out) <= len(std), (name, len(out), len(std))
        assert len(OU.dht_tables(out)) == 4 and [t[0] for t in OU.dht_tables(out)] == [0x00, 0x10, 0x01, 0x11]


# ------------------------------------------------------------------------------------------------ 3. shared tables
@pytest.mark.parametrize("group_frames", [1, 3, None], ids=["g1", "g3", "whole"])
def test_shared_tables_are_the_optimal_tables_of_the_summed_counts(group_frames):
    from tstar_amd import jpeg, jpeg_recode as JR
    n = 2
    files = U.batch(48, 48, "420")
    geom = JR.covered(files[0])
    stats, info = JR.new_stats(True), {}
    out = JR.recode_host_chunk(files, geom, n, group_frames, stats, info=info)
    assert JR.recode_host(files, n, optimize=True, shared=True, group_frames=group_frames) == out
    group, kept = info["group"], info["kept"]
    # kept frames sit between the frames of the groups and come back as their sources: the decoder returns OK for none of them
    # (grayscale, progressive, a category the decoder's tables refuse), so they belong to no group and the groups close over them
    assert kept.sum() == 3 and [out[j] for j in np.flatnonzero(kept)] == [files[j] for j in np.flatnonzero(kept)]
    assert (group[kept] == -1).all() and (group[~kept] >= 0).all() and 0 < np.flatnonzero(kept)[0] < len(files) - 1
    members = [np.flatnonzero(group == g) for g in range(int(group.max()) + 1)]
    size = group_frames or len(files)
    assert all(len(m) <= size for m in members) and all(len(m) == size for m in members[:-1]) and sum(map(len, members)) == 10
    plan = jpeg.plan_segments(out, geom)
    sets = set()
    for g, m in enumerate(members):
        counts = sum(OU.frame_counts(files[j], n).astype(np.int64) for j in m).astype(np.uint32)
        assert np.array_equal(counts, info["hist"][g])
        want = OU.tables_of_counts(counts)
        for j in m:
            if kept[j]:
                continue
            assert [(b.tolist(), v) for _, b, v in OU.dht_tables(out[j])] == want
            assert np.array_equal(OU.pixels(out[j]), OU.pixels(files[j]))
            # the Huffman part of the frame's decoder table set is what the planner makes of the output file's own DHT segments
            ts = plan.table_sets[plan.frames["table_set"][j]]
            assert np.array_equal(JR.huffman_of_specs(info["specs"][g]), ts[:JR._HUFF_BYTES])
            src = jpeg.plan_segments([files[j]], geom)
            assert np.array_equal(JR.optimized_table_set(src.table_sets[0], info["specs"][g]), ts)
            sets.add((g, plan.quant[j].tobytes()))
    assert stats["table_sets"] == len(sets) and stats["optimized"] == stats["recoded"] == 10 and stats["kept"] == 3
    assert stats["bytes_out"] == sum(map(len, out)) and "table_bytes" not in stats
    if group_frames == 1:
        assert out == _recode(files, n, optimize=True)[0]                 # groups of one frame: the per-frame files


def test_the_per_frame_mode_is_the_shared_mode_with_groups_of_one():
    """What the one scan stage rests on: a frame's own tables are the tables of a group that holds the frame alone.  File for file,
    and every stats key but the two that say how tables are counted (bytes per frame, sets per arena)."""
    from tstar_amd import jpeg_recode as JR
    for files, n, want, want_stats in OU.groups_of_one_cases():
        stats = {}
        assert JR.recode_host(files, n, stats, optimize=True, shared=True, group_frames=1) == want
        assert set(want_stats) - set(stats) == {"table_bytes"} and set(stats) - set(want_stats) == {"table_sets"}
        assert OU.without(stats, "table_sets") == OU.without(want_stats, "table_bytes")
        bare = {}                                                           # the chunk entry alone, from an empty dict: the same keys
        assert JR.recode_host_chunk(files, JR.covered(files[0]), n, 1, bare) == want and bare == stats
        gray = [JR.covered(f) is None for f in files]
        assert want_stats.get("kept", 0) == sum(gray) and want_stats["optimized"] == stats["table_sets"] == len(files) - sum(gray)
        assert [a == b for a, b in zip(want, files)] == gray                # the grayscale file alone comes back as it was
        assert all(OU.markers(o) == (n, [k % 8 for k in range(4 if n else 0)]) for o, g in zip(want, gray) if not g)


# ------------------------------------------------------------------------------------------------ 4. guards
def test_a_group_whose_table_overflows_is_kept_whole():
    from tstar_amd import jpeg_encode as JE, jpeg_recode as JR
    files = U.batch(48, 48, "420", with_kept=False)[:7]
    geom = JR.covered(files[0])
    plain = JR.recode_host_chunk(files, geom, 2, 3)
    for table in range(4):
        stats, info = JR.new_stats(True), {}
        out = JR.recode_host_chunk(files, geom, 2, 3, stats, counts=OU.fibonacci_hist(3, 1, table, 33), info=info)
        assert info["specs"]["status"][1].tolist() == [JE.HUFF_CLEN_OVERFLOW if t == table else JE.HUFF_OK for t in range(4)]
        assert out[3:6] == files[3:6] and info["kept"].tolist() == [False] * 3 + [True] * 3 + [False]
        assert stats["kept"] == 3 and stats["recoded"] == stats["optimized"] == 4
        assert all(np.array_equal(OU.pixels(out[j]), OU.pixels(files[j])) for j in (0, 1, 2, 6))
    # 32 symbols are still limited to 16 bits: nothing is kept
    info = {}
    JR.recode_host_chunk(files, geom, 2, 3, counts=OU.fibonacci_hist(3, 1, 1, 32), info=info)
    assert not info["kept"].any() and len(plain) == 7


@pytest.mark.parametrize("value", [1024, -32768])
def test_a_coefficient_without_a_code_keeps_the_frame_and_stays_inside_the_histogram(value):
    from tstar_amd import jpeg_encode as JE, jpeg_recode as JR
    geom = (48, 48, 3, 2, 2)
    _, data = U.source(48, 48, "420", "q75")
    _, coef, quant = U.host_coefficients(data)
    coefs = np.stack([coef, coef, coef]).copy()
    coefs[1, 64 * 7 + 5] = value                                          # an AC coefficient
    coefs[2, 0] = -32768                                                  # a DC value: the difference (category 16) has no code
    assert JR.code_host(coefs[1:2], quant, geom, 2, optimize=True) is None and JR.code_host(coefs[2:3], quant, geom, 2, optimize=True) is None
    tables = {}
    _, _, status = JE.scan_host(coefs, 48, 48, "4:2:0", threads=1, restart_blocks=2, optimize=True, tables=tables)
    assert status.tolist() == [JE.STATUS_OK, JE.STATUS_BAD_COEF, JE.STATUS_BAD_COEF]
    group = np.array([0, 0, 0], dtype=np.int32)
    scans, st, specs, hist = JR.code_host_shared(coefs, geom, 2, group, 1)
    assert st.tolist() == status.tolist() and scans[1] is None and scans[2] is None and scans[0] is not None
    # every frame has counted, every block one DC symbol; the reserved bin and everything beyond the categories stays empty
    assert np.array_equal(hist[0], tables["hist"].sum(axis=0))
    assert int(hist[0, 0].sum() + hist[0, 2].sum()) == 3 * 54 and not hist[0, :, 256].any() and not hist[0, [0, 2], 12:].any()
    assert not (hist[0, [1, 3]][:, [s for s in range(256) if s & 15 > 10]]).any()


def test_keywords_and_the_environment_variable(tmp_path, monkeypatch):
    from tstar_amd import jpeg_encode as JE, jpeg_recode as JR, jpeg_resident
    from tstar_amd.video import open_video
    _, data = U.source(48, 48, "420", "q75")
    with pytest.raises(ValueError, match="1..65535"):
        JE.recode_frames([data], restart_blocks=0, device=False)
    with pytest.raises(ValueError, match="1..65535"):
        JE.recode_mjpeg(str(tmp_path / "none.mjpeg"), str(tmp_path / "out.mjpeg"), restart_blocks=0, device=False)
    with pytest.raises(ValueError, match="1..65535"):
        JR.recode_mode(0)
    with pytest.raises(ValueError, match="optimize"):
        JR.recode_host([data], 2, shared=True)
    with pytest.raises(ValueError, match="group_frames"):
        JR.recode_host_chunk([data], (48, 48, 3, 2, 2), 2, 0)
    assert JR.group_limit(36) == 1_000_000_000 // (36 * 64) and JR.group_limit(48960) == 319 and JR.group_limit(10 ** 8) == 1
    g, n = JR.make_groups(np.array([1, 0, 1, 1, 1, 0, 1], dtype=bool), 2)
    assert g.tolist() == [0, -1, 0, 1, 1, -1, 2] and n == 3
    assert JR.make_groups(np.zeros(3, dtype=bool), 2)[1] == 0
    path = str(tmp_path / "two.mjpeg")
    JU.write_mjpeg(path, [data, data])
    monkeypatch.delenv("TSTAR_JPEG_RECODE", raising=False)
    monkeypatch.delenv("TSTAR_JPEG_RECODE_OPTIMIZE", raising=False)
    with pytest.raises(ValueError, match="recode_blocks"):
        open_video(path, device="cpu", fps=1.0, resident="jpeg", recode_optimize=True)
    with pytest.raises(ValueError, match="recode_blocks"):
        open_video(path, device="cpu", fps=1.0, recode_optimize=True)
    with pytest.raises(ValueError, match="recode_blocks"):
        jpeg_resident.load_resident(None, "cuda", recode_optimize=True)
    # the variable is read only when the keyword is absent
    assert JR.recode_optimize_mode() is False and JR.recode_optimize_mode(True) is True
    monkeypatch.setenv("TSTAR_JPEG_RECODE_OPTIMIZE", "1")
    assert JR.recode_optimize_mode() is True and JR.recode_optimize_mode(False) is False
    monkeypatch.setenv("TSTAR_JPEG_RECODE_OPTIMIZE", "yes")
    assert JR.recode_optimize_mode(False) is False
    with pytest.raises(ValueError, match="TSTAR_JPEG_RECODE_OPTIMIZE"):
        JR.recode_optimize_mode()
    # the variable alone leaves a store that is not re-coded as it is
    monkeypatch.setenv("TSTAR_JPEG_RECODE_OPTIMIZE", "1")
    st = open_video(path, device="cpu", fps=1.0)
    assert st.num_seconds == 2 and not hasattr(st, "recode_stats")


def test_the_default_is_todays_recode(tmp_path):
    """optimize=False: the bytes and the stats dictionary of the standard-table re-code, no new key; recode_mjpeg carries the keyword."""
    from tstar_amd import jpeg_encode as JE, jpeg_recode as JR
    files = U.batch(48, 48, "420")
    out, stats = _recode(files, 2)
    assert out == _recode(files, 2, optimize=False)[0] == JR.recode_host(files, 2)
    assert stats == {"recoded": 10, "kept": 3, "bytes_in": sum(map(len, files)), "bytes_out": sum(map(len, out))}
    assert JR.new_stats() == {"recoded": 0, "kept": 0, "bytes_in": 0, "bytes_out": 0}
    opt, ostats = _recode(files, 2, optimize=True)
    assert set(ostats) == set(stats) | {"optimized", "table_bytes"} and ostats["optimized"] == 10 and ostats["kept"] == 3
    assert all(len(a) <= len(b) for a, b in zip(opt, out)) and ostats["bytes_out"] < stats["bytes_out"]
    src, dst = str(tmp_path / "src.mjpeg"), str(tmp_path / "dst.mjpeg")
    clean = U.batch(48, 48, "420", with_kept=False)
    JU.write_mjpeg(src, clean)
    for kw, want in ((dict(), _recode(clean, 2)[0]), (dict(optimize=True), _recode(clean, 2, optimize=True)[0]),
                     (dict(optimize=True, restart_blocks=0, piece=3), _recode(clean, 0, optimize=True)[0])):
        kw.setdefault("restart_blocks", 2)
        assert JE.recode_mjpeg(src, dst, device=False, **kw) == len(clean)
        with open(dst, "rb") as f:
            assert f.read() == b"".join(want)


# ------------------------------------------------------------------------------------------------ 5. sanitizers
def test_recode_optimize_sanitizer_program(tmp_path):
    """csrc/jpeg_recode_opt_check_main.cpp with the host twin of the shared-table scan stage, the header writer and the assembly's
    mirror, built with -fsanitize=address,undefined (a stand-alone CPU program; nothing is loaded into Python): exact-size heap
    blocks, groups with a frame outside them, crafted counts that overflow, coefficients of 1024 and -32768, refused arguments."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_recode_opt_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_recode_host.cpp"), os.path.join(csrc, "jpeg_enc_host.cpp"), os.path.join(csrc, "jpeg_host.cpp"),
           os.path.join(csrc, "jpeg_recode_opt_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the compiler lacks the sanitizer runtime: " + r.stderr.strip().splitlines()[-1][:200])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok" in run.stdout
