"""CPU: the split entropy path without a GPU -- tstar_jpeg_entropy_split_host (sub-sequences, relaxation rounds, scan, write
pass, redo: the device launcher's mirror, same core, same round order) against the sequential host decoder
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
SIZES = [(8, 8), (17, 33), (97, 301)]
QUALITIES = [30, 100]
GUARD = 1024
SENTINEL16, SENTINEL32, SENTINEL64 = 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def sub_sizes():
    from tstar_amd import jpeg
    assert jpeg.SUB_BYTES_MIN == 8 and jpeg.SPLIT_SUB_BYTES not in (jpeg.SUB_BYTES_MIN, 64)
    return [jpeg.SUB_BYTES_MIN, 64, jpeg.SPLIT_SUB_BYTES]


def host_decode(datas, geom):
    """The yardstick: (coef int16 [n, blocks * 64], quant uint16 [n, 192], status int32 [n])."""
    from tstar_amd import jpeg
    blocks = jpeg._sizes(geom)[0]
    coef = np.zeros((len(datas), blocks * 64), dtype=np.int16)
    quant = np.zeros((len(datas), 192), dtype=np.uint16)
    status, _ = jpeg.entropy_batch(datas, geom, coef, quant)
    return coef, quant, status


def enough_rounds(plan, sub_bytes):
    """Sub-sequence i of a segment starts from the sequential decoder's state from round i on (the first one always does), so
    no exit changes after round n - 1 of an n-sub-sequence segment: it has converged by round n."""
    lens = (plan.segments["end"] - plan.segments["begin"]).astype(np.int64)
    return max(1, int((lens.max(initial=1) + sub_bytes - 1) // sub_bytes))


def split_decode(datas, geom, sub_bytes, min_split_bytes, max_rounds=None, plan=None):
    """plan + the split path on the CPU, every output and the workspace between sentinels
    -> (plan, coef [n, blocks * 64], seg_status, seg_info)."""
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    if plan is None:
        plan = jpeg.plan_segments(datas, geom)
    n, nseg = len(datas), len(plan.segments)
    assert nseg > 0
    if max_rounds is None:
        max_rounds = enough_rounds(plan, sub_bytes)
    blocks = jpeg._sizes(geom)[0]
    buf = np.frombuffer(b"".join(datas), dtype=np.uint8)
    assert plan.total_bytes == len(buf)
    ws_bytes = jpeg.split_workspace_bytes(len(buf), nseg, sub_bytes)
    assert ws_bytes % 8 == 0
    coef = np.full(n * blocks * 64 + 2 * GUARD, SENTINEL16, dtype=np.int16)
    status = np.full(nseg + 2 * GUARD, SENTINEL32, dtype=np.int32)
    info = np.full(nseg + 2 * GUARD, SENTINEL32, dtype=np.int32)
    ws = np.full(ws_bytes // 8 + 2 * GUARD, SENTINEL64, dtype=np.uint64)
    rc = lib.tstar_jpeg_entropy_split_host(buf.ctypes.data, len(buf), plan.segments.ctypes.data, plan.table_sets.ctypes.data,
                                           len(plan.table_sets), plan.frames.ctypes.data, n, nseg, *geom, sub_bytes, min_split_bytes,
                                           max_rounds, ws[GUARD:].ctypes.data, ws_bytes, coef[GUARD:].ctypes.data,
                                           status[GUARD:].ctypes.data, info[GUARD:].ctypes.data)
    assert rc == 0, lib.tstar_last_error()
    for arr, fill in ((coef, SENTINEL16), (status, SENTINEL32), (info, SENTINEL32), (ws, SENTINEL64)):
        assert (arr[:GUARD] == fill).all() and (arr[-GUARD:] == fill).all(), "a write outside the output buffers or the workspace"
    return plan, coef[GUARD:-GUARD].reshape(n, blocks * 64), status[GUARD:GUARD + nseg], info[GUARD:GUARD + nseg]


def seg_lens(plan):
    return (plan.segments["end"] - plan.segments["begin"]).astype(np.int64)


def check_info(plan, info, min_split_bytes):
    """Split and converged for every segment of at least min_split_bytes, one lane for every other."""
    long = seg_lens(plan) >= min_split_bytes
    assert (info[long] > 0).all(), info[long]
    assert (info[~long] == 0).all()


@pytest.mark.parametrize("sub", [0, 1, 2], ids=["smallest", "64", "default"])
@pytest.mark.parametrize("sampling", JU.SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_equals_the_sequential_decoder(size, sampling, sub):
    """{synthetic, noise} x {default, optimised, restart tables} x qualities {30, 100} of one geometry in one call: segments
    above and below min_split_bytes and several table sets side by side."""
    from tstar_amd import jpeg
    sub_bytes = sub_sizes()[sub]
    H, W = size
    datas = [d for q in QUALITIES for _, d in JU.matrix_files(H, W, sampling, q)]
    geom = jpeg.probe(datas[0])[1]
    want_c, want_q, want_s = host_decode(datas, geom)
    assert not want_s.any()
    min_split = 64
    plan, coef, seg_status, info = split_decode(datas, geom, sub_bytes, min_split)
    assert (plan.route == jpeg.ROUTE_DEVICE).all()
    assert not seg_status.any()
    assert np.array_equal(plan.quant, want_q)
    bad = np.nonzero((coef != want_c).any(axis=1))[0]
    assert len(bad) == 0, f"frames {bad.tolist()} differ from the sequential decoder's coefficients"
    check_info(plan, info, min_split)
    assert (info > 0).any() and len(plan.table_sets) >= 2


def _long_code_lengths(data):
    out = 0
    for m, a, b in JU.segments(data)[0]:
        if m == 0xC4:
            q = a + 4
            while q < b:
                counts = data[q + 1:q + 17]
                out += sum(counts[9:])
                q += 17 + sum(counts)
    return out


def test_the_matrix_holds_the_hard_places():
    """What the matrix above must contain to mean anything, asserted on the very streams it decodes: a cut on the 00 of an FF 00
    pair, codes longer than the 9-bit fast table, a block that spans three or more sub-sequences, and one launch that mixes
    segments above and below min_split_bytes and two table sets."""
    from tstar_amd import jpeg
    H, W = 97, 301
    files = dict(JU.matrix_files(H, W, "420", 100))
    noise = files["noise/optimize"]
    assert _long_code_lengths(noise) >= 1, "no code longer than 9 bits"
    geom = jpeg.probe(noise)[1]
    plan = jpeg.plan_segments([noise], geom)
    assert len(plan.segments) == 1
    begin, end = int(plan.segments["begin"][0]), int(plan.segments["end"][0])
    for sub_bytes in sub_sizes()[:2]:
        cuts = [p for p in range(begin + sub_bytes, end, sub_bytes) if noise[p - 1] == 0xFF and noise[p] == 0x00]
        assert cuts, f"no cut of {sub_bytes}-byte sub-sequences lands on the 00 of an FF 00 pair"
    # more sub-sequences than blocks + 1: one of them holds no block boundary, so its block spans three or more
    blocks = jpeg._sizes(geom)[0]
    n_sub = (end - begin + 7) // 8
    assert n_sub > blocks + 1
    _, coef, seg_status, info = split_decode([noise], geom, 8, 64, plan=plan)
    assert not seg_status.any() and info[0] > 1 and np.array_equal(coef, host_decode([noise], geom)[0])
    # the mix, in the 17x33 cell
    datas = [d for q in QUALITIES for _, d in JU.matrix_files(17, 33, "420", q)]
    geom = jpeg.probe(datas[0])[1]
    plan, _, _, info = split_decode(datas, geom, 64, 64)
    assert (info == 0).any() and (info > 0).any() and len(plan.table_sets) >= 2
    assert len({int(plan.frames["table_set"][f]) for f in plan.segments["frame"][info > 0]}) >= 2, "the cut segments share one table set"


def test_a_flat_picture_completes_more_than_an_mcu_row_per_sub_sequence():
    """A flat picture at quality 30 is a few bits per block: a sub-sequence of the default size completes more blocks than an MCU
    row holds, so its lane crosses a row of MCUs (and the predictors of hundreds of blocks come out of the scan)."""
    from tstar_amd import jpeg
    H, W = 97, 301
    flat = np.full((H, W, 3), (90, 140, 200), dtype=np.uint8)
    data = JU.encode(flat, "420", 30)
    geom = jpeg.probe(data)[1]
    plan = jpeg.plan_segments([data], geom)
    blocks = jpeg._sizes(geom)[0]
    sub_bytes = jpeg.SPLIT_SUB_BYTES
    n_sub = (int(seg_lens(plan)[0]) + sub_bytes - 1) // sub_bytes
    row = ((W + 15) // 16) * 6
    assert n_sub >= 2 and blocks / n_sub > row, "no sub-sequence is sure to complete more than one MCU row"
    want_c, _, want_s = host_decode([data], geom)
    for sb in sub_sizes():
        _, coef, seg_status, info = split_decode([data], geom, sb, 64, plan=plan)
        assert not want_s.any() and not seg_status.any() and info[0] > 0 and np.array_equal(coef, want_c)


def test_one_round_abandons_what_needs_more_and_zero_never_splits():
    from tstar_amd import jpeg
    datas = [JU.encode(JU.noise_picture(97, 301, seed=11), "420", 75), JU.encode(JU.noise_picture(97, 301, seed=12), "420", 75, "restart")]
    geom = jpeg.probe(datas[0])[1]
    want_c, want_q, want_s = host_decode(datas, geom)
    assert not want_s.any()
    plan, coef, seg_status, info = split_decode(datas, geom, 64, 64)
    assert info[0] > 1, "the stream converges in the first round: nothing to abandon"
    check_info(plan, info, 64)
    assert not seg_status.any() and np.array_equal(coef, want_c)
    # one round only
    _, coef1, status1, info1 = split_decode(datas, geom, 64, 64, max_rounds=1, plan=plan)
    assert info1[0] == -1
    assert (info1[info > 1] == -1).all() and np.array_equal(info1[info <= 1], info[info <= 1])
    assert not status1.any() and np.array_equal(coef1, want_c)
    # exactly as many rounds as it takes, and one fewer
    need = int(info.max())
    _, coef2, status2, info2 = split_decode(datas, geom, 64, 64, max_rounds=need, plan=plan)
    assert np.array_equal(info2, info) and not status2.any() and np.array_equal(coef2, want_c)
    _, coef3, status3, info3 = split_decode(datas, geom, 64, 64, max_rounds=need - 1, plan=plan)
    assert (info3[info == need] == -1).all() and not status3.any() and np.array_equal(coef3, want_c)
    # never split: the one-lane path alone
    buf = np.frombuffer(b"".join(datas), dtype=np.uint8)
    core_c, core_s = jpeg.entropy_segments_host(buf, plan, geom)
    _, coef0, status0, info0 = split_decode(datas, geom, 64, 0, plan=plan)
    assert not info0.any() and np.array_equal(status0, core_s) and np.array_equal(coef0, core_c)


def _segment_with_remainder(sub_bytes, remainder):
    from tstar_amd import jpeg
    for seed in range(2000):
        data = JU.encode(JU.noise_picture(17, 33, seed=seed), "420", 75)
        geom = jpeg.probe(data)[1]
        plan = jpeg.plan_segments([data], geom)
        n = int(seg_lens(plan)[0])
        if n >= 2 * sub_bytes and n % sub_bytes == remainder:
            return data, geom, plan
    raise AssertionError(f"no 17x33 stream whose segment is {remainder} over a multiple of {sub_bytes} bytes")


@pytest.mark.parametrize("sub_bytes", [8, 64])
@pytest.mark.parametrize("remainder", [0, 1])
def test_segment_lengths_at_the_edge_of_a_sub_sequence(sub_bytes, remainder):
    """A segment that is a whole number of sub-sequences, and one that is one byte over (its last sub-sequence is that byte)."""
    data, geom, plan = _segment_with_remainder(sub_bytes, remainder)
    want_c, _, want_s = host_decode([data], geom)
    _, coef, seg_status, info = split_decode([data], geom, sub_bytes, 1, plan=plan)
    assert not want_s.any() and not seg_status.any() and info[0] > 0 and np.array_equal(coef, want_c)


def test_a_frame_of_one_block():
    from tstar_amd import jpeg
    for q in (30, 100):
        data = JU.encode(JU.noise_picture(8, 8, seed=q), "gray", q)
        geom = jpeg.probe(data)[1]
        assert jpeg._sizes(geom)[0] == 1
        want_c, _, want_s = host_decode([data], geom)
        for sb in sub_sizes():
            _, coef, seg_status, info = split_decode([data], geom, sb, 1)
            assert not want_s.any() and not seg_status.any() and info[0] > 0 and np.array_equal(coef, want_c)


def broken_streams():
    """Truncated, flipped, stray-byte and loud variants of a restart-coded and a marker-free 97x301 stream, the intact two first."""
    data = JU.encode(JU.noise_picture(97, 301, seed=3), "420", 75, "restart")
    plain = JU.encode(JU.noise_picture(97, 301, seed=3), "420", 75)
    datas = [data, plain, plain[:-2] + b"\x12\x34\x56" + plain[-2:]]
    segs, _ = JU.segments(plain)
    a = next(a for m, a, _ in segs if m == 0xDB)
    loud = bytearray(plain)
    for k in range(64):
        loud[a + 5 + k] = min(255, 8 * loud[a + 5 + k])
    datas.append(bytes(loud))
    datas += [plain[:n] for n in range(0, len(plain), 97)] + [plain[:-1], plain[:-2]]
    for src in (data, plain):
        s0 = JU.segments(src)[1]
        for p in range(s0, len(src) - 2, max(1, (len(src) - 2 - s0) // 120)):
            m = bytearray(src)
            m[p] ^= 0xFF
            datas.append(bytes(m))
        for p in range(s0 + 5, len(src) - 2, max(1, (len(src) - 2 - s0) // 60)):
            m = bytearray(src)
            m[p] ^= 0x04
            datas.append(bytes(m))
    return datas


def test_broken_streams_have_the_sequential_decoders_status():
    """Wherever the sequential decoder's status is not OK so is the split path's, and it is the same status; an accepted stream
    (many flipped streams are valid streams of another picture) decodes to the same coefficients.  The write pass never
    refuses what one lane accepts: that would show as UNCOVERED where the sequential decoder says OK."""
    from tstar_amd import jpeg
    datas = broken_streams()
    geom = jpeg.probe(datas[0])[1]
    want_c, want_q, want_s = host_decode(datas, geom)
    plan = jpeg.plan_segments(datas, geom)
    routed = plan.route == jpeg.ROUTE_DEVICE
    assert routed.sum() > 100 and (want_s[~routed] != jpeg.OK).all()
    seen = set()
    for sub_bytes in sub_sizes()[1:]:
        _, coef, seg_status, info = split_decode(datas, geom, sub_bytes, 64, plan=plan)
        got = plan.frame_status(seg_status)
        assert np.array_equal(got[routed], want_s[routed])
        ok = routed & (want_s == jpeg.OK)
        assert ok.sum() >= 3 and np.array_equal(coef[ok], want_c[ok]) and np.array_equal(plan.quant[ok], want_q[ok])
        check_info(plan, info, 64)
        seen |= set(got[routed].tolist())
        # and segment by segment the one-lane core's statuses
        buf = np.frombuffer(b"".join(datas), dtype=np.uint8)
        assert np.array_equal(seg_status, jpeg.entropy_segments_host(buf, plan, geom)[1])
    assert seen == {jpeg.OK, jpeg.MALFORMED, jpeg.UNCOVERED}


def test_bad_arguments_are_refused_and_the_workspace_query_does_no_work():
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    data = JU.encode(JU.noise_picture(17, 33, seed=1), "420", 75)
    geom = jpeg.probe(data)[1]
    plan = jpeg.plan_segments([data], geom)
    buf = np.frombuffer(data, dtype=np.uint8)
    blocks = jpeg._sizes(geom)[0]
    q = lib.tstar_jpeg_split_workspace_bytes
    need = q(len(buf), 1, 64)
    assert need > 0 and need % 8 == 0 and q(len(buf), 1, 8) > need > q(len(buf), 1, 128)
    assert q(0, 1, 64) == 0 and q(len(buf), 0, 64) == 0 and q(len(buf), 1, 4) == 0 and q(len(buf), 1, 66) == 0 and q(1 << 32, 1, 64) == 0
    with pytest.raises(ValueError):
        jpeg.split_workspace_bytes(len(buf), 1, 7)
    coef = np.full(blocks * 64, SENTINEL16, dtype=np.int16)
    status, info = np.full(1, SENTINEL32, dtype=np.int32), np.full(1, SENTINEL32, dtype=np.int32)
    ws = np.zeros(need // 8, dtype=np.uint64)
    good = [buf.ctypes.data, len(buf), plan.segments.ctypes.data, plan.table_sets.ctypes.data, 1, plan.frames.ctypes.data, 1, 1, *geom,
            64, 64, 8, ws.ctypes.data, need, coef.ctypes.data, status.ctypes.data, info.ctypes.data]
    for at, value in ((0, None), (2, None), (3, None), (5, None), (16, None), (18, None), (19, None), (20, None), (4, 0), (6, 0), (7, 0),
                      (1, 0), (8, 0), (11, 3), (13, 4), (13, 0), (13, 66), (13, -64), (14, -1), (15, 0), (15, -1), (15, (1 << 16) + 1),
                      (17, need - 1), (17, 0), (16, ws.ctypes.data + 4)):
        args = list(good)
        args[at] = value
        assert lib.tstar_jpeg_entropy_split_host(*args) == 1, (at, value)
    assert (coef == SENTINEL16).all() and status[0] == SENTINEL32 and info[0] == SENTINEL32 and not ws.any()      # nothing ran
    assert lib.tstar_jpeg_entropy_split_host(*good) == 0
    assert status[0] == jpeg.OK and info[0] > 0 and np.array_equal(coef, host_decode([data], geom)[0][0])


def test_the_knob(monkeypatch):
    from tstar_amd import jpeg
    monkeypatch.delenv("TSTAR_JPEG_SPLIT_BYTES", raising=False)
    assert jpeg.split_min_bytes() == jpeg.SPLIT_MIN_BYTES > 0
    for text, want in (("0", 0), ("1", 1), ("4096", 4096), ("", jpeg.SPLIT_MIN_BYTES)):
        monkeypatch.setenv("TSTAR_JPEG_SPLIT_BYTES", text)
        assert jpeg.split_min_bytes() == want
    for text in ("-1", "many", str(1 << 31)):
        monkeypatch.setenv("TSTAR_JPEG_SPLIT_BYTES", text)
        with pytest.raises(ValueError, match="TSTAR_JPEG_SPLIT_BYTES"):
            jpeg.split_min_bytes()
    assert jpeg.SPLIT_SUB_BYTES % 4 == 0 and jpeg.SPLIT_SUB_BYTES >= jpeg.SUB_BYTES_MIN and 1 <= jpeg.SPLIT_MAX_ROUNDS <= 1 << 16
    # the host mode has no use for it
    monkeypatch.setenv("TSTAR_JPEG_SPLIT_BYTES", "many")
    from tstar_amd.video import open_video
    st = open_video([JU.encode(JU.synthetic_picture(40, 50, frame=i), "420") for i in range(2)], device="cpu")
    assert st.entropy_stats == {"device": 0, "host": 2} and st.entropy_split_stats == {"split": 0, "abandoned": 0, "rounds_max": 0}


def test_split_core_under_address_and_ub_sanitizers(tmp_path):
    """The host mirror built with -fsanitize=address,undefined (a stand-alone CPU program; nothing is loaded into python, nothing
    of the GPU is involved) and driven by csrc/jpeg_split_check_main.cpp: every truncation and every single byte of the entropy
    data corrupted in three ways for two small streams, a spread of both for the rest of the corpus, with sub-sequences of 8,
    64 and 128 bytes and with one round only, every buffer and the workspace an exact-size heap block.  An out-of-bounds
    access or undefined operation aborts the tool; it also requires status OK <=> the sequential decoder's OK."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_split_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_host.cpp"), os.path.join(csrc, "jpeg_split_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []

    def add(name, data):
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(data)
        files.append(str(p))

    add("small_noise", JU.encode(JU.noise_picture(17, 33, seed=2), "420", 75))                       # the two exhaustive ones first
    add("small_synthetic", JU.encode(JU.synthetic_picture(17, 33), "444", 90, "optimize"))
    for kind, pic in (("s", JU.synthetic_picture(40, 50)), ("n", JU.noise_picture(33, 17, seed=2))):
        for sampling, tables in (("420", "default"), ("422", "restart"), ("444", "optimize"), ("gray", "default")):
            add(f"{kind}_{sampling}_{tables}", JU.encode(pic, sampling, 75, tables))
    add("long_codes", JU.encode(JU.noise_picture(97, 301, seed=3), "420", 100, "optimize"))
    add("flat", JU.encode(np.full((97, 301, 3), (90, 140, 200), dtype=np.uint8), "420", 30))
    add("one_block", JU.encode(JU.noise_picture(8, 8, seed=1), "gray", 100))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "--exhaustive", "2"] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files) and all(" intact=0 " in ln and ln.endswith(" differ=0") for ln in lines), r.stdout
    assert all(int(ln.split(" streams=")[1].split()[0]) > 300 for ln in lines[:2]), "the exhaustive sweeps did not run"
