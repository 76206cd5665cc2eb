"""CPU: JPEG decode at 1/2, 1/4, 1/8 size without a GPU -- the host twin of the reduced inverse DCTs and the scaled chroma stage
against Pillow's ``Image.draft`` (libjpeg-turbo) BYTE FOR BYTE, the refusals, and open_video(device="cpu", jpeg_scale=s)."""
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_scale_util as SU  # noqa: E402
import jpeg_util as JU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_turbo():
    assert JU.turbo(), "Pillow here is not built on libjpeg-turbo: the byte-equality yardstick does not apply"


@pytest.mark.parametrize("sampling", SU.SAMPLINGS)
@pytest.mark.parametrize("size", SU.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_equals_pillow_draft(size, sampling):
    """Every scale, quality and kind of picture of one size and sampling: the bytes of im.draft(mode, (W // s, H // s)), whose size
    is asserted first.  The geometries the scaled decode does not cover (test_uncovered_...) are the only ones passed over, and
    only where the rule of DESIGN.md 8j says so."""
    _need_turbo()
    W, H = size
    checked = 0
    for quality in SU.QUALITIES:
        for kind in SU.KINDS:
            data = JU.encode(SU.picture(kind, W, H), sampling, quality)
            geom, coef, quant = SU.coefficients([data])
            for s in SU.SCALES:
                want = SU.pillow_draft(data, s)                      # asserts im.size == (ow, oh)
                rc, ow, oh, _, cov = SU.sizes(geom, s)
                assert rc == 0 and (ow, oh) == (want.shape[1], want.shape[0]) and bool(cov) == SU.covered(W, sampling, s)
                if not cov:
                    continue
                rc, got = SU.reconstruct_host(geom, coef, quant, s)
                assert rc == 0
                diff = np.nonzero(got[0] != want)
                assert len(diff[0]) == 0, f"{kind} q{quality} 1/{s}: {len(diff[0])} bytes differ, first at {[int(a[0]) for a in diff]}"
                checked += 1
    assert checked == 9 * sum(SU.covered(W, sampling, s) for s in SU.SCALES)


@pytest.mark.parametrize("size,s", [((8, 8), 2), ((16, 16), 4)], ids=["8x8-1/2", "16x16-1/4"])
def test_uncovered_422_is_reported_and_refused(size, s):
    """4:2:2 whose scaled chroma row is 2 samples long goes through libjpeg's triangle filter in a way this decoder does not state:
    the sizes entry says uncovered, the reconstruct entry refuses, the other samplings of the size are covered."""
    from tstar_amd import _lib
    W, H = size
    data = JU.encode(SU.picture("noise", W, H), "422", 75)
    geom, coef, quant = SU.coefficients([data])
    assert SU.chroma_row(W, "422", s) == 2
    assert SU.sizes(geom, s) == (0, SU.ceil_div(W, s), SU.ceil_div(H, s), SU.sizes(geom, s)[3], 0)
    rc, out = SU.reconstruct_host(geom, coef, quant, s)
    assert rc == 1 and (out == 0xA5).all() and "not covered at this scale" in _lib.load().tstar_last_error().decode()
    assert SU.sizes(geom, 8)[4] == 1                                   # replication has no such case
    for sampling in ("420", "444", "gray"):
        g2, _, _ = SU.coefficients([JU.encode(SU.picture("noise", W, H), sampling, 75)])
        assert SU.sizes(g2, s)[4] == 1, sampling


@pytest.mark.parametrize("sampling", SU.SAMPLINGS)
def test_scale_1_is_the_existing_entry(sampling):
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    W, H = 77, 45
    datas = [JU.encode(SU.picture(kind, W, H), sampling, 75) for kind in ("noise", "gradient")]
    geom, coef, quant = SU.coefficients(datas)
    want = np.empty((2, H, W, 3), dtype=np.uint8)
    _lib.check(lib.tstar_jpeg_reconstruct_host(coef.ctypes.data, quant.ctypes.data, 2, *geom, want.ctypes.data, 1), "tstar_jpeg_reconstruct_host")
    rc, got = SU.reconstruct_host(geom, coef, quant, 1, threads=2)
    assert rc == 0 and np.array_equal(got, want)
    assert SU.sizes(geom, 1) == (0, W, H, jpeg._sizes(geom)[1], 1)
    assert jpeg.scaled_sizes(geom, 1) == (W, H, jpeg._sizes(geom)[1], True)


def test_bad_arguments_are_refused_before_anything_is_written():
    from tstar_amd import _lib
    lib = _lib.load()
    W, H = 40, 24
    geom, coef, quant = SU.coefficients([JU.encode(SU.picture("noise", W, H), "422", 75)])
    for s in (0, 3, 5, 16, -2):
        rc, out = SU.reconstruct_host(geom, coef, quant, 8)            # a buffer of some size; the call below names the bad scale
        out[:] = 0xA5
        rc = lib.tstar_jpeg_reconstruct_scaled_host(coef.ctypes.data, quant.ctypes.data, 1, *geom, s, out.ctypes.data, 1)
        assert rc == 1 and (out == 0xA5).all(), s
        assert SU.sizes(geom, s)[0] == 1, s
    out = np.full((1, 12, 20, 3), 0xA5, dtype=np.uint8)
    for args in ((None, quant.ctypes.data, 1, out.ctypes.data), (coef.ctypes.data, None, 1, out.ctypes.data),
                 (coef.ctypes.data, quant.ctypes.data, 1, None), (coef.ctypes.data, quant.ctypes.data, 0, out.ctypes.data)):
        rc = lib.tstar_jpeg_reconstruct_scaled_host(args[0], args[1], args[2], *geom, 2, args[3], 1)
        assert rc == 1 and (out == 0xA5).all()
    assert lib.tstar_jpeg_sizes_scaled(*geom, 2, None) == 1
    assert SU.sizes((W, H, 2, 1, 1), 2)[0] == 1 and SU.sizes((W, H, 3, 2, 2), 2)[:3] == (0, 20, 12)
    assert SU.sizes((4, 4, 3, 2, 2), 2)[0] == 1                        # refused at full size: refused here
    # a geometry that is not covered at the scale (4:2:2, chroma row of 2): refused with the fill untouched
    g8, c8, q8 = SU.coefficients([JU.encode(SU.picture("noise", 8, 8), "422", 75)])
    rc, out = SU.reconstruct_host(g8, c8, q8, 2)
    assert rc == 1 and (out == 0xA5).all()


# ------------------------------------------------------------------------------------------------ open_video
def _frames(W=77, H=45, n=6, sampling="420"):
    return [JU.encode(SU.picture(SU.KINDS[i % 3], W, H, seed=i), sampling, 80) for i in range(n)]


@pytest.mark.parametrize("s", SU.SCALES)
@pytest.mark.parametrize("sampling", SU.SAMPLINGS)
def test_open_video_on_the_cpu_gives_pillows_draft(tmp_path, sampling, s):
    """A folder and a list, chunked: [n, oh, ow, 3] of Pillow's draft; the store says what it is."""
    _need_turbo()
    from tstar_amd.video import open_video
    W, H = 77, 45
    datas = _frames(W, H, 6, sampling)
    want = np.stack([SU.pillow_draft(d, s) for d in datas])
    st = open_video(datas, device="cpu", jpeg_scale=s)
    assert tuple(st.frames.shape) == (6, SU.ceil_div(H, s), SU.ceil_div(W, s), 3) and st.shape == tuple(st.frames.shape)
    assert np.array_equal(st.frames.numpy(), want)
    assert (st.jpeg_scale, st.source_size) == (s, (W, H))
    assert st.decode_stats == {"device": 0, "host": 6, "pillow": 0} and st.entropy_stats == {"device": 0, "host": 6}
    for i, d in enumerate(datas):
        (tmp_path / f"f{i}.jpg").write_bytes(d)
    st = open_video(str(tmp_path), device="cpu", jpeg_scale=s)
    assert np.array_equal(st.frames.numpy(), want)


@pytest.mark.parametrize("s", SU.SCALES)
def test_open_video_mixes_pillow_frames_into_a_uniform_store(s):
    """Baseline frames, a progressive one (in front: the prelude; and behind) and a CMYK one: Pillow's draft serves them at the same
    scale, the store is one tensor, decode_stats counts them."""
    _need_turbo()
    from PIL import Image
    from tstar_amd.video import open_video
    W, H = 77, 45
    pics = [SU.picture(SU.KINDS[i % 3], W, H, seed=10 + i) for i in range(7)]
    b = io.BytesIO()
    Image.fromarray(pics[4]).convert("CMYK").save(b, "JPEG", quality=80)
    datas = [JU.encode(pics[0], "420", 80, progressive=True), JU.encode(pics[1], "420", 80), JU.encode(pics[2], "420", 80, "restart"),
             JU.encode(pics[3], "420", 80, progressive=True), b.getvalue(), JU.encode(pics[5], "444", 80), JU.encode(pics[6], "420", 80, "optimize")]
    want = np.stack([SU.pillow_draft(d, s) for d in datas])
    st = open_video(datas, device="cpu", jpeg_scale=s)
    assert np.array_equal(st.frames.numpy(), want)
    assert st.decode_stats == {"device": 0, "host": 3, "pillow": 4}     # the 4:4:4 frame is not of the batch's geometry: Pillow's too
    assert (st.jpeg_scale, st.source_size) == (s, (W, H))


def test_open_video_sends_a_geometry_that_is_uncovered_at_the_scale_to_pillow():
    _need_turbo()
    from tstar_amd.video import open_video
    datas = [JU.encode(SU.picture(SU.KINDS[i % 3], 16, 16, seed=i), "422", 80) for i in range(3)]
    st = open_video(datas, device="cpu", jpeg_scale=4)
    assert st.decode_stats == {"device": 0, "host": 0, "pillow": 3}
    assert np.array_equal(st.frames.numpy(), np.stack([SU.pillow_draft(d, 4) for d in datas]))
    assert open_video(datas, device="cpu", jpeg_scale=8).decode_stats == {"device": 0, "host": 3, "pillow": 0}


def test_open_video_refusals_speak_of_the_files_own_size():
    from tstar_amd.video import open_video
    datas = _frames(77, 45, 4)
    other = JU.encode(SU.picture("noise", 77, 48), "420", 80)
    for pos, odd in ((2, other), (1, JU.encode(SU.picture("noise", 77, 48), "420", 80, progressive=True))):
        frames = list(datas)
        frames[pos] = odd
        with pytest.raises(ValueError, match=rf"Cannot open video file: <jpeg list>\[{pos}\] is 77x48, the first frame is 77x45"):
            open_video(frames, device="cpu", jpeg_scale=4)
    narrow = [JU.encode(SU.picture("noise", 5, 40), "444", 80)] * 2
    with pytest.raises(ValueError, match=r"Cannot open video file: <jpeg list>\[0\] is 5x40: jpeg_scale=8 needs"):
        open_video(narrow, device="cpu", jpeg_scale=8)
    assert tuple(open_video(narrow, device="cpu", jpeg_scale=4).frames.shape) == (2, 10, 2, 3)
    prog = [JU.encode(SU.picture("noise", 5, 40), "444", 80, progressive=True)] * 2
    with pytest.raises(ValueError, match=r"Cannot open video file: <jpeg list>\[0\] is 5x40: jpeg_scale=8 needs"):
        open_video(prog, device="cpu", jpeg_scale=8)


def test_keyword_variable_and_default(monkeypatch, tmp_path):
    _need_turbo()
    from tstar_amd import jpeg
    from tstar_amd.video import open_video
    datas = _frames(40, 24, 3)
    monkeypatch.delenv("TSTAR_JPEG_SCALE", raising=False)
    plain = open_video(datas, device="cpu")
    assert (plain.jpeg_scale, plain.source_size) == (1, (40, 24))
    assert np.array_equal(plain.frames.numpy(), np.stack([JU.pillow_rgb(d) for d in datas]))     # no keyword: the store as it always was
    assert np.array_equal(open_video(datas, device="cpu", jpeg_scale=1).frames.numpy(), plain.frames.numpy())
    monkeypatch.setenv("TSTAR_JPEG_SCALE", "4")
    st = open_video(datas, device="cpu")
    assert st.jpeg_scale == 4 and np.array_equal(st.frames.numpy(), np.stack([SU.pillow_draft(d, 4) for d in datas]))
    assert open_video(datas, device="cpu", jpeg_scale=2).jpeg_scale == 2                           # the keyword wins
    # the variable alone leaves a source that is not JPEG as it is; the keyword on it is an error
    # (a .y4m path that does not exist: under the variable it gets as far as the .y4m reader, which names the file)
    y4m = str(tmp_path / "missing.y4m")
    with pytest.raises(ValueError, match=r"^Cannot open video file: .*missing\.y4m$"):
        open_video(y4m, device="cpu")
    with pytest.raises(ValueError, match="jpeg_scale=2 needs a Motion-JPEG"):
        open_video(y4m, device="cpu", jpeg_scale=2)
    synthetic = open_video("synthetic://n=2,h=9,w=16", device="cpu")
    assert tuple(synthetic.frames.shape) == (2, 9, 16, 3) and synthetic.jpeg_scale == 1
    for bad in ("3", "x", "0", "16"):
        monkeypatch.setenv("TSTAR_JPEG_SCALE", bad)
        with pytest.raises(ValueError, match="jpeg_scale="):
            open_video(datas, device="cpu")
    monkeypatch.delenv("TSTAR_JPEG_SCALE")
    for bad in (3, 0, -2, 16, 2.5, "x"):
        with pytest.raises(ValueError, match="jpeg_scale="):
            open_video(datas, device="cpu", jpeg_scale=bad)
    assert jpeg.scale_mode() == 1 and jpeg.scale_mode(8) == 8


# ------------------------------------------------------------------------------------------------ sanitizers
def test_host_twin_under_address_and_ub_sanitizers(tmp_path):
    """csrc/jpeg_scale_check_main.cpp with the host stage, built with -fsanitize=address,undefined (a stand-alone CPU program; nothing
    is loaded into python, nothing of the GPU is involved), over the edge sizes in every sampling with buffers of exactly the stated
    sizes.  The hashes it prints are those of Pillow's draft."""
    _need_turbo()
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_scale_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_host.cpp"), os.path.join(csrc, "jpeg_scale_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files, expect = [], []
    for (W, H) in SU.SIZES:
        for sampling in SU.SAMPLINGS:
            data = JU.encode(SU.picture("noise", W, H), sampling, 75)
            p = tmp_path / f"{W}x{H}_{sampling}.jpg"
            p.write_bytes(data)
            files.append(str(p))
            for s in SU.SCALES:
                if SU.covered(W, sampling, s):
                    h = 1469598103934665603
                    for v in SU.pillow_draft(data, s).tobytes():
                        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
                    expect.append(f"{p} scale={s} covered=1 size={SU.ceil_div(W, s)}x{SU.ceil_div(H, s)} same=1 fnv={h:016x}")
                else:
                    expect.append(f"{p} scale={s} covered=0 refused=1")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines() == expect
