"""The JPEG encoder's host twin (csrc/jpeg_enc_host.cpp) against Pillow, byte for byte; no GPU needed.

The twin and the kernels share every integer (csrc/jpeg_enc_math.h); tests/test_gpu_jpeg_encode.py pins the kernels against
the twin, this file pins the twin against ``Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=s)``.
"""
import base64
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from jpeg_encode_util import CONTENTS, QUALITIES, SMALL_SIZES, SUBSAMPLINGS, new_counters, picture, pillow_bytes, sos_end


@pytest.mark.parametrize("size", SMALL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_whole_files_equal_pillow(size):
    from tstar_amd import jpeg_encode as JE
    H, W = size
    for content in CONTENTS:
        a = picture(content, H, W)
        for q in QUALITIES:
            for s in SUBSAMPLINGS:
                got = JE.encode_frames(a, q, s, device=False)
                assert len(got) == 1 and got[0] == pillow_bytes(a, q, s), (content, size, q, s)


@pytest.mark.parametrize("quality,subsampling", [(75, "4:2:0"), (100, "4:2:2")])
def test_360x640_equals_pillow(quality, subsampling):
    from tstar_amd import jpeg_encode as JE
    batch = np.stack([picture("noise", 360, 640), picture("smooth", 360, 640)])
    got = JE.encode_frames(batch, quality, subsampling, device=False)
    assert got == [pillow_bytes(a, quality, subsampling) for a in batch]


def test_defaults_are_pillows():
    from PIL import Image
    from tstar_amd import jpeg_encode as JE
    a = picture("smooth", 45, 80)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG")
    assert JE.encode_frames(a, device=False)[0] == buf.getvalue()
    assert JE.encode_frames(a, 75, 2, device=False)[0] == buf.getvalue()          # Pillow's numeric subsampling values
    with pytest.raises(ValueError):
        JE.encode_frames(a, 0, device=False)
    with pytest.raises(ValueError):
        JE.encode_frames(a, 101, device=False)
    with pytest.raises(ValueError):
        JE.encode_frames(a, 75, "4:1:1", device=False)
    with pytest.raises(ValueError):
        JE.encode_frames(a[..., 0], device=False)


def test_the_inputs_reach_every_path():
    """Conditions on the inputs of the tests above, from the twin's counters: each special path of the scan is taken."""
    from tstar_amd import jpeg_encode as JE

    def run(content, H, W, q, s):
        c = new_counters()
        JE.encode_host(picture(content, H, W), q, s, counters=c)
        return dict(zip(JE.COUNTERS, (int(v) for v in c)))

    noise = run("noise", 90, 161, 100, "4:4:4")
    assert noise["stuffed"] > 0 and noise["no_eob"] > 0, noise
    smooth = [run("smooth", H, W, 100, "4:2:0") for H, W in SMALL_SIZES]      # isolated small high-frequency terms behind long zero runs
    assert sum(c["zrl"] for c in smooth) > 0, smooth
    both = run("noise", 24, 40, 75, "4:2:0")          # 3 x 5 real luma blocks inside 4 x 6
    assert both["dummy_right"] == 3 and both["dummy_bottom"] == 6, both
    right = run("noise", 16, 24, 75, "4:2:2")         # 3 luma blocks per row inside 4, no dummy row
    assert right["dummy_right"] == 2 and right["dummy_bottom"] == 0, right
    assert pillow_bytes(picture("noise", 16, 24), 75, "4:2:2") == JE.encode_frames(picture("noise", 16, 24), 75, "4:2:2", device=False)[0]
    none = run("noise", 16, 16, 75, "4:2:0")
    assert none["dummy_right"] == 0 and none["dummy_bottom"] == 0, none


@pytest.mark.parametrize("size", [(17, 23), (24, 40), (33, 7), (90, 161)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_two_stages_separately(size):
    """Block stage == what the project's decoder reads out of Pillow's file (coefficients in the MCU-padded layout, dummy blocks
    included, and tables); scan stage fed the DECODED coefficients == Pillow's entropy-coded bytes."""
    from tstar_amd import jpeg
    from tstar_amd import jpeg_encode as JE
    H, W = size
    for content in ("noise", "smooth"):
        a = picture(content, H, W)
        for q in (5, 75, 100):
            for s in SUBSAMPLINGS:
                hs, vs = JE.sampling(s)
                ref = pillow_bytes(a, q, s)
                geom = (W, H, 3, hs, vs)
                blocks = JE.Plan(W, H, hs, vs).blocks
                dcoef = np.zeros((1, blocks * 64), dtype=np.int16)
                dquant = np.zeros((1, 192), dtype=np.uint16)
                status, msg = jpeg.entropy_batch([ref], geom, dcoef, dquant)
                assert status[0] == 0, msg
                coef, quant = JE.blocks_host(a, q, s)
                assert np.array_equal(quant.reshape(-1), dquant[0]), (content, size, q, s)
                assert np.array_equal(coef, dcoef), (content, size, q, s)
                scans, lengths, st = JE.scan_host(dcoef, W, H, s)
                assert st[0] == 0 and scans[0] == ref[sos_end(ref):] and lengths[0] == len(scans[0]), (content, size, q, s)


def test_scan_stage_refuses_coefficients_no_jpeg_can_code():
    from tstar_amd import jpeg_encode as JE
    blocks = JE.Plan(8, 8, 1, 1).blocks
    coef = np.zeros((1, blocks * 64), dtype=np.int16)
    coef[0, 5] = 1024                                  # an AC value of category 11
    scans, lengths, st = JE.scan_host(coef, 8, 8, "4:4:4")
    assert st[0] == JE.STATUS_BAD_COEF and scans[0] is None


@pytest.mark.parametrize("size", SMALL_SIZES + [(360, 640)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_header_equals_pillow(size):
    from tstar_amd import jpeg_encode as JE
    H, W = size
    a = picture("black", H, W)
    for q in QUALITIES:
        for s in SUBSAMPLINGS:
            ref = pillow_bytes(a, q, s)
            head = JE.header(W, H, q, s)
            assert head == ref[:sos_end(ref)], (size, q, s)
            assert len(head) == JE.Plan(W, H, *JE.sampling(s)).header_bytes


def test_capacity_exact_and_one_short():
    from tstar_amd import jpeg_encode as JE
    for content, H, W, q, s in (("noise", 33, 7, 100, "4:2:0"), ("smooth", 45, 80, 75, "4:2:2"), ("black", 1, 1, 75, "4:4:4")):
        a = picture(content, H, W)
        ref = pillow_bytes(a, q, s)
        L, pad = len(ref), 64
        for cap, want in ((L, JE.STATUS_OK), (L - 1, JE.STATUS_SHORT), (0, JE.STATUS_SHORT)):
            buf = np.full(L + pad, 0xA5, dtype=np.uint8)
            out, lengths, status = JE.encode_host(a, q, s, slot_bytes=cap, out=buf)
            assert status[0] == want and lengths[0] == L, (content, cap)
            if want == JE.STATUS_OK:
                assert buf[:L].tobytes() == ref
                assert (buf[L:] == 0xA5).all()
            else:
                assert (buf == 0xA5).all()            # a short slot is left as it was, and so is the canary behind it
        # the scan stage alone, two frames in slots back to back: the slot of the second starts where the first's capacity ends
        coef, _ = JE.blocks_host(np.stack([a, a]), q, s)
        scan_len = L - 623
        scans, lengths, status = JE.scan_host(coef, W, H, s, slot_bytes=scan_len)
        assert list(status) == [0, 0] and scans[0] == scans[1] == ref[623:]
        scans, lengths, status = JE.scan_host(coef, W, H, s, slot_bytes=scan_len - 1)
        assert list(status) == [1, 1] and list(lengths) == [scan_len, scan_len]


def test_plan_is_pure_and_refuses_by_name():
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    p = JE.Plan(640, 360, 2, 2, 4, 4096)
    assert p.blocks == 40 * 23 * 6 and p.coef_bytes == p.blocks * 128 and p.header_bytes == 623
    assert p.max_scan_bytes == 2 * ((p.blocks * 1660 + 7) // 8) + 2
    assert p.block_wgs == (4 * p.blocks + 31) // 32 and p.entropy_wgs_x == (p.blocks + 255) // 256
    # the unstuffed stream is never larger than the slot, so the workspace follows the slot, not the bound
    assert p.workspace_bytes < 4 * (p.blocks * 4 + 4096 + 4096 // 16 + 256) + 1024
    for args, word in (((640, 360, 2, 2, 0, 4096), "n must"), ((640, 360, 1, 2, 1, 4096), "geometry"), ((640, 360, 2, 2, 1, 1), "slot_bytes"),
                       ((0, 360, 2, 2, 1, 4096), "geometry"), ((16384, 16384, 1, 1, 1, 4096), "too large")):
        with pytest.raises(_lib.TStarHipError, match=word):
            JE.Plan(*args)


def test_frames_to_base64_is_the_reference_statement():
    from PIL import Image
    from tstar_amd import jpeg_encode as JE
    a = picture("smooth", 90, 161)
    # TStar/utilites.py:28-35
    buffered = io.BytesIO()
    Image.fromarray(a).save(buffered, format="JPEG")
    want = base64.b64encode(buffered.getvalue()).decode("utf-8")
    assert JE.frames_to_base64(a[None]) == [want]


def test_container_round_trip_on_the_host(tmp_path):
    from tstar_amd import jpeg
    from tstar_amd import jpeg_encode as JE
    frames = np.stack([picture("smooth", 45, 80), picture("noise", 45, 80), picture("black", 45, 80)])
    files = JE.encode_frames(frames, 90, "4:2:0", device=False)
    assert files == [pillow_bytes(a, 90) for a in frames]
    for name, fps in (("a.avi", None), ("b.avi", 2.5), ("c.avi", 30000 / 1001)):
        path = str(tmp_path / name)
        assert JE.save_mjpeg(frames, path, quality=90, fps=fps, device=False) == 3
        assert os.path.getsize(path) == JE.avi_bytes([len(f) for f in files])
        src = jpeg.avi_mjpeg(path)
        try:
            assert src.n_frames == 3 and [bytes(src.read(i)) for i in range(3)] == files
            assert abs(src.fps - (1.0 if fps is None else fps)) < 1e-6
        finally:
            src.close()
    path = str(tmp_path / "d.mjpeg")
    JE.save_mjpeg(frames, path, quality=90, device=False)
    src = jpeg.mjpeg_stream(path, fps=1.0)
    try:
        assert src.n_frames == 3 and [bytes(src.read(i)) for i in range(3)] == files
    finally:
        src.close()
    with pytest.raises(ValueError, match="expected .avi"):
        JE.save_mjpeg(frames, str(tmp_path / "e.mp4"), device=False)


def test_avi_that_would_need_opendml_is_refused_by_name():
    from tstar_amd import jpeg_encode as JE
    lens = [300_000] * 3600                            # 3 600 frames of 300 kB: just over 1 GiB
    assert JE.avi_bytes(lens) >= JE.AVI_LIMIT
    with pytest.raises(ValueError, match=r"OpenDML.*\.mjpeg"):
        JE.check_avi_size(lens, "big.avi")
    with pytest.raises(ValueError, match=r"\.mjpeg"):
        JE.write_avi("/nonexistent/never_opened.avi", _Sized(lens), 640, 360)
    assert JE.check_avi_size([290_000] * 3600) < JE.AVI_LIMIT


class _Sized(list):
    """Stand-ins with a length and no bytes: the size check comes before the file is opened."""

    def __init__(self, lens):
        super().__init__(_Len(n) for n in lens)


class _Len:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_host_twin_under_address_and_ub_sanitizers(tmp_path):
    """The twin built with -fsanitize=address,undefined (CPU build; nothing of the GPU is involved) and driven by
    csrc/jpeg_enc_check_main.cpp over case files at exact, short and zero capacities.  Any out-of-bounds access or undefined
    operation aborts the tool."""
    gxx = os.environ.get("CXX") or shutil.which("g++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "tstar_amd", "csrc")
    exe = str(tmp_path / "jpeg_enc_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-pthread",
           os.path.join(csrc, "jpeg_enc_host.cpp"), os.path.join(csrc, "jpeg_host.cpp"), os.path.join(csrc, "jpeg_enc_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = [("noise", 1, 1, 75, 2, 2), ("noise", 1, 9, 100, 2, 2), ("noise", 19, 1, 100, 2, 1), ("noise", 24, 40, 100, 2, 2),
             ("smooth", 33, 7, 5, 2, 2), ("smooth", 45, 80, 75, 2, 1), ("noise", 17, 23, 100, 1, 1), ("white", 16, 16, 95, 2, 2)]
    files = []
    for k, (content, H, W, q, hs, vs) in enumerate(cases):
        p = tmp_path / f"case{k}.bin"
        p.write_bytes(struct.pack("<5i", W, H, q, hs, vs) + picture(content, H, W).tobytes())
        files.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files) and all(" ok=1 " in ln for ln in lines), r.stdout


def test_surface():
    from tstar_amd import _lib, build
    new = {"tstar_jpeg_encode_plan", "tstar_jpeg_encode_header", "tstar_jpeg_encode_blocks", "tstar_jpeg_encode_blocks_host",
           "tstar_jpeg_encode_scan", "tstar_jpeg_encode_scan_host", "tstar_jpeg_encode", "tstar_jpeg_encode_host"}
    with open(os.path.join(ROOT, "include", "tstar_hip.h")) as f:
        declared = set(re.findall(r"\b(tstar_[a-z0-9_]+)\s*\(", f.read()))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in new:
        assert hasattr(lib, name)
    assert lib.tstar_abi_version() == 3
    assert "jpeg_enc.hip" in build.sources() and "jpeg_enc_host.cpp" in build.sources()
    from tstar_amd.video import FrameStore
    assert callable(FrameStore.jpeg_frames) and callable(FrameStore.save_mjpeg)
