"""GPU: the split entropy path on the device -- tstar_jpeg_entropy_split_device == its host mirror word for word (coefficients,
statuses, seg_info round for round), hence the sequential host decoder; the reconstructed RGB == Pillow (libjpeg-turbo) byte
for byte; sentinel tails, wave and workgroup edges, refused arguments, broken streams, and open_video in device mode."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402
import test_jpeg_split_host as SH  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (17, 33), (97, 301)]
GUARD = 4096
COEF_SENTINEL, WORD_SENTINEL, RGB_SENTINEL, WS_SENTINEL = 0x7FC0, 0x7FC00000, 0xA5, 0x5A


def _need_turbo():
    if not JU.turbo():
        pytest.skip("Pillow on this machine is not built on libjpeg-turbo: its bytes are not the yardstick the byte-equality "
                    "is defined against (the comparison is not loosened instead)")


def device_split(datas, geom, sub_bytes, min_split_bytes, max_rounds=None, reconstruct=False):
    """One upload, one call; coefficients, statuses, seg_info and the workspace have sentinel tails that must come back untouched,
    and the upload must come back as it went.  -> (plan, coef int16 [n, blocks * 64], seg_status, seg_info, rgb or None)."""
    import torch
    from tstar_amd import _lib, jpeg
    lib = _lib.load()
    batch = jpeg.DeviceBatch(datas, geom)
    n, nseg = len(datas), len(batch.plan.segments)
    assert nseg > 0
    if max_rounds is None:
        max_rounds = SH.enough_rounds(batch.plan, sub_bytes)
    blocks, plane_bytes = jpeg._sizes(geom)
    host = np.zeros(batch.nbytes, dtype=np.uint8)
    batch.fill(host)
    d_buf = torch.from_numpy(host).cuda()
    ws_bytes = jpeg.split_workspace_bytes(batch.total, nseg, sub_bytes)
    d_coef = torch.full((n * blocks * 64 + GUARD,), COEF_SENTINEL, dtype=torch.int16, device="cuda")
    d_status = torch.full((nseg + GUARD,), WORD_SENTINEL, dtype=torch.int32, device="cuda")
    d_info = torch.full((nseg + GUARD,), WORD_SENTINEL, dtype=torch.int32, device="cuda")
    d_ws = torch.full((ws_bytes + GUARD,), WS_SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_ws.data_ptr() % 8 == 0
    base, parts = d_buf.data_ptr(), batch.parts
    _lib.check(lib.tstar_jpeg_entropy_split_device(
        base, batch.total, base + parts["segments"][0], base + parts["table_sets"][0], len(batch.plan.table_sets), base + parts["frames"][0],
        n, nseg, *geom, sub_bytes, min_split_bytes, max_rounds, d_ws.data_ptr(), ws_bytes, d_coef.data_ptr(), d_status.data_ptr(),
        d_info.data_ptr(), _lib.stream_ptr()), "tstar_jpeg_entropy_split_device")
    rgb = None
    if reconstruct:
        W, H = geom[0], geom[1]
        d_planes = torch.empty(n * plane_bytes, dtype=torch.uint8, device="cuda")
        d_rgb = torch.full((n * H * W * 3 + GUARD,), RGB_SENTINEL, dtype=torch.uint8, device="cuda")
        _lib.check(lib.tstar_jpeg_reconstruct(d_coef.data_ptr(), base + parts["quant"][0], n, *geom, d_planes.data_ptr(),
                                              d_rgb.data_ptr(), _lib.stream_ptr()), "tstar_jpeg_reconstruct")
        out = d_rgb.cpu().numpy()
        assert (out[-GUARD:] == RGB_SENTINEL).all()
        rgb = out[:-GUARD].reshape(n, H, W, 3)
    torch.cuda.synchronize()
    coef, status, info, ws = d_coef.cpu().numpy(), d_status.cpu().numpy(), d_info.cpu().numpy(), d_ws.cpu().numpy()
    assert (coef[-GUARD:] == COEF_SENTINEL).all(), "a kernel wrote behind the coefficient buffer"
    assert (status[-GUARD:] == WORD_SENTINEL).all(), "a kernel wrote behind the status array"
    assert (info[-GUARD:] == WORD_SENTINEL).all(), "a kernel wrote behind seg_info"
    assert (ws[-GUARD:] == WS_SENTINEL).all(), "a kernel wrote behind the workspace"
    assert np.array_equal(d_buf.cpu().numpy(), host), "a kernel wrote into its input"
    return batch.plan, coef[:-GUARD].reshape(n, blocks * 64), status[:nseg], info[:nseg], rgb


def check_against_mirror(datas, geom, sub_bytes, min_split_bytes, max_rounds=None, reconstruct=False):
    """The device call and the host mirror on the same bytes with the same arguments: the same words."""
    plan, coef, seg_status, info, rgb = device_split(datas, geom, sub_bytes, min_split_bytes, max_rounds, reconstruct)
    _, m_coef, m_status, m_info = SH.split_decode(datas, geom, sub_bytes, min_split_bytes, max_rounds, plan=plan)
    assert np.array_equal(info, m_info), "seg_info differs from the host mirror's"
    assert np.array_equal(seg_status, m_status)
    ok = plan.frame_status(m_status) == 0
    assert np.array_equal(coef[ok], m_coef[ok])
    return plan, coef, seg_status, info, rgb


@pytest.mark.parametrize("sub", [0, 2], ids=["smallest", "default"])
@pytest.mark.parametrize("sampling", JU.SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_split_equals_the_mirror_the_host_decoder_and_pillow(size, sampling, sub):
    """The host test's matrix cell by cell: {synthetic, noise} x {default, optimised, restart tables} x qualities {30, 100}."""
    from tstar_amd import jpeg
    _need_turbo()
    sub_bytes = SH.sub_sizes()[sub]
    H, W = size
    datas = [d for q in SH.QUALITIES for _, d in JU.matrix_files(H, W, sampling, q)]
    geom = jpeg.probe(datas[0])[1]
    want_c, want_q, want_s = SH.host_decode(datas, geom)
    assert not want_s.any()
    plan, coef, seg_status, info, rgb = check_against_mirror(datas, geom, sub_bytes, 64, reconstruct=True)
    assert not seg_status.any() and np.array_equal(plan.quant, want_q)
    bad = np.nonzero((coef != want_c).any(axis=1))[0]
    assert len(bad) == 0, f"frames {bad.tolist()} differ from the host decoder's coefficients"
    SH.check_info(plan, info, 64)
    for i, d in enumerate(datas):
        assert np.array_equal(rgb[i], JU.pillow_rgb(d)), f"frame {i} differs from Pillow"


def test_360x640_frames_split_by_the_default_arguments():
    """The largest size, with the arguments load_jpeg passes: synthetic frames converge in a few rounds; noise at quality 100 (no
    end-of-block codes to fall into step at) does not within SPLIT_MAX_ROUNDS and is decoded by one lane, in the same call."""
    from tstar_amd import jpeg
    _need_turbo()
    H, W = 360, 640
    datas = [JU.encode(JU.synthetic_picture(H, W, frame=f), "420", 85, t) for f, t in ((3, "default"), (4, "optimize"), (5, "restart"))]
    datas += [JU.encode(JU.noise_picture(H, W, seed=1), "420", 30), JU.encode(JU.noise_picture(H, W, seed=2), "420", 100, "optimize")]
    geom = jpeg.probe(datas[0])[1]
    want_c, want_q, want_s = SH.host_decode(datas, geom)
    assert not want_s.any()
    plan, coef, seg_status, info, rgb = check_against_mirror(datas, geom, jpeg.SPLIT_SUB_BYTES, jpeg.SPLIT_MIN_BYTES, jpeg.SPLIT_MAX_ROUNDS,
                                                             reconstruct=True)
    assert not seg_status.any() and np.array_equal(coef, want_c)
    first = plan.frames["first_segment"]
    assert all(0 < info[first[i]] <= jpeg.SPLIT_MAX_ROUNDS for i in (0, 1, 3)) and info[first[4]] == -1
    assert (info[first[2]:first[3]] == 0).any()                                # restart intervals of three MCUs stay one lane
    for i, d in enumerate(datas):
        assert np.array_equal(rgb[i], JU.pillow_rgb(d)), f"frame {i} differs from Pillow"


def _stream_of(n_sub):
    """A marker-free stream (17x33, or 97x301 for the larger counts) and a sub_bytes (a multiple of 4) that cut it into exactly
    n_sub sub-sequences."""
    from tstar_amd import jpeg
    H, W = (17, 33) if n_sub < 100 else (97, 301)
    for q in range(100, 59, -1):
        for seed in range(12):
            data = JU.encode(JU.noise_picture(H, W, seed=seed), "444", q)
            geom = jpeg.probe(data)[1]
            plan = jpeg.plan_segments([data], geom)
            n = int(SH.seg_lens(plan)[0])
            for sub_bytes in range(8, 132, 4):
                if (n + sub_bytes - 1) // sub_bytes == n_sub:
                    return data, geom, sub_bytes
    raise AssertionError(f"no stream of {n_sub} sub-sequences")


@pytest.mark.parametrize("n_sub", [64, 65, 256, 257])
def test_sub_sequence_counts_at_wave_and_workgroup_edges(n_sub):
    """64 and 65 sub-sequences of one segment: one wave full, and one lane into the next; 256 and 257: the same for the workgroup
    whose waves share one staged table set.  A second, shorter frame behind it puts a segment boundary inside the last wave."""
    from tstar_amd import jpeg
    data, geom, sub_bytes = _stream_of(n_sub)
    other = JU.encode(JU.noise_picture(geom[1], geom[0], seed=999), "444", 75, "optimize")
    datas = [data, other]
    want_c, _, want_s = SH.host_decode(datas, geom)
    assert not want_s.any()
    plan, coef, seg_status, info, _ = check_against_mirror(datas, geom, sub_bytes, 1)
    assert int((SH.seg_lens(plan)[0] + sub_bytes - 1) // sub_bytes) == n_sub and len(plan.table_sets) == 2
    assert not seg_status.any() and (info > 0).all() and np.array_equal(coef, want_c)


def test_broken_streams_equal_the_mirror():
    """The host test's truncated, flipped, stray-byte and loud streams in one call: the statuses of the host mirror (which are
    the sequential decoder's), and its coefficients for every frame that is OK."""
    from tstar_amd import jpeg
    datas = SH.broken_streams()
    geom = jpeg.probe(datas[0])[1]
    want_s = SH.host_decode(datas, geom)[2]
    plan, coef, seg_status, info, _ = check_against_mirror(datas, geom, 64, 64)
    routed = plan.route == jpeg.ROUTE_DEVICE
    got = plan.frame_status(seg_status)
    assert np.array_equal(got[routed], want_s[routed])
    assert {jpeg.OK, jpeg.MALFORMED, jpeg.UNCOVERED} == set(got[routed].tolist())
    SH.check_info(plan, info, 64)


def test_never_split_and_one_round():
    """min_split_bytes = 0 is the one-lane launcher's result with seg_info all 0; max_rounds = 1 abandons what needs more rounds
    and still decodes it."""
    from tstar_amd import jpeg
    datas = [JU.encode(JU.noise_picture(97, 301, seed=11), "420", 75), JU.encode(JU.noise_picture(97, 301, seed=12), "420", 75, "restart")]
    geom = jpeg.probe(datas[0])[1]
    want_c, _, want_s = SH.host_decode(datas, geom)
    plan, coef, seg_status, info, _ = check_against_mirror(datas, geom, 64, 0, max_rounds=4)
    assert not info.any() and not seg_status.any() and np.array_equal(coef, want_c)
    plan, coef, seg_status, info, _ = check_against_mirror(datas, geom, 64, 64, max_rounds=1)
    assert info[0] == -1 and not seg_status.any() and np.array_equal(coef, want_c)


def test_not_cut_kept_and_redone_segments_in_one_launch():
    """The one-lane kernel's two modes side by side: 17x33 frames with min_split_bytes between their lengths, so that in ONE call
    the short ones are not cut (seg_info 0: decoded by one lane), an intact long one converges and is kept (the one-lane kernel
    skips it), and a long one with a corrupted byte converges, is refused by the write pass and decoded again by one lane,
    whose status stands.  The corrupted byte is one after which the sequential decoder says UNCOVERED: the write pass leaves
    MALFORMED for whatever it refuses, so only the redo can have written that status.  Everything equals the host mirror word
    for word."""
    from tstar_amd import jpeg
    H, W = 17, 33
    short = [JU.encode(JU.synthetic_picture(H, W), "420", 30), JU.encode(JU.noise_picture(H, W, seed=4), "420", 75, "restart")]
    long = [JU.encode(JU.noise_picture(H, W, seed=s), "420", 95) for s in (5, 6)]
    geom = jpeg.probe(long[0])[1]
    s0 = JU.segments(long[1])[1]
    broken = None
    for p in range(s0 + (len(long[1]) - 2 - s0) // 2, len(long[1]) - 2):       # the first flip the sequential decoder calls UNCOVERED
        if long[1][p - 1] == 0xFF or long[1][p] == 0xFF or long[1][p] ^ 0x10 == 0xFF:
            continue                                                            # no new marker, no broken FF 00 pair: the plan stays
        m = bytearray(long[1])
        m[p] ^= 0x10
        if SH.host_decode([bytes(m)], geom)[2][0] == jpeg.UNCOVERED:
            broken = bytes(m)
            break
    assert broken is not None
    datas = [short[0], long[0], short[1], broken]
    want_c, _, want_s = SH.host_decode(datas, geom)
    assert want_s[:3].tolist() == [jpeg.OK] * 3 and want_s[3] == jpeg.UNCOVERED != jpeg.MALFORMED
    lens = SH.seg_lens(jpeg.plan_segments(datas, geom))
    min_split = int(lens[[1, -1]].min())
    assert lens[0] < min_split and lens[2:-1].max() < min_split
    plan, coef, seg_status, info, _ = check_against_mirror(datas, geom, 8, min_split)
    assert (plan.route == jpeg.ROUTE_DEVICE).all() and plan.frames["n_segments"].tolist()[::2] == [1, len(lens) - 3]
    SH.check_info(plan, info, min_split)
    assert info[0] == 0 and info[1] > 0 and info[-1] > 0 and not info[2:-1].any()
    assert not seg_status[:-1].any() and seg_status[-1] == jpeg.UNCOVERED      # not cut, kept, not cut ... and the redo's status
    assert np.array_equal(coef[:3], want_c[:3])


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
    need = jpeg.split_workspace_bytes(batch.total, 1, 64)
    d_coef = torch.full((blocks * 64,), COEF_SENTINEL, dtype=torch.int16, device="cuda")
    d_status = torch.full((1,), WORD_SENTINEL, dtype=torch.int32, device="cuda")
    d_info = torch.full((1,), WORD_SENTINEL, dtype=torch.int32, device="cuda")
    d_ws = torch.full((need,), WS_SENTINEL, dtype=torch.uint8, device="cuda")
    base, parts, s = d_buf.data_ptr(), batch.parts, _lib.stream_ptr()
    good = [base, batch.total, base + parts["segments"][0], base + parts["table_sets"][0], 1, base + parts["frames"][0], 1, 1, *geom,
            64, 64, 8, d_ws.data_ptr(), need, d_coef.data_ptr(), d_status.data_ptr(), d_info.data_ptr(), s]
    for at, value in ((0, None), (2, None), (3, None), (5, None), (16, None), (18, None), (19, None), (20, None), (4, 0), (6, 0), (7, 0),
                      (1, 0), (1, 1 << 32), (8, 0), (11, 3), (13, 4), (13, 0), (13, 66), (13, -64), (14, -1), (15, 0), (15, -1),
                      (15, (1 << 16) + 1), (17, need - 1), (17, 0), (16, d_ws.data_ptr() + 4), (2, base + parts["segments"][0] + 1),
                      (20, d_info.data_ptr() + 1)):
        args = list(good)
        args[at] = value
        assert lib.tstar_jpeg_entropy_split_device(*args) == 1, (at, value)
    torch.cuda.synchronize()
    assert (d_coef.cpu().numpy() == COEF_SENTINEL).all() and int(d_status.cpu()[0]) == WORD_SENTINEL      # nothing was launched
    assert int(d_info.cpu()[0]) == WORD_SENTINEL and (d_ws.cpu().numpy() == WS_SENTINEL).all()
    assert lib.tstar_jpeg_entropy_split_device(*good) == 0
    torch.cuda.synchronize()
    assert int(d_status.cpu()[0]) == jpeg.OK and int(d_info.cpu()[0]) > 0


def test_open_video_splits_marker_free_frames(tmp_path, monkeypatch):
    """A 6-frame 97x301 AVI without restart markers: with a small TSTAR_JPEG_SPLIT_BYTES every frame is decoded by many lanes,
    with 0 by one lane as before; both stores are Pillow's bytes."""
    import torch
    from tstar_amd.video import open_video
    _need_turbo()
    monkeypatch.delenv("TSTAR_JPEG_ENTROPY", raising=False)
    H, W = 97, 301
    frames = [JU.encode(JU.synthetic_picture(H, W, frame=i), "420", 85) for i in range(6)]
    path = tmp_path / "clip.avi"
    JU.write_avi(str(path), frames, W, H, rate=1)
    ref = np.stack([JU.pillow_rgb(d) for d in frames])
    monkeypatch.setenv("TSTAR_JPEG_SPLIT_BYTES", "256")
    st = open_video(str(path), jpeg_entropy="device")
    assert st.decode_stats == {"device": 6, "host": 0, "pillow": 0} and st.entropy_stats == {"device": 6, "host": 0}
    assert st.entropy_split_stats["split"] == 6 and st.entropy_split_stats["abandoned"] == 0 and st.entropy_split_stats["rounds_max"] >= 1
    assert list(st.entropy_split_stats) == ["split", "abandoned", "rounds_max"]
    assert np.array_equal(st.frames.cpu().numpy(), ref)
    monkeypatch.setenv("TSTAR_JPEG_SPLIT_BYTES", "0")
    st0 = open_video(str(path), jpeg_entropy="device")
    assert st0.entropy_split_stats == {"split": 0, "abandoned": 0, "rounds_max": 0} and st0.entropy_stats == {"device": 6, "host": 0}
    assert torch.equal(st0.frames, st.frames)
    monkeypatch.delenv("TSTAR_JPEG_SPLIT_BYTES")
    host = open_video(str(path))
    assert host.entropy_split_stats == {"split": 0, "abandoned": 0, "rounds_max": 0} and torch.equal(host.frames, st.frames)
