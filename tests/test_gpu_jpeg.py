"""GPU: the JPEG decode front end on the device -- kernels == Pillow (libjpeg-turbo) == host path, byte for byte; chunking;
the three containers; the searcher over a decoded AVI."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402

QUALITIES, SAMPLINGS, SIZES = JU.QUALITIES, JU.SAMPLINGS, JU.SIZES

pytestmark = pytest.mark.gpu


def _need_turbo():
    if not JU.turbo():
        pytest.skip("Pillow on this machine is not built on libjpeg-turbo: its bytes are not the yardstick the byte-equality "
                    "is defined against (the comparison is not loosened instead)")


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_path_equals_pillow_and_host(size, sampling, quality):
    """The CPU matrix on the device: {synthetic, noise} x {default tables, optimised tables, restart interval} of one
    geometry form one chunked batch (chunk 3: ten frames = three full chunks and a partial one; at the odd sizes every second
    chunk starts at a store address that is not a multiple of four)."""
    from tstar_amd import jpeg
    _need_turbo()
    H, W = size
    files = JU.matrix_files(H, W, sampling, quality)
    datas = [d for _, d in files] + [JU.strip_dht(d) for lab, d in files if not lab.endswith("optimize")]
    st = jpeg.load_jpeg(jpeg.JpegList(datas), device="cuda", chunk=3)
    assert st.decode_stats == {"device": len(datas), "host": 0, "pillow": 0}
    got = st.frames.cpu().numpy()
    host = jpeg.decode_host(datas)
    for i, d in enumerate(datas):
        ref = JU.pillow_rgb(d)
        assert np.array_equal(host[i], ref), f"frame {i}: host path != Pillow"
        diff = np.nonzero(got[i] != ref)
        assert len(diff[0]) == 0, f"frame {i}: {len(diff[0])} bytes differ from Pillow, first at {[int(a[0]) for a in diff]}"


@pytest.mark.parametrize("n", [1, 2, 3, 4, 9])
def test_chunk_edges(n):
    """Chunk 3: n = 1, chunk - 1, chunk, chunk + 1 and three chunks, at an odd size (33x17: a frame is 1683 bytes, so every
    second chunk starts at an address that is not a multiple of four and takes the byte-store form of the colour kernel)
    and at an even one."""
    from tstar_amd import jpeg
    _need_turbo()
    datas = [JU.encode(JU.noise_picture(33, 17, seed=i), "420", 75) for i in range(n)]
    st = jpeg.load_jpeg(jpeg.JpegList(datas), device="cuda", chunk=3)
    assert st.frames.shape == (n, 33, 17, 3) and st.decode_stats["device"] == n
    assert np.array_equal(st.frames.cpu().numpy(), np.stack([JU.pillow_rgb(d) for d in datas]))
    datas = [JU.encode(JU.synthetic_picture(72, 128, frame=i % 8), "422", 85) for i in range(n)]
    st = jpeg.load_jpeg(jpeg.JpegList(datas), device="cuda", chunk=3)
    assert np.array_equal(st.frames.cpu().numpy(), np.stack([JU.pillow_rgb(d) for d in datas]))


def test_default_chunking_and_fallback_frames_on_the_device():
    from tstar_amd.video import open_video
    _need_turbo()
    pics = [JU.synthetic_picture(360, 640, frame=i % 8) for i in range(70)]
    datas = [JU.encode(p, "420", 85) for p in pics]
    datas[5] = JU.encode(pics[5], "420", 85, progressive=True)
    datas[69] = JU.encode(pics[69], "444", 85)
    st = open_video(datas)
    assert st.decode_stats == {"device": 68, "host": 0, "pillow": 2}
    assert np.array_equal(st.frames.cpu().numpy(), np.stack([JU.pillow_rgb(d) for d in datas]))


@pytest.fixture(scope="module")
def clip120(tmp_path_factory):
    """120 synthetic 72x128 frames as a folder of JPEGs, a .mjpeg stream and a 30 fps AVI (with and without idx1)."""
    from tstar_amd.video import synthetic_frames_numpy
    root = tmp_path_factory.mktemp("clip120")
    frames = synthetic_frames_numpy(range(120), 120, 72, 128, seed=11)
    jpegs = [JU.encode(f, "420", 85) for f in frames]
    folder = root / "frames"
    folder.mkdir()
    for i, d in enumerate(jpegs):
        (folder / f"frame{i}.jpg").write_bytes(d)              # frame2.jpg before frame10.jpg: natural order matters
    JU.write_mjpeg(str(root / "clip.mjpeg"), jpegs)
    JU.write_avi(str(root / "clip.avi"), jpegs, 128, 72, rate=30, index=True)
    JU.write_avi(str(root / "clip_noidx.avi"), [JU.strip_dht(d) for d in jpegs], 128, 72, rate=30, index=False)
    return root, np.stack([JU.pillow_rgb(d) for d in jpegs])


def test_open_video_on_folder_mjpeg_and_avi(clip120):
    from tstar_amd.video import load_video_frames, open_video
    _need_turbo()
    root, ref = clip120
    stores = {"folder": open_video(str(root / "frames"), fps=30.0), "mjpeg": open_video(str(root / "clip.mjpeg"), fps=30.0),
              "avi": open_video(str(root / "clip.avi")), "avi, no idx1, no DHT": open_video(str(root / "clip_noidx.avi"))}
    for name, st in stores.items():
        assert (st.raw_fps, st.raw_total_frames, st.num_seconds) == (30.0, 120, 4), name
        assert st.frames.is_cuda and st.decode_stats == {"device": 4, "host": 0, "pillow": 0}, name
        assert np.array_equal(st.frames.cpu().numpy(), ref[[0, 30, 60, 90]]), name
    # the grounder's 8 uniform frames: raw indices floor(i * 120 / 8), served from the nearest stored second
    raw = [i * 15 for i in range(8)]
    nearest = [min(3, int(round(r / 30.0))) * 30 for r in raw]
    for video, kw in ((str(root / "frames"), dict(fps=30.0)), (str(root / "clip.mjpeg"), dict(fps=30.0)), (str(root / "clip.avi"), {})):
        assert np.array_equal(load_video_frames(video, 8, **kw), ref[nearest]), video
    # a folder at its default rate (one file per logical second) holds every raw frame: the exact 8
    assert np.array_equal(load_video_frames(str(root / "frames"), 8), ref[raw])
    st = open_video(str(root / "clip.mjpeg"))                               # .mjpeg default: 25 fps
    assert (st.raw_fps, st.num_seconds) == (25.0, 4) and np.array_equal(st.frames.cpu().numpy(), ref[[0, 25, 50, 75]])


def test_searcher_over_avi_equals_searcher_over_pillow_frames(tmp_path):
    """Identical pixels in, identical bits out: TStarSearcher over the decoded AVI and over a FrameStore built from the
    Pillow-decoded arrays, same seed -> the same keyframes, timestamps and P_history."""
    import torch
    from tstar_amd.interface_heuristic import OWLInterface
    from tstar_amd.interface_searcher import TStarSearcher
    from tstar_amd.video import FrameStore, synthetic_frames_numpy
    _need_turbo()
    N = 96
    frames = synthetic_frames_numpy(range(N), N, 360, 640, seed=3)
    jpegs = [JU.encode(f, "420", 85) for f in frames]
    path = str(tmp_path / "video.avi")
    JU.write_avi(path, jpegs, 640, 360, rate=1)
    ref = np.stack([JU.pillow_rgb(d) for d in jpegs])
    h = OWLInterface(synthetic_seed=0, max_batch=8, device="cuda:0")
    out = []
    for video in (path, FrameStore(torch.from_numpy(ref).cuda(), 1.0, N, name="pillow")):
        s = TStarSearcher(video, h, ["couch"], ["tv"], search_nframes=4, image_grid_shape=(4, 4), search_budget=0.2,
                          confidence_threshold=0.6, rng=np.random.RandomState(2025), keep_visual_history=False)
        kf, ts = s.search()
        out.append((np.asarray(kf), list(ts), [np.asarray(p) for p in s.P_history], s.store))
    (kf_a, ts_a, ph_a, st_a), (kf_b, ts_b, ph_b, _) = out
    assert st_a.decode_stats == {"device": N, "host": 0, "pillow": 0}
    assert np.array_equal(st_a.frames.cpu().numpy(), ref)
    assert ts_a == ts_b and len(ts_a) == 4
    assert np.array_equal(kf_a, kf_b) and kf_a.shape == (4, 360, 640, 3)
    assert len(ph_a) == len(ph_b) and len(ph_a) > 0
    for a, b in zip(ph_a, ph_b):
        assert np.array_equal(a, b)
