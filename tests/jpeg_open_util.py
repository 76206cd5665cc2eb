"""What the CPU and the GPU tests of the JPEG open share: a ten-frame list that walks every rung of the open's ladder, the
defects every opener must refuse with one text, and a planner patch that reports a good frame refused."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402

H, W, N, QUALITY = 72, 128, 10, 85
CHUNKS = (None, 3)
# of frames 2 .. 9, the ones behind the prelude: the planner's route and the host entropy decoder's status
ROUTES = [0, 1, 0, 0, 0, 0, 1, 0]
HOST_STATUS = [0, 3, 2, 0, 0, 0, 2, 0]
PILLOW_FRAMES = (0, 1, 3, 4, 8)
REFUSED_GOOD_FRAME = 5              # a good, device-routed frame that refuse_frame() reports as not OK
NAME = "<jpeg list>"


@functools.lru_cache(maxsize=None)
def pictures(h=H, w=W):
    """The first ten frames of a synthetic video; a height the video cannot have (80) is cropped from the next one it can."""
    from tstar_amd.video import synthetic_frames_numpy
    return np.ascontiguousarray(synthetic_frames_numpy(range(N), 95, -(-h // 9) * 9, w, seed=7)[:, :h])


def _enc(i, sampling="420", tables="default", progressive=False, h=H, w=W):
    return JU.encode(pictures(h, w)[i], sampling, QUALITY, tables, progressive)


@functools.lru_cache(maxsize=None)
def ladder():
    """Frames 0, 1 progressive (the prelude: no covered frame yet); 2 fixes the geometry; 3 is 4:4:4 (GEOMETRY, same size: Pillow's);
    4 carries three stray bytes in front of EOI (device-routed, refused by the decode core); 5 optimized tables; 6, 9 restart-coded;
    7 default tables; 8 progressive (host-routed)."""
    junk = _enc(4)
    assert junk[-2:] == b"\xff\xd9"
    return (_enc(0, progressive=True), _enc(1, progressive=True), _enc(2), _enc(3, "444"), junk[:-2] + b"\x12\x34\x56" + junk[-2:],
            _enc(5, tables="optimize"), _enc(6, tables="restart"), _enc(7), _enc(8, progressive=True), _enc(9, tables="restart"))


@functools.lru_cache(maxsize=None)
def ladder_pixels():
    """Pillow's decode of every frame of the ladder, uint8 [10,72,128,3] (computed once, never written)."""
    out = np.stack([JU.pillow_rgb(d) for d in ladder()])
    out.setflags(write=False)
    return out


def _with(pos, data):
    out = list(ladder())
    out[pos] = data
    return out


HUFFMAN = "bad Huffman code or data ends inside an AC code"
PROBE = "tstar_jpeg_probe: segment length runs past the end of the data"


def _size(pos):
    return f"Cannot open video file: {NAME}[{pos}] is {W}x80, the first frame is {W}x{H}"


def _why(pos, why):
    return f"Cannot open video file: {NAME}[{pos}] ({why})"


DEFECTS = ("frame 6 cut to half its bytes", "frame 7 is a covered 80 x 128 frame", "frame 7 is a progressive 80 x 128 frame",
           "the list opens with a covered frame cut to 200 bytes", "a cut frame at 1 behind a progressive frame 0",
           "a progressive frame of another size at 1", "a covered frame of another size at 1")


@functools.lru_cache(maxsize=None)
def defects():
    """name (DEFECTS) -> (frames, the text every opener refuses them with)."""
    good = ladder()
    return {
        "frame 6 cut to half its bytes": (_with(6, good[6][:len(good[6]) // 2]), _why(6, HUFFMAN)),
        "frame 7 is a covered 80 x 128 frame": (_with(7, _enc(7, h=80)), _size(7)),
        "frame 7 is a progressive 80 x 128 frame": (_with(7, _enc(7, progressive=True, h=80)), _size(7)),
        "the list opens with a covered frame cut to 200 bytes": (_with(0, good[2][:200]), _why(0, PROBE)),
        "a cut frame at 1 behind a progressive frame 0": (_with(1, good[2][:200]), _why(1, PROBE)),
        "a progressive frame of another size at 1": (_with(1, _enc(1, progressive=True, h=80)), _size(1)),
        "a covered frame of another size at 1": (_with(1, _enc(1, h=80)), _size(1)),
    }


def source(frames=None):
    from tstar_amd import jpeg
    return jpeg.JpegList(list(ladder() if frames is None else frames), fps=1.0, name=NAME)


def refuse_frame(monkeypatch, frame=REFUSED_GOOD_FRAME, first_planned=2):
    """Make SegmentPlan.frame_status report list frame ``frame`` as UNCOVERED.  Plans come in list order from ``first_planned`` on
    (the frame that fixed the geometry), so the frames planned before a call are counted here."""
    from tstar_amd import jpeg
    real = jpeg.SegmentPlan.frame_status
    seen = [first_planned]

    def frame_status(self, seg_status):
        out = real(self, seg_status)
        j = frame - seen[0]
        seen[0] += len(self.route)
        if 0 <= j < len(out):
            assert out[j] == jpeg.OK
            out[j] = jpeg.UNCOVERED
        return out

    monkeypatch.setattr(jpeg.SegmentPlan, "frame_status", frame_status)
