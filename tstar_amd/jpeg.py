"""JPEG decode front end: Motion-JPEG AVI, raw .mjpeg streams, folders / lists of JPEG frames -> the resident store.

Replaces the decode half of read_frame_batch (reference interface_searcher.py:157-169) for intra-only JPEG video.
Only the raw frames the searcher can ever ask for (int(sec * fps) for every logical second, :360) are read from disk.
Each is entropy-decoded on a host thread pool (tstar_jpeg_entropy_batch: serial per scan, so it stays on the CPU) into
pinned memory; dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB run as HIP kernels (tstar_jpeg_reconstruct)
straight into the store, the copy and kernels of one chunk overlapping the entropy decode of the next.  The result is
byte-equal to Pillow / libjpeg-turbo.  Frames the kernels do not cover (progressive, arithmetic, CMYK, unusual sampling)
are decoded by Pillow and copied in; ``FrameStore.decode_stats`` says how many frames went which way.

``entropy="device"`` moves the entropy stage to the GPU as well (tstar_jpeg_plan_segments cuts the frames into restart
segments on the host, tstar_jpeg_entropy_device decodes one segment per lane): the compressed bytes go up instead of the
coefficients, and a frame the device does not vouch for is run through the host decoder again, whose verdict stands.
A frame without restart markers is one segment; the device mode cuts segments of at least TSTAR_JPEG_SPLIT_BYTES bytes into
sub-sequences of SPLIT_SUB_BYTES bytes, one lane each (tstar_jpeg_entropy_split_device: self-synchronising parallel Huffman
decoding), and ``FrameStore.entropy_split_stats`` says how many segments went that way.

``scale`` 2, 4 or 8 (``open_video(..., jpeg_scale=)``, TSTAR_JPEG_SCALE) decodes every frame at 1/2, 1/4 or 1/8 size, byte for byte
Pillow's ``Image.draft``: the entropy stages are the same, the reconstruction runs reduced inverse DCTs
(tstar_jpeg_reconstruct_scaled, tstar_jpeg_reconstruct_scaled_host), and frames that go to Pillow are drafted to the same scale.
"""
from __future__ import annotations

import ctypes as C
import mmap
import os
import re
import struct
from typing import List, Optional, Sequence

import numpy as np

JPEG_EXT = (".jpg", ".jpeg")
MJPEG_EXT = (".mjpeg", ".mjpg")
OK, MALFORMED, UNCOVERED, GEOMETRY = 0, 1, 2, 3


class NotMotionJpeg(ValueError):
    """An AVI whose video stream is another codec: open_video may still hand it to decord / cv2 where a host has them."""


def natural_key(name: str):
    """f2.jpg sorts before f10.jpg: digit runs compare as numbers."""
    return [(0, int(p), "") if p.isdigit() else (1, 0, p.lower()) for p in re.split(r"(\d+)", name) if p]


# ------------------------------------------------------------------------------------------------ sources
class JpegFrames:
    """Random access to the JPEG bytes of a stream's raw frames."""

    def __init__(self, name: str, fps: float, n_frames: int):
        self.name, self.fps, self.n_frames = name, float(fps), int(n_frames)
        if not self.fps > 0:
            raise ValueError(f"Cannot open video file: {name} (frame rate {fps!r} is not positive)")

    def read(self, i: int) -> bytes:
        raise NotImplementedError

    def label(self, i: int) -> str:
        return f"{self.name} frame {i}"

    def close(self) -> None:
        pass


class JpegList(JpegFrames):
    """A list of file paths and / or ``bytes`` objects, one JPEG each."""

    def __init__(self, items: Sequence, fps: float = 1.0, name: str = "<jpeg list>"):
        super().__init__(name, fps, len(items))
        self.items = list(items)

    def read(self, i):
        it = self.items[i]
        if isinstance(it, (bytes, bytearray, memoryview)):
            return bytes(it)
        with open(it, "rb") as f:
            return f.read()

    def label(self, i):
        it = self.items[i]
        return f"{self.name}[{i}]" if isinstance(it, (bytes, bytearray, memoryview)) else str(it)


def jpeg_folder(path: str, fps: float = 1.0) -> JpegList:
    names = sorted((f for f in os.listdir(path) if f.lower().endswith(JPEG_EXT)), key=natural_key)
    if not names:
        raise ValueError(f"Cannot open video file: {path} (the folder holds no .jpg / .jpeg files)")
    return JpegList([os.path.join(path, f) for f in names], fps, name=path)


class _Mapped(JpegFrames):
    """Frames as (offset, size) byte ranges of one memory-mapped file."""

    def __init__(self, path, fps, ranges, fh, mm):
        super().__init__(path, fps, len(ranges))
        self.ranges, self._fh, self._mm = ranges, fh, mm

    def read(self, i):
        off, size = self.ranges[i]
        return self._mm[off:off + size]

    def close(self):
        self._mm.close()
        self._fh.close()


def _map_file(path):
    if not os.path.isfile(path) or os.path.getsize(path) == 0:
        raise ValueError(f"Cannot open video file: {path}")
    fh = open(path, "rb")
    return fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)


def mjpeg_stream(path: str, fps: float = 25.0) -> _Mapped:
    """Concatenated JPEGs.  Frame boundaries come from walking each frame's marker segments and stuffed entropy data
    (tstar_jpeg_frame_end), not from searching for FFD8: thumbnails inside APPn segments carry their own SOI / EOI."""
    from . import _lib
    lib = _lib.load()
    fh, mm = _map_file(path)
    try:
        buf = np.frombuffer(mm, dtype=np.uint8)
        base, size = buf.ctypes.data, len(mm)
        ranges, pos = [], 0
        while pos < size:
            if mm[pos] != 0xFF:                       # padding between frames (some writers align them)
                nxt = mm.find(b"\xff\xd8", pos)
                if nxt < 0 and ranges and not mm[pos:].strip(b"\x00"):
                    break                             # zero padding after the last frame
                if nxt < 0 or mm[pos:nxt].strip(b"\x00"):
                    raise ValueError(f"Cannot open video file: {path} (bytes that are no JPEG at offset {pos})")
                pos = nxt
            end = lib.tstar_jpeg_frame_end(base, size, pos)
            if end == 0:
                raise ValueError(f"Cannot open video file: {path} (frame {len(ranges)} at offset {pos} is broken or truncated)")
            ranges.append((pos, end - pos))
            pos = end
        del buf
        if not ranges:
            raise ValueError(f"Cannot open video file: {path} (no JPEG frame)")
        return _Mapped(path, fps, ranges, fh, mm)
    except Exception:
        try:
            mm.close()
        except BufferError:
            pass
        fh.close()
        raise


def _riff_chunks(mm, start, end):
    """(fourcc, data offset, data size) of the chunks in [start, end); sizes are clipped to the enclosing range."""
    p = start
    while p + 8 <= end:
        cid, size = mm[p:p + 4], struct.unpack_from("<I", mm, p + 4)[0]
        if p + 8 + size > end:
            size = end - p - 8                        # a truncated last chunk: what is there
        yield cid, p + 8, size
        p += 8 + size + (size & 1)


def avi_mjpeg(path: str) -> _Mapped:
    """An AVI (RIFF) file whose video stream is Motion-JPEG.  Rate and stream number from ``strh`` / ``avih``, the frames'
    byte ranges from ``idx1`` when present, else by walking the ``movi`` list.  A zero-length video chunk (a dropped frame)
    repeats the previous one.  OpenDML files (``AVIX`` extension segments, above 1 GiB) are refused by name."""
    fh, mm = _map_file(path)

    def bad(why):
        return ValueError(f"Cannot open video file: {path} ({why})")

    try:
        size = len(mm)
        if size < 12 or mm[0:4] != b"RIFF" or mm[8:12] != b"AVI ":
            raise bad("not a RIFF AVI file")
        riff_end = min(size, 8 + struct.unpack_from("<I", mm, 4)[0])
        if riff_end + 12 <= size and mm[riff_end:riff_end + 4] == b"RIFF" and mm[riff_end + 8:riff_end + 12] == b"AVIX":
            raise bad("OpenDML AVI with AVIX extension segments is not supported")
        usec, vstream, rate, scale, fourcc, movi, idx1, n_streams = 0, None, 0, 0, None, None, None, 0
        for cid, off, sz in _riff_chunks(mm, 12, riff_end):
            if cid == b"LIST" and sz >= 4 and mm[off:off + 4] == b"hdrl":
                for c2, o2, s2 in _riff_chunks(mm, off + 4, off + sz):
                    if c2 == b"avih" and s2 >= 4:
                        usec = struct.unpack_from("<I", mm, o2)[0]
                    elif c2 == b"LIST" and s2 >= 4 and mm[o2:o2 + 4] == b"strl":
                        kind, handler, sc, rt, comp = None, b"", 0, 0, None
                        for c3, o3, s3 in _riff_chunks(mm, o2 + 4, o2 + s2):
                            if c3 == b"strh" and s3 >= 28:
                                kind, handler = mm[o3:o3 + 4], mm[o3 + 4:o3 + 8]
                                sc, rt = struct.unpack_from("<II", mm, o3 + 20)
                            elif c3 == b"strf" and s3 >= 20:
                                comp = mm[o3 + 16:o3 + 20]
                        if kind == b"vids" and vstream is None:
                            vstream, scale, rate, fourcc = n_streams, sc, rt, (comp if comp is not None else handler)
                        n_streams += 1
            elif cid == b"LIST" and sz >= 4 and mm[off:off + 4] == b"movi":
                movi = (off, sz)
            elif cid == b"idx1":
                idx1 = (off, sz)
        if vstream is None or movi is None:
            raise bad("no video stream or no movi list")
        if fourcc.upper() != b"MJPG":
            raise NotMotionJpeg(f"Cannot open video file: {path} (video codec {fourcc.decode('latin-1')!r}: only Motion-JPEG "
                                f"('MJPG') AVI is decoded here)")
        fps = rate / scale if rate and scale else (1e6 / usec if usec else 0.0)
        if not fps > 0:
            raise bad("no frame rate in strh / avih")
        ids = (b"%02ddc" % vstream, b"%02ddb" % vstream)
        ranges: List = []

        def add(off, sz):
            if sz == 0:
                if ranges:
                    ranges.append(ranges[-1])         # dropped frame: the previous picture stays on screen
            else:
                ranges.append((off, sz))

        movi_off, movi_sz = movi
        if idx1 is not None and idx1[1] >= 16:
            entries = [struct.unpack_from("<4sIII", mm, idx1[0] + 16 * k) for k in range(idx1[1] // 16)]
            # offsets count from the 'movi' fourcc (the usual reading) or from the start of the file (some muxers): take
            # the one under which the first entry lands on a chunk header carrying its own id
            rel = None
            for cand in (movi_off, 0):
                o = cand + entries[0][2]
                if o + 8 <= size and mm[o:o + 4] == entries[0][0]:
                    rel = cand
                    break
            if rel is None:
                raise bad("idx1 offsets point at no chunk")
            for cid, _flags, o, sz in entries:
                if cid in ids:
                    o += rel
                    if o + 8 + sz > size or mm[o:o + 4] != cid:
                        raise bad(f"idx1 entry for frame {len(ranges)} points outside the file or at another chunk")
                    add(o + 8, sz)
        else:
            def walk(start, end):
                for cid, o, sz in _riff_chunks(mm, start, end):
                    if cid == b"LIST" and sz >= 4 and mm[o:o + 4] == b"rec ":
                        walk(o + 4, o + sz)
                    elif cid in ids:
                        add(o, sz)
            walk(movi_off + 4, movi_off + movi_sz)
        if not ranges:
            raise bad("the video stream holds no frame")
        return _Mapped(path, fps, ranges, fh, mm)
    except Exception:
        mm.close()
        fh.close()
        raise


def open_source(video, fps: Optional[float] = None) -> Optional[JpegFrames]:
    """The JPEG source ``video`` names, or None when it is none of: a folder of .jpg / .jpeg files, a list of paths /
    bytes, a .mjpeg / .mjpg stream, an .avi file."""
    if isinstance(video, JpegFrames):
        return video
    if isinstance(video, (list, tuple)):
        return JpegList(video, 1.0 if fps is None else fps)
    if not isinstance(video, (str, os.PathLike)):
        return None
    path = os.fspath(video)
    if os.path.isdir(path):
        return jpeg_folder(path, 1.0 if fps is None else fps)
    low = path.lower()
    if low.endswith(MJPEG_EXT):
        return mjpeg_stream(path, 25.0 if fps is None else fps)
    if low.endswith(".avi"):
        if fps is not None:
            raise ValueError(f"Cannot open video file: {path} (an AVI carries its own frame rate; fps= is for frame folders and .mjpeg streams)")
        return avi_mjpeg(path)
    return None


# ------------------------------------------------------------------------------------------------ decode
def probe(data: bytes):
    """(status, (W, H, ncomp, hs, vs), message)."""
    from . import _lib
    lib = _lib.load()
    info = (C.c_int32 * 5)()
    rc = lib.tstar_jpeg_probe(data, len(data), info)
    msg = lib.tstar_last_error().decode() if rc else ""
    return rc, tuple(info), msg


def _sizes(geom):
    from . import _lib
    out = (C.c_size_t * 2)()
    _lib.check(_lib.load().tstar_jpeg_sizes(*geom, out), "tstar_jpeg_sizes")
    return int(out[0]), int(out[1])


SCALES = (1, 2, 4, 8)


def scale_mode(jpeg_scale: Optional[int] = None) -> int:
    """The keyword when given, else TSTAR_JPEG_SCALE, else 1: the factor 1, 2, 4 or 8 a JPEG source is decoded down by."""
    v = jpeg_scale if jpeg_scale is not None else (os.environ.get("TSTAR_JPEG_SCALE") or 1)
    try:
        s = int(v) if not isinstance(v, (bool, float)) else 0
    except (TypeError, ValueError):
        s = 0
    if s not in SCALES:
        raise ValueError(f"jpeg_scale={v!r}: expected one of {SCALES}")
    return s


def scaled_sizes(geom, scale: int):
    """(ow, oh, bytes of the per-frame plane workspace, covered) of a decode of ``geom`` at 1/scale size (tstar_jpeg_sizes_scaled)."""
    from . import _lib
    out = (C.c_size_t * 4)()
    _lib.check(_lib.load().tstar_jpeg_sizes_scaled(*geom, scale, out), "tstar_jpeg_sizes_scaled")
    return int(out[0]), int(out[1]), int(out[2]), bool(out[3])


def entropy_batch(datas: Sequence[bytes], geom, coef: np.ndarray, quant: np.ndarray, threads: int = 0):
    """Entropy-decode ``datas`` into coef int16 [>= n, blocks * 64] / quant uint16 [>= n, 192] -> (status int32 [n], message)."""
    from . import _lib
    lib = _lib.load()
    n = len(datas)
    blocks, _ = _sizes(geom)
    assert coef.dtype == np.int16 and coef.flags.c_contiguous and coef.size >= n * blocks * 64
    assert quant.dtype == np.uint16 and quant.flags.c_contiguous and quant.size >= n * 192
    ptrs = (C.c_char_p * n)(*datas)
    lens = (C.c_size_t * n)(*[len(d) for d in datas])
    status = np.full(n, -1, dtype=np.int32)
    rc = lib.tstar_jpeg_entropy_batch(ptrs, lens, n, *geom, coef.ctypes.data, quant.ctypes.data, threads, status.ctypes.data)
    if rc not in (0, 3):
        _lib.check(rc, "tstar_jpeg_entropy_batch")
    return status, (lib.tstar_last_error().decode() if rc else "")


# records of the device entropy stage (include/tstar_hip.h; csrc/jpeg_entropy_core.h)
SEGMENT_DTYPE = np.dtype([("frame", "<u4"), ("begin", "<u4"), ("end", "<u4"), ("first_mcu", "<u4"), ("n_mcu", "<u4"), ("last", "<u4")])
FRAME_DTYPE = np.dtype([("table_set", "<i4"), ("first_segment", "<i4"), ("n_segments", "<i4"), ("reserved", "<i4")])
TABLE_SET_BYTES = 9016
ROUTE_DEVICE, ROUTE_HOST = 0, 1
ENTROPY_MODES = ("host", "device")


def entropy_mode(entropy: Optional[str] = None) -> str:
    """The keyword when given, else TSTAR_JPEG_ENTROPY, else "host"."""
    mode = entropy if entropy is not None else (os.environ.get("TSTAR_JPEG_ENTROPY") or "host")
    if mode not in ENTROPY_MODES:
        raise ValueError(f"JPEG entropy mode {mode!r}: expected one of {ENTROPY_MODES}")
    return mode


# The split path of the device mode (include/tstar_hip.h, tstar_jpeg_entropy_split_device).  Defaults from the sweep in
# profiles/jpeg_split_entropy_measure.md; rounds behind the one in which a segment converges only copy states, so a generous
# max_rounds is cheap, while ONE abandoned 1080p frame costs a launch as much as the unsplit path did.
SPLIT_SUB_BYTES = 128          # bytes of a sub-sequence (one lane)
SPLIT_MAX_ROUNDS = 48          # a segment that has not converged by then is decoded by one lane
SPLIT_MIN_BYTES = 4096         # default of TSTAR_JPEG_SPLIT_BYTES: shorter segments stay one lane (a restart interval of an MCU row)
SUB_BYTES_MIN = 8              # TSTAR_JPEG_SUB_BYTES_MIN


def split_min_bytes() -> int:
    """min_split_bytes of the device mode: TSTAR_JPEG_SPLIT_BYTES when set (0: never split, the device mode as it was before the
    split path, for A/B runs), else SPLIT_MIN_BYTES."""
    v = os.environ.get("TSTAR_JPEG_SPLIT_BYTES")
    if v is None or v == "":
        return SPLIT_MIN_BYTES
    try:
        n = int(v)
    except ValueError:
        n = -1
    if n < 0 or n >= 1 << 31:
        raise ValueError(f"TSTAR_JPEG_SPLIT_BYTES={v!r}: expected a byte count >= 0 (0: never split)")
    return n


def split_workspace_bytes(total_bytes: int, n_segments: int, sub_bytes: int = SPLIT_SUB_BYTES) -> int:
    """Bytes of workspace a split call over ``n_segments`` segments inside ``total_bytes`` bytes needs (no HIP work)."""
    from . import _lib
    n = int(_lib.load().tstar_jpeg_split_workspace_bytes(total_bytes, n_segments, sub_bytes))
    if n == 0:
        raise ValueError(f"split_workspace_bytes: bad arguments (total_bytes={total_bytes}, n_segments={n_segments}, sub_bytes={sub_bytes})")
    return n


def split_threshold(min_split_bytes: int, longest: int) -> int:
    """The min_split_bytes a split call over segments of at most ``longest`` bytes is made with: the segment lengths are known on
    the host, and a call without a segment to split says 0 (never split), so that it does not queue the rounds at all."""
    return min_split_bytes if longest >= min_split_bytes else 0


def split_launch(head, longest: int, min_split_bytes: int, max_rounds: int, ws_ptr: int, ws_bytes: int, coef_ptr: int, status_ptr: int,
                 info_ptr: int, stream: int, sub_bytes: int = SPLIT_SUB_BYTES) -> None:
    """tstar_jpeg_entropy_split_device over the batch ``head`` describes (the leading arguments up to the geometry:
    DeviceBatch._head, or the same of a gathered batch), the one place that calls it; ``longest``: see split_threshold."""
    from . import _lib
    _lib.check(_lib.load().tstar_jpeg_entropy_split_device(*head, sub_bytes, split_threshold(min_split_bytes, longest), max_rounds, ws_ptr,
                                                           ws_bytes, coef_ptr, status_ptr, info_ptr, stream), "tstar_jpeg_entropy_split_device")


def count_split(sstats: dict, seg_info: np.ndarray) -> None:
    """Add a split call's seg_info (0 one lane, r > 0 converged in round r, -1 abandoned) to ``entropy_split_stats``."""
    sstats["split"] += int((seg_info != 0).sum())
    sstats["abandoned"] += int((seg_info < 0).sum())
    sstats["rounds_max"] = max(sstats["rounds_max"], int(seg_info.max(initial=0)))


def device_entropy_chunk(blocks: int, n_frames: int, chunk: Optional[int] = None, coef_budget: int = 512 << 20,
                         max_frames: int = 1024) -> int:
    """Frames per chunk of the device entropy path.  A frame without restart markers is one lane, so a launch wants as many
    frames as fit: bounded by ``coef_budget`` bytes of device coefficients (blocks * 128 per frame), by ``max_frames`` and
    by the frames there are; never below 1.  ``chunk`` overrides the budget, not the frame count."""
    if blocks <= 0 or n_frames <= 0:
        raise ValueError("device_entropy_chunk: blocks and n_frames must be positive")
    c = int(chunk) if chunk else min(max_frames, coef_budget // (blocks * 128))
    return max(1, min(c, n_frames))


class SegmentPlan:
    """What tstar_jpeg_plan_segments says about a batch: route int32 [n], frames FRAME_DTYPE [n], quant uint16 [n,192],
    table_sets uint8 [n_sets, TABLE_SET_BYTES], segments SEGMENT_DTYPE [n_segments], offsets uint64 [n], total_bytes."""

    def __init__(self, route, frames, quant, table_sets, segments, offsets, total_bytes):
        self.route, self.frames, self.quant, self.table_sets = route, frames, quant, table_sets
        self.segments, self.offsets, self.total_bytes = segments, offsets, int(total_bytes)

    def frame_status(self, seg_status: np.ndarray) -> np.ndarray:
        """int32 [n]: the status of a frame's first segment, in stream order, that is not OK; -1 for a host-routed frame."""
        out = np.where(self.route == ROUTE_DEVICE, OK, -1).astype(np.int32)
        bad = np.nonzero(seg_status)[0]
        for i in bad[::-1]:                                # the earliest segment of a frame is written last
            out[self.segments["frame"][i]] = seg_status[i]
        return out


def pack_offsets(datas: Sequence[bytes]):
    """(offsets uint64 [n], total bytes) of the frames laid end to end."""
    lens = np.fromiter((len(d) for d in datas), dtype=np.uint64, count=len(datas))
    offsets = np.zeros(len(datas), dtype=np.uint64)
    np.cumsum(lens[:-1], out=offsets[1:])
    return offsets, int(lens.sum())


def plan_segments(datas: Sequence[bytes], geom, offsets: Optional[np.ndarray] = None, cap_sets: int = 4,
                  cap_segments: Optional[int] = None) -> SegmentPlan:
    """Cut ``datas`` (frames of geometry ``geom``) into segments for the device entropy stage.  ``offsets``: where each frame
    sits in the byte buffer the segments index (default: end to end)."""
    from . import _lib
    lib = _lib.load()
    n = len(datas)
    if offsets is None:
        offsets, total = pack_offsets(datas)
    else:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        total = int(max(int(o) + len(d) for o, d in zip(offsets, datas)))
    ptrs = (C.c_char_p * n)(*datas)
    lens = (C.c_size_t * n)(*[len(d) for d in datas])
    route = np.empty(n, dtype=np.int32)
    frames = np.empty(n, dtype=FRAME_DTYPE)
    quant = np.empty((n, 192), dtype=np.uint16)
    out5 = (C.c_size_t * 5)()
    if cap_segments is None:
        # frames of one geometry and restart interval have one segment count: the first frame's, times n, fits in one call
        # (planning one frame twice is cheap; planning a chunk of restart-coded frames twice is not)
        per = 1 if n == 1 else len(plan_segments(datas[:1], geom, offsets[:1], cap_sets=1, cap_segments=64).segments)
        cap_segments = max(64, (per + 1) * n)
    while True:
        sets = np.empty((cap_sets, TABLE_SET_BYTES), dtype=np.uint8)
        segs = np.empty(cap_segments, dtype=SEGMENT_DTYPE)
        rc = lib.tstar_jpeg_plan_segments(ptrs, lens, offsets.ctypes.data, n, *geom, route.ctypes.data, frames.ctypes.data,
                                          quant.ctypes.data, sets.ctypes.data, cap_sets, segs.ctypes.data, cap_segments, out5)
        if rc != 4:
            break
        cap_sets, cap_segments = max(cap_sets, int(out5[0])), max(cap_segments, int(out5[1]))
    _lib.check(rc, "tstar_jpeg_plan_segments")
    assert (int(out5[2]), int(out5[3]), int(out5[4])) == (TABLE_SET_BYTES, SEGMENT_DTYPE.itemsize, FRAME_DTYPE.itemsize)
    return SegmentPlan(route, frames, quant, sets[:int(out5[0])], segs[:int(out5[1])], offsets, total)


def _host_batch(buf: np.ndarray, plan: SegmentPlan, geom, coef: Optional[np.ndarray]):
    """What the two host entry points share -> (coef, seg_status, the leading arguments of the call up to the geometry)."""
    n, nseg = len(plan.route), len(plan.segments)
    blocks, _ = _sizes(geom)
    if coef is None:
        coef = np.empty((n, blocks * 64), dtype=np.int16)
    assert coef.dtype == np.int16 and coef.flags.c_contiguous and coef.size >= n * blocks * 64
    assert buf.dtype == np.uint8 and buf.flags.c_contiguous and buf.size >= plan.total_bytes
    status = np.full(nseg, -1, dtype=np.int32)
    head = (buf.ctypes.data, plan.total_bytes, plan.segments.ctypes.data, plan.table_sets.ctypes.data, len(plan.table_sets),
            plan.frames.ctypes.data, n, nseg, *geom)
    return coef, status, head


def entropy_segments_host(buf: np.ndarray, plan: SegmentPlan, geom, coef: Optional[np.ndarray] = None):
    """The device kernel's decode core on the CPU over ``buf`` (uint8, the frames at plan.offsets) -> (coef int16
    [n, blocks * 64], seg_status int32 [n_segments])."""
    from . import _lib
    coef, status, head = _host_batch(buf, plan, geom, coef)
    if len(status):
        _lib.check(_lib.load().tstar_jpeg_entropy_segments_host(*head, coef.ctypes.data, status.ctypes.data),
                   "tstar_jpeg_entropy_segments_host")
    return coef, status


def entropy_split_host(buf: np.ndarray, plan: SegmentPlan, geom, sub_bytes: int = SPLIT_SUB_BYTES, min_split_bytes: int = SPLIT_MIN_BYTES,
                       max_rounds: int = SPLIT_MAX_ROUNDS, coef: Optional[np.ndarray] = None):
    """The split launcher's CPU mirror (same core, same round order) over ``buf`` -> (coef int16 [n, blocks * 64], seg_status
    int32 [n_segments], seg_info int32 [n_segments]: 0 one lane, r > 0 converged in round r, -1 abandoned)."""
    from . import _lib
    coef, status, head = _host_batch(buf, plan, geom, coef)
    nseg = len(status)
    info = np.full(nseg, -9, dtype=np.int32)
    if nseg:
        ws = np.empty(split_workspace_bytes(plan.total_bytes, nseg, sub_bytes) // 8 + 1, dtype=np.uint64)
        _lib.check(_lib.load().tstar_jpeg_entropy_split_host(
            *head, sub_bytes, min_split_bytes, max_rounds, ws.ctypes.data, ws.nbytes, coef.ctypes.data, status.ctypes.data,
            info.ctypes.data), "tstar_jpeg_entropy_split_host")
    return coef, status, info


def device_entropy_take(lens: Sequence[int], byte_budget: int = 1 << 30) -> int:
    """How many of a chunk's frames (compressed sizes ``lens``, in order) go up together: whole files are uploaded, metadata
    included, and a segment addresses the upload with 32 bits, so a chunk stops before ``byte_budget`` bytes; never below 1."""
    total = 0
    for k, n in enumerate(lens):
        total += int(n)
        if k and total > byte_budget:
            return k
    return max(1, len(lens))


def _round16(x: int) -> int:
    return (x + 15) & ~15


class DeviceBatch:
    """One chunk's upload for the device entropy stage: the compressed bytes, then (16-byte aligned) the quant rows, the frame
    records, the segments and the table sets, in ONE buffer so that one copy carries everything."""

    def __init__(self, datas: Sequence[bytes], geom):
        self.offsets, self.total = pack_offsets(datas)
        self.plan = plan_segments(datas, geom, self.offsets)
        p = self.plan
        self.parts = {}
        at = _round16(self.total)
        for name, arr in (("quant", p.quant), ("frames", p.frames), ("segments", p.segments), ("table_sets", p.table_sets)):
            self.parts[name] = (at, arr.nbytes)
            at = _round16(at + arr.nbytes)
        self.nbytes = at
        self.datas = datas
        seg = p.segments
        self.longest = int((seg["end"].astype(np.int64) - seg["begin"]).max(initial=0))      # bytes of the longest segment

    def fill(self, host: np.ndarray) -> None:
        """Write the upload into ``host`` (uint8, at least nbytes)."""
        for o, d in zip(self.offsets, self.datas):
            host[int(o):int(o) + len(d)] = np.frombuffer(d, dtype=np.uint8)
        p = self.plan
        for name, arr in (("quant", p.quant), ("frames", p.frames), ("segments", p.segments), ("table_sets", p.table_sets)):
            at, nb = self.parts[name]
            host[at:at + nb] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)

    def _head(self, d_buf, geom):
        """The leading arguments of both device entry points, up to the geometry."""
        p = self.plan
        base = d_buf.data_ptr()
        return (base, self.total, base + self.parts["segments"][0], base + self.parts["table_sets"][0], len(p.table_sets),
                base + self.parts["frames"][0], len(p.route), len(p.segments), *geom)

    def launch(self, d_buf, d_coef, d_seg_status, geom, stream: int) -> None:
        """Entropy-decode on the device: d_buf holds what fill() wrote; d_coef int16 [>= n, blocks * 64]."""
        from . import _lib
        _lib.check(_lib.load().tstar_jpeg_entropy_device(*self._head(d_buf, geom), d_coef.data_ptr(), d_seg_status.data_ptr(), stream),
                   "tstar_jpeg_entropy_device")

    def launch_split(self, d_buf, d_coef, d_seg_status, d_seg_info, d_workspace, geom, stream: int, sub_bytes: int = SPLIT_SUB_BYTES,
                     min_split_bytes: int = SPLIT_MIN_BYTES, max_rounds: int = SPLIT_MAX_ROUNDS) -> None:
        """launch() through the split path: d_seg_info int32 [>= n_segments]; d_workspace uint8, 8-byte aligned, at least
        split_workspace_bytes(self.total, n_segments, sub_bytes)."""
        split_launch(self._head(d_buf, geom), self.longest, min_split_bytes, max_rounds, d_workspace.data_ptr(),
                     d_workspace.numel() * d_workspace.element_size(), d_coef.data_ptr(), d_seg_status.data_ptr(), d_seg_info.data_ptr(),
                     stream, sub_bytes)


def _pillow_rgb(data: bytes, label: str, scale: int = 1, check_size=None) -> np.ndarray:
    """Pillow's pixels of one JPEG, at 1/scale size through ``Image.draft`` (libjpeg's scaled decode).  ``check_size(w, h)`` sees the
    file's own size before anything is decoded."""
    import io
    from PIL import Image
    try:
        with Image.open(io.BytesIO(data)) as im:
            w, h = im.size
            if check_size is not None:
                check_size(w, h)
            if scale > 1:
                im.draft(im.mode, (w // scale, h // scale))
                if im.size != (-(-w // scale), -(-h // scale)):
                    raise ValueError(f"Pillow decodes it at {im.size[0]}x{im.size[1]}, not at 1/{scale} of {w}x{h}")
            return np.array(im.convert("RGB"), dtype=np.uint8)
    except _SizeError:
        raise
    except Exception as e:
        raise ValueError(f"Cannot open video file: {label} ({e})")


class _SizeError(ValueError):
    """A frame whose size the open refuses: the message names the file already."""


def decode_host(datas: Sequence[bytes], threads: int = 0) -> np.ndarray:
    """JPEG bytes -> uint8 [n,H,W,3] through the host path alone (entropy stage + scalar reference of the kernels); every
    frame must be one the decoder covers, of the first frame's geometry.  Raises ValueError naming the frame otherwise."""
    from . import _lib
    datas = list(datas)
    rc, geom, msg = probe(datas[0])
    if rc:
        raise ValueError(f"JPEG frame 0: {msg}")
    blocks, _ = _sizes(geom)
    n = len(datas)
    coef = np.empty((n, blocks * 64), dtype=np.int16)
    quant = np.empty((n, 192), dtype=np.uint16)
    status, msg = entropy_batch(datas, geom, coef, quant, threads)
    if status.any():
        raise ValueError(f"JPEG {msg}")
    W, H = geom[0], geom[1]
    out = np.empty((n, H, W, 3), dtype=np.uint8)
    _lib.check(_lib.load().tstar_jpeg_reconstruct_host(coef.ctypes.data, quant.ctypes.data, n, *geom, out.ctypes.data, threads),
               "tstar_jpeg_reconstruct_host")
    return out


def wanted_frames(n_frames: int, fps: float):
    """Raw frame of every logical second (interface_searcher.py:360)."""
    return [int(sec * fps) for sec in range(int(n_frames / fps))]


# ------------------------------------------------------------------------------------------------ open
class JpegOpen:
    """What an open of a JPEG source knows before its first chunk, and what every mode does with ONE frame: ``raw`` is the raw frame
    behind every frame k the open decodes, the first of them fixes the picture size (W, H), the first one the kernels cover fixes the
    geometry.  The three counter dicts of the store live here; ``seconds`` [len(raw)] says how many logical seconds frame k serves
    (default one each), and every count is in seconds.  ``scale``: every frame is decoded at 1/scale size, ow x oh = ceil(W / scale) x
    ceil(H / scale) (the kernels' reduced inverse DCTs, Pillow's ``draft`` for the frames that go to Pillow); W, H and every message
    keep speaking of the file's own size."""

    def __init__(self, src: JpegFrames, raw: Sequence[int], device, seconds: Optional[np.ndarray] = None, scale: int = 1):
        self.src, self.raw, self.device, self.scale = src, raw, device, int(scale)
        self.first = src.read(raw[0])
        self.W = self.H = self.ow = self.oh = self.geom = None
        self.blocks = self.plane_bytes = 0
        self.seconds = np.ones(len(raw), dtype=np.int64) if seconds is None else seconds
        self.reconstructs = "host" if str(device).startswith("cpu") else "device"       # who turns coefficients into pixels
        self.stats = {"device": 0, "host": 0, "pillow": 0}
        self.estats = {"device": 0, "host": 0}
        self.sstats = {"split": 0, "abandoned": 0, "rounds_max": 0}

    @classmethod
    def for_geometry(cls, src: JpegFrames, raw: Sequence[int], device, geom, scale: int = 1) -> "JpegOpen":
        """An open whose geometry is known up front (every frame of ``raw`` was probed by the caller): what ``prelude`` leaves behind
        after the first covered frame, without decoding anything.  An EntropyRunner can be driven over it outside ``load_jpeg``."""
        ctx = cls(src, raw, device, scale=scale)
        ctx.check_size(0, int(geom[0]), int(geom[1]))
        ctx.geom = tuple(int(v) for v in geom)
        ctx.blocks, ctx.plane_bytes = _sizes(ctx.geom)
        if ctx.scale > 1:
            ctx.plane_bytes = scaled_sizes(ctx.geom, ctx.scale)[2]
        return ctx

    def attach(self, store):
        store.decode_stats, store.entropy_stats, store.entropy_split_stats = self.stats, self.estats, self.sstats
        store.jpeg_scale, store.source_size = self.scale, (self.W, self.H)
        return store

    def count(self, frames, decode: Optional[str] = None, entropy: Optional[str] = None) -> None:
        n = int(self.seconds[frames].sum())
        if decode is not None:
            self.stats[decode] += n
        if entropy is not None:
            self.estats[entropy] += n

    def read(self, k: int) -> bytes:
        return self.first if k == 0 else self.src.read(self.raw[k])

    def error(self, k: int, why: str) -> ValueError:
        return ValueError(f"Cannot open video file: {self.src.label(self.raw[k])} ({why})")

    def check_size(self, k: int, w: int, h: int) -> None:
        """The first frame's size is the picture size; ValueError for a later frame of another, or for a picture with a side shorter than
        the scale (Pillow's draft, the yardstick, cannot be held to the scale there)."""
        if self.W is None:
            if min(w, h) < self.scale:
                raise _SizeError(f"Cannot open video file: {self.src.label(self.raw[k])} is {w}x{h}: jpeg_scale={self.scale} needs a picture "
                                 f"of at least {self.scale}x{self.scale}")
            self.W, self.H = int(w), int(h)
            self.ow, self.oh = -(-self.W // self.scale), -(-self.H // self.scale)
        elif (w, h) != (self.W, self.H):
            raise _SizeError(f"Cannot open video file: {self.src.label(self.raw[k])} is {w}x{h}, the first frame is {self.W}x{self.H}")

    def pillow(self, k: int, data: bytes) -> np.ndarray:
        """Frame k as Pillow decodes it at the open's scale (exact, on the host), size-checked and counted."""
        arr = _pillow_rgb(data, self.src.label(self.raw[k]), self.scale, lambda w, h: self.check_size(k, w, h))
        self.count([k], "pillow")
        return arr

    def prelude(self, k: int, data: bytes) -> Optional[np.ndarray]:
        """One step while no covered frame has been seen: frame k is probed alone -> None when the kernels cover it at the open's scale
        (its geometry is the open's from here on), else Pillow's pixels; ValueError when it is broken or of another size."""
        rc, info, msg = probe(data)
        if rc == MALFORMED:
            raise self.error(k, msg)
        if rc != OK:
            return self.pillow(k, data)
        self.check_size(k, info[0], info[1])
        blocks, plane_bytes = _sizes(info)
        if self.scale > 1:
            _, _, plane_bytes, covered = scaled_sizes(info, self.scale)
            if not covered:                               # 4:2:2 whose scaled chroma rows are at most 2 samples long
                return self.pillow(k, data)
        self.geom, self.blocks, self.plane_bytes = info, blocks, plane_bytes
        return None

    def host_verdict(self, k: int, data: bytes):
        """Frame k, which a batch did not return OK for, alone through the host entropy decoder, whose verdict stands -> (coef int16
        [1, blocks * 64], quant int16 [1, 192]) (torch, host) to reconstruct when it is OK after all, else Pillow's pixels (uncovered,
        or covered sampling other than the batch's); ValueError when it is broken or of another size."""
        import torch
        coef1, quant1 = torch.empty((1, self.blocks * 64), dtype=torch.int16), torch.empty((1, 192), dtype=torch.int16)
        status, message = entropy_batch([data], self.geom, coef1.numpy(), quant1.numpy().view(np.uint16), 1)
        self.count([k], entropy="host")
        if status[0] == OK:
            self.count([k], self.reconstructs)
            return coef1, quant1
        if status[0] == MALFORMED:
            raise self.error(k, message.split(': ', 2)[-1])
        if status[0] == GEOMETRY:
            _, info, _ = probe(data)
            self.check_size(k, info[0], info[1])
        return self.pillow(k, data)

    def reconstruct(self, coef_ptr: int, quant_ptr: int, n: int, planes_ptr: int, out_ptr: int, stream: int) -> None:
        """n frames of device coefficients -> u8 [n,oh,ow,3] at ``out_ptr`` on ``stream``: the one place an open calls the device stage.
        Scale 1 is tstar_jpeg_reconstruct as it always was."""
        from . import _lib
        lib = _lib.load()
        if self.scale == 1:
            _lib.check(lib.tstar_jpeg_reconstruct(coef_ptr, quant_ptr, n, *self.geom, planes_ptr, out_ptr, stream), "tstar_jpeg_reconstruct")
        else:
            _lib.check(lib.tstar_jpeg_reconstruct_scaled(coef_ptr, quant_ptr, n, *self.geom, self.scale, planes_ptr, out_ptr, stream),
                       "tstar_jpeg_reconstruct_scaled")

    def reconstruct_host(self, coef_ptr: int, quant_ptr: int, n: int, out_ptr: int, threads: int) -> None:
        """The same through the host twin, for a CPU store."""
        from . import _lib
        lib = _lib.load()
        if self.scale == 1:
            _lib.check(lib.tstar_jpeg_reconstruct_host(coef_ptr, quant_ptr, n, *self.geom, out_ptr, threads), "tstar_jpeg_reconstruct_host")
        else:
            _lib.check(lib.tstar_jpeg_reconstruct_scaled_host(coef_ptr, quant_ptr, n, *self.geom, self.scale, out_ptr, threads),
                       "tstar_jpeg_reconstruct_scaled_host")

    def reconstruct_one(self, coef1, quant1, out, planes=None) -> None:
        """One frame from host_verdict's coefficients into ``out`` (u8 [1,oh,ow,3] on the device), on the current stream."""
        import torch
        from . import _lib
        if planes is None:
            planes = torch.empty(self.plane_bytes, dtype=torch.uint8, device=self.device)
        dc, dq = coef1.to(self.device), quant1.to(self.device)
        self.reconstruct(dc.data_ptr(), dq.data_ptr(), 1, planes.data_ptr(), out.data_ptr(), _lib.stream_ptr())


class EntropyRunner:
    """The device-entropy stage of an open, chunk by chunk.  Owns its buffers -- two pinned uploads and two pinned status blocks (grown
    on demand, used in turn), and ONE d_buf, d_ws and d_coef [chunk, blocks * 64]: every chunk of an open goes to the same stream, in
    order -- the chunk size (device_entropy_chunk) and the take rule (device_entropy_take).  ``submit`` queues a chunk without waiting;
    ``collect`` waits for it and says which frames the device did not return OK for."""

    def __init__(self, ctx: JpegOpen, chunk: Optional[int], min_split_bytes: int):
        import torch
        self.ctx, self.min_split = ctx, min_split_bytes
        self.chunk = device_entropy_chunk(ctx.blocks, len(ctx.raw), chunk)
        self.d_coef = torch.empty((self.chunk, ctx.blocks * 64), dtype=torch.int16, device=ctx.device)
        self.pinned, self.status, self.done = [None, None], [None, None], [None, None]
        self.d_buf = self.d_ws = None
        self.submitted = 0

    def read(self, k0: int):
        """The files of the chunk that starts at frame k0."""
        datas = [self.ctx.read(k) for k in range(k0, min(len(self.ctx.raw), k0 + self.chunk))]
        return datas[:device_entropy_take([len(d) for d in datas])]

    def submit(self, k0: int, datas, stream):
        """Plan, fill, upload, entropy-decode into d_coef and copy the statuses back, all on ``stream`` -> the ticket for collect();
        d_buf holds the chunk as DeviceBatch.fill wrote it until the next submit."""
        import torch
        batch = DeviceBatch(datas, self.ctx.geom)
        nseg, b, device = len(batch.plan.segments), self.submitted & 1, self.ctx.device
        self.submitted += 1
        if self.done[b] is not None:
            self.done[b].synchronize()                    # this pinned buffer's previous copy has left
        if self.pinned[b] is None or self.pinned[b].numel() < batch.nbytes:
            self.pinned[b] = torch.empty(batch.nbytes + batch.nbytes // 4, dtype=torch.uint8).pin_memory()
        if self.status[b] is None or self.status[b].numel() < 2 * nseg:          # statuses, then seg_info
            self.status[b] = torch.empty(2 * (nseg + nseg // 4 + 64), dtype=torch.int32).pin_memory()
        batch.fill(self.pinned[b].numpy())
        with torch.cuda.stream(stream):
            if self.d_buf is None or self.d_buf.numel() < batch.nbytes:
                # allocated under the stream: a replaced buffer is not handed out again before the work queued on it is done
                self.d_buf = None
                self.d_buf = torch.empty(batch.nbytes + batch.nbytes // 4, dtype=torch.uint8, device=device)
            self.d_buf[:batch.nbytes].copy_(self.pinned[b][:batch.nbytes], non_blocking=True)
            if nseg:
                d_status = torch.empty(2 * nseg, dtype=torch.int32, device=device)
                ws_bytes = split_workspace_bytes(batch.total, nseg)
                if self.d_ws is None or self.d_ws.numel() * 8 < ws_bytes:
                    self.d_ws = None
                    self.d_ws = torch.empty((ws_bytes + ws_bytes // 4) // 8 + 1, dtype=torch.int64, device=device)
                batch.launch_split(self.d_buf, self.d_coef, d_status[:nseg], d_status[nseg:], self.d_ws, self.ctx.geom, stream.cuda_stream,
                                   min_split_bytes=self.min_split)
                self.status[b][:2 * nseg].copy_(d_status, non_blocking=True)
            self.done[b] = torch.cuda.Event(blocking=True)       # the wait in collect sleeps: the CPU is what this stage saves
            self.done[b].record(stream)
        return k0, batch, b

    def collect(self, ticket, split_stats: bool = True):
        """Wait for a chunk's statuses -> the frames (positions in the chunk) the device did not return OK for, host-routed ones
        included; the others are counted as the device's, and the split counters are updated (``split_stats=False``: left alone, for
        a caller that counts ``seg_info`` itself)."""
        k0, batch, b = ticket
        self.done[b].synchronize()
        nseg = len(batch.plan.segments)
        status = self.status[b][:2 * nseg].numpy()
        fstat = batch.plan.frame_status(status[:nseg])
        if split_stats:
            count_split(self.ctx.sstats, status[nseg:])
        self.ctx.count(k0 + np.flatnonzero(fstat == OK), "device", "device")
        return [int(j) for j in np.nonzero(fstat)[0]]

    def seg_info(self, ticket) -> np.ndarray:
        """The split path's word on every segment of a collected chunk (int32 [n_segments]: 0 one lane, r > 0 converged in round r,
        -1 abandoned), valid until the second submit after the chunk's."""
        _, batch, b = ticket
        nseg = len(batch.plan.segments)
        return self.status[b][nseg:2 * nseg].numpy().copy()


def _device_entropy_chunks(ctx: JpegOpen, store, s0: int, chunk: Optional[int], min_split_bytes: int, side) -> None:
    """load_jpeg from frame s0 on with the entropy stage on the device: every chunk is submitted, reconstructed into the store and
    collected one chunk later (the host plans the next chunk while this one runs); a frame the device did not return OK for gets the
    host decoder's verdict."""
    import torch
    run = EntropyRunner(ctx, chunk, min_split_bytes)
    planes = torch.empty((run.chunk, ctx.plane_bytes), dtype=torch.uint8, device=ctx.device)

    def finish(ticket):
        k0, batch, _ = ticket
        for j in run.collect(ticket):
            verdict = ctx.host_verdict(k0 + j, batch.datas[j])
            with torch.cuda.stream(side):                 # behind the chunk's kernels, which wrote cleared coefficients' pixels here
                if isinstance(verdict, tuple):
                    ctx.reconstruct_one(*verdict, store[k0 + j:k0 + j + 1], planes)
                else:
                    store[k0 + j].copy_(torch.from_numpy(verdict))

    before = None
    while s0 < len(ctx.raw):
        datas = run.read(s0)
        ticket = run.submit(s0, datas, side)
        batch = ticket[1]
        if len(batch.plan.segments):
            ctx.reconstruct(run.d_coef.data_ptr(), run.d_buf.data_ptr() + batch.parts["quant"][0], len(datas), planes.data_ptr(),
                            store[s0:s0 + len(datas)].data_ptr(), side.cuda_stream)
        if before is not None:
            finish(before)
        before = ticket
        s0 += len(datas)
    if before is not None:
        finish(before)


def _host_entropy_chunks(ctx: JpegOpen, store, s0: int, chunk: Optional[int], threads: int, side) -> None:
    """load_jpeg from frame s0 on with the entropy stage on the host thread pool: coefficients into (on a GPU: two sets of pinned)
    buffers, reconstruction by the HIP kernels on the side stream while the next chunk is entropy-decoded, or by their host mirror."""
    import torch
    n_sec, geom, on_gpu = len(ctx.raw), ctx.geom, side is not None
    c = min(chunk if chunk else max(1, min(64, (48 << 20) // (ctx.blocks * 128))), n_sec)
    coefs = [torch.empty((c, ctx.blocks * 64), dtype=torch.int16, pin_memory=on_gpu) for _ in range(1 + on_gpu)]
    quants = [torch.empty((c, 192), dtype=torch.int16, pin_memory=on_gpu) for _ in range(1 + on_gpu)]
    if on_gpu:
        d_coef = [torch.empty((c, ctx.blocks * 64), dtype=torch.int16, device=ctx.device) for _ in range(2)]
        d_quant = [torch.empty((c, 192), dtype=torch.int16, device=ctx.device) for _ in range(2)]
        planes = torch.empty((c, ctx.plane_bytes), dtype=torch.uint8, device=ctx.device)    # one: the side stream runs chunks in order
        done = [None, None]
    ci = 0
    while s0 < n_sec:
        b = ci & 1 if on_gpu else 0
        if on_gpu and done[b] is not None:
            done[b].synchronize()                         # the pinned buffers' previous copy has left
        datas = [ctx.read(k) for k in range(s0, min(n_sec, s0 + c))]
        n = len(datas)
        coef, quant = coefs[b], quants[b]
        status, _ = entropy_batch(datas, geom, coef.numpy(), quant.numpy().view(np.uint16), threads)
        ctx.count(s0 + np.flatnonzero(status == OK), ctx.reconstructs, "host")
        fallback = []
        for j in (int(j) for j in np.nonzero(status)[0]):
            verdict = ctx.host_verdict(s0 + j, datas[j])
            if isinstance(verdict, tuple):
                coef[j], quant[j] = verdict[0][0], verdict[1][0]
            else:
                fallback.append((j, verdict))
        if on_gpu:
            with torch.cuda.stream(side):
                d_coef[b][:n].copy_(coef[:n], non_blocking=True)
                d_quant[b][:n].copy_(quant[:n], non_blocking=True)
                ctx.reconstruct(d_coef[b].data_ptr(), d_quant[b].data_ptr(), n, planes.data_ptr(), store[s0:s0 + n].data_ptr(), side.cuda_stream)
                done[b] = torch.cuda.Event()
                done[b].record(side)
                for j, arr in fallback:                   # after the kernels, which wrote whatever the stale coefficients gave into these slots
                    store[s0 + j].copy_(torch.from_numpy(arr))
        else:
            out = store[s0:s0 + n].numpy()
            ctx.reconstruct_host(coef.data_ptr(), quant.data_ptr(), n, out.ctypes.data, threads)
            for j, arr in fallback:
                out[j] = arr
        s0 += n
        ci += 1


def load_jpeg(src: JpegFrames, device: str = "cuda", chunk: Optional[int] = None, threads: int = 0, entropy: Optional[str] = None,
              scale: int = 1):
    """Decode the wanted frames of ``src`` into a FrameStore (RGB u8 [N,H,W,3] on ``device``; at ``scale`` 2, 4 or 8 the frames are
    decoded at 1/scale size, [N, ceil(H / scale), ceil(W / scale), 3], byte for byte Pillow's ``draft``).  ``entropy``: "host" (the
    default; TSTAR_JPEG_ENTROPY when absent) or "device", where the Huffman decode runs on the GPU too and the store's
    ``entropy_stats`` says how many frames each side entropy-decoded.  The device mode works on larger chunks (a frame without
    restart markers is one segment): next to the store it holds up to 512 MiB of coefficients plus half as much of planes on the
    device while loading, against two times 64 frames' worth in host mode (``device_entropy_chunk``; ``chunk`` lowers both), and
    72 bytes of workspace per SPLIT_SUB_BYTES compressed bytes of a chunk.  Segments of at least TSTAR_JPEG_SPLIT_BYTES bytes
    (``split_min_bytes``; 0: none) are decoded by many lanes; ``entropy_split_stats`` counts the segments that were
    (``split``), those of them given up after SPLIT_MAX_ROUNDS rounds and decoded by one lane (``abandoned``) and the most
    rounds a segment took (``rounds_max``).  A JpegOpen carries the open: its prelude sends frames to Pillow until one is covered, then
    the chunks go through _device_entropy_chunks (an EntropyRunner, as ``jpeg_resident.load_resident`` drives one) or _host_entropy_chunks."""
    import torch
    from .video import FrameStore
    want = wanted_frames(src.n_frames, src.fps)
    if not want:
        raise ValueError(f"Cannot open video file: {src.name} (shorter than one second)")
    on_gpu = not str(device).startswith("cpu")
    if entropy == "device" and not on_gpu:
        raise ValueError("load_jpeg: entropy='device' needs a GPU store (device='cpu' was asked for)")
    dev_entropy = entropy_mode(entropy) == "device" and on_gpu       # TSTAR_JPEG_ENTROPY=device leaves a CPU store on the host path
    min_split = split_min_bytes() if dev_entropy else 0
    ctx = JpegOpen(src, want, device, scale=scale)
    side = torch.cuda.Stream(device=device) if on_gpu else None
    store, s0 = None, 0
    try:
        while s0 < len(want) and ctx.geom is None:
            arr = ctx.prelude(s0, ctx.read(s0))
            if store is None:                             # the first frame has fixed the picture size
                store = torch.empty((len(want), ctx.oh, ctx.ow, 3), dtype=torch.uint8, device=device)
            if arr is not None:
                store[s0].copy_(torch.from_numpy(arr))
                s0 += 1
        if s0 < len(want) and dev_entropy:
            _device_entropy_chunks(ctx, store, s0, chunk, min_split, side)
        elif s0 < len(want):
            _host_entropy_chunks(ctx, store, s0, chunk, threads, side)
    finally:
        # also on the way out with an error: the side stream may still be writing the previous chunk into the store, the
        # planes and the staged coefficients, and the allocator must not hand those blocks out before it is done
        if side is not None:
            side.synchronize()
    return ctx.attach(FrameStore(store, src.fps, src.n_frames, name=src.name))
