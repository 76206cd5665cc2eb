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
        from . import _lib
        _lib.check(_lib.load().tstar_jpeg_entropy_split_device(
            *self._head(d_buf, geom), sub_bytes, min_split_bytes, max_rounds, d_workspace.data_ptr(),
            d_workspace.numel() * d_workspace.element_size(), d_coef.data_ptr(), d_seg_status.data_ptr(), d_seg_info.data_ptr(), stream),
            "tstar_jpeg_entropy_split_device")


def _pillow_rgb(data: bytes, label: str) -> np.ndarray:
    import io
    from PIL import Image
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.array(im.convert("RGB"), dtype=np.uint8)
    except Exception as e:
        raise ValueError(f"Cannot open video file: {label} ({e})")


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


def load_jpeg(src: JpegFrames, device: str = "cuda", chunk: Optional[int] = None, threads: int = 0, entropy: Optional[str] = None):
    """Decode the wanted frames of ``src`` into a FrameStore (RGB u8 [N,H,W,3] on ``device``).  ``entropy``: "host" (the
    default; TSTAR_JPEG_ENTROPY when absent) or "device", where the Huffman decode runs on the GPU too and the store's
    ``entropy_stats`` says how many frames each side entropy-decoded.  The device mode works on larger chunks (a frame without
    restart markers is one segment): next to the store it holds up to 512 MiB of coefficients plus half as much of planes on the
    device while loading, against two times 64 frames' worth in host mode (``device_entropy_chunk``; ``chunk`` lowers both), and
    72 bytes of workspace per SPLIT_SUB_BYTES compressed bytes of a chunk.  Segments of at least TSTAR_JPEG_SPLIT_BYTES bytes
    (``split_min_bytes``; 0: none) are decoded by many lanes; ``entropy_split_stats`` counts the segments that were
    (``split``), those of them given up after SPLIT_MAX_ROUNDS rounds and decoded by one lane (``abandoned``) and the most
    rounds a segment took (``rounds_max``)."""
    import torch
    from . import _lib
    from .video import FrameStore
    lib = _lib.load()
    want = wanted_frames(src.n_frames, src.fps)
    if not want:
        raise ValueError(f"Cannot open video file: {src.name} (shorter than one second)")
    on_gpu = not str(device).startswith("cpu")
    if entropy == "device" and not on_gpu:
        raise ValueError("load_jpeg: entropy='device' needs a GPU store (device='cpu' was asked for)")
    dev_entropy = entropy_mode(entropy) == "device" and on_gpu       # TSTAR_JPEG_ENTROPY=device leaves a CPU store on the host path

    # the first wanted frame fixes the picture size; the first frame the kernels cover fixes the device geometry
    first = src.read(want[0])
    rc, info, msg = probe(first)
    if rc == MALFORMED:
        raise ValueError(f"Cannot open video file: {src.label(want[0])} ({msg})")
    if rc == OK:
        W, H = info[0], info[1]
    else:
        H, W = _pillow_rgb(first, src.label(want[0])).shape[:2]
    n_sec = len(want)
    store = torch.empty((n_sec, H, W, 3), dtype=torch.uint8, device=device)
    stats = {"device": 0, "host": 0, "pillow": 0}
    estats = {"device": 0, "host": 0}
    sstats = {"split": 0, "abandoned": 0, "rounds_max": 0}
    min_split = split_min_bytes() if dev_entropy else 0
    geom = None
    bufs = None
    side = torch.cuda.Stream(device=device) if on_gpu else None
    done = [None, None]

    def alloc(g):
        blocks, plane_bytes = _sizes(g)
        c = chunk if chunk else max(1, min(64, (48 << 20) // (blocks * 128)))
        c = min(c, n_sec)
        b = {"chunk": c, "blocks": blocks}
        if dev_entropy:
            c = b["chunk"] = device_entropy_chunk(blocks, n_sec, chunk)
            b["pinned"] = [None, None]                  # uploads (grown on demand); statuses come back into "status"
            b["status"] = [None, None]
            b["d_buf"] = None
            b["d_ws"] = None
            b["d_coef"] = torch.empty((c, blocks * 64), dtype=torch.int16, device=device)
            b["planes"] = torch.empty((c, plane_bytes), dtype=torch.uint8, device=device)
        elif on_gpu:
            b["coef"] = [torch.empty((c, blocks * 64), dtype=torch.int16).pin_memory() for _ in range(2)]
            b["quant"] = [torch.empty((c, 192), dtype=torch.int16).pin_memory() for _ in range(2)]
            b["d_coef"] = [torch.empty((c, blocks * 64), dtype=torch.int16, device=device) for _ in range(2)]
            b["d_quant"] = [torch.empty((c, 192), dtype=torch.int16, device=device) for _ in range(2)]
            b["planes"] = torch.empty((c, plane_bytes), dtype=torch.uint8, device=device)   # one: the side stream runs chunks in order
        else:
            b["coef"] = [torch.empty((c, blocks * 64), dtype=torch.int16)]
            b["quant"] = [torch.empty((c, 192), dtype=torch.int16)]
        return b

    def fallback_rgb(data, label, status, message=None):
        """A frame the host entropy stage did not return OK for: ValueError when it is broken or of another size, else what
        Pillow decodes (uncovered, or covered sampling other than the batch's: exact, on the host)."""
        if status == MALFORMED:
            if message is None:
                one_c = np.empty((1, bufs["blocks"] * 64), dtype=np.int16)
                _, message = entropy_batch([data], geom, one_c, np.empty((1, 192), dtype=np.uint16), 1)
            raise ValueError(f"Cannot open video file: {label} ({message.split(': ', 2)[-1]})")
        if status == GEOMETRY:
            _, inf, _ = probe(data)
            if (inf[0], inf[1]) != (W, H):
                raise ValueError(f"Cannot open video file: {label} is {inf[0]}x{inf[1]}, the first frame is {W}x{H}")
        arr = _pillow_rgb(data, label)
        if arr.shape != (H, W, 3):
            raise ValueError(f"Cannot open video file: {label} is {arr.shape[1]}x{arr.shape[0]}, the first frame is {W}x{H}")
        return arr

    pending = []                                        # device entropy: chunks launched whose statuses are not read yet

    def submit_device(s0, idx, datas, b):
        """Upload, entropy-decode and reconstruct one chunk on the side stream; the statuses are read in finish_device."""
        n = len(idx)
        batch = DeviceBatch(datas, geom)
        nseg = len(batch.plan.segments)
        if done[b] is not None:
            done[b].synchronize()                         # this pinned buffer's previous copy has left
        if bufs["pinned"][b] is None or bufs["pinned"][b].numel() < batch.nbytes:
            bufs["pinned"][b] = torch.empty(batch.nbytes + batch.nbytes // 4, dtype=torch.uint8).pin_memory()
        if bufs["status"][b] is None or bufs["status"][b].numel() < 2 * nseg:       # statuses, then seg_info
            bufs["status"][b] = torch.empty(2 * (nseg + nseg // 4 + 64), dtype=torch.int32).pin_memory()
        batch.fill(bufs["pinned"][b].numpy())
        with torch.cuda.stream(side):
            if bufs["d_buf"] is None or bufs["d_buf"].numel() < batch.nbytes:
                # in order on the side stream, so one device buffer serves every chunk (allocated under that stream: a
                # replaced one is not handed out again before the work queued on it is done)
                bufs["d_buf"] = torch.empty(batch.nbytes + batch.nbytes // 4, dtype=torch.uint8, device=device)
            d_buf = bufs["d_buf"]
            d_buf[:batch.nbytes].copy_(bufs["pinned"][b][:batch.nbytes], non_blocking=True)
            if nseg:
                d_status = torch.empty(2 * nseg, dtype=torch.int32, device=device)
                ws_bytes = split_workspace_bytes(batch.total, nseg)
                if bufs["d_ws"] is None or bufs["d_ws"].numel() * 8 < ws_bytes:             # like d_buf: one, in order on the side stream
                    bufs["d_ws"] = torch.empty((ws_bytes + ws_bytes // 4) // 8 + 1, dtype=torch.int64, device=device)
                # the segment lengths are known here: a chunk without a long segment does not queue the rounds at all
                seg = batch.plan.segments
                longest = int((seg["end"].astype(np.int64) - seg["begin"]).max())
                batch.launch_split(d_buf, bufs["d_coef"], d_status[:nseg], d_status[nseg:], bufs["d_ws"], geom, side.cuda_stream,
                                   min_split_bytes=min_split if longest >= min_split else 0)
                bufs["status"][b][:2 * nseg].copy_(d_status, non_blocking=True)
                # host-routed and refused frames reconstruct from cleared coefficients; finish_device overwrites their slots
                _lib.check(lib.tstar_jpeg_reconstruct(bufs["d_coef"].data_ptr(), d_buf.data_ptr() + batch.parts["quant"][0], n, *geom,
                                                      bufs["planes"].data_ptr(), store[s0:s0 + n].data_ptr(), side.cuda_stream),
                           "tstar_jpeg_reconstruct")
            done[b] = torch.cuda.Event(blocking=True)            # the wait in finish_device sleeps: the CPU is what this mode saves
            done[b].record(side)
        pending.append((s0, idx, datas, b, batch))

    def finish_device():
        """Read one launched chunk's statuses; every frame the device did not return OK for goes through the host decoder,
        whose verdict stands: its coefficients are reconstructed on the device, or the frame is Pillow's / an error."""
        s0, idx, datas, b, batch = pending.pop(0)
        done[b].synchronize()
        nseg = len(batch.plan.segments)
        fstat = batch.plan.frame_status(bufs["status"][b][:nseg].numpy())
        info = bufs["status"][b][nseg:2 * nseg].numpy()
        sstats["split"] += int((info != 0).sum())
        sstats["abandoned"] += int((info < 0).sum())
        sstats["rounds_max"] = max(sstats["rounds_max"], int(info.max(initial=0)))
        redo = [int(j) for j in np.nonzero(fstat)[0]]
        for j in redo:
            coef1 = torch.empty((1, bufs["blocks"] * 64), dtype=torch.int16)
            quant1 = torch.empty((1, 192), dtype=torch.int16)
            st1, msg = entropy_batch([datas[j]], geom, coef1.numpy(), quant1.numpy().view(np.uint16), 1)
            estats["host"] += 1
            with torch.cuda.stream(side):
                if st1[0] == OK:
                    dc, dq = coef1.to(device), quant1.to(device)
                    _lib.check(lib.tstar_jpeg_reconstruct(dc.data_ptr(), dq.data_ptr(), 1, *geom, bufs["planes"].data_ptr(),
                                                          store[s0 + j:s0 + j + 1].data_ptr(), side.cuda_stream), "tstar_jpeg_reconstruct")
                    stats["device"] += 1
                else:
                    store[s0 + j].copy_(torch.from_numpy(fallback_rgb(datas[j], src.label(idx[j]), int(st1[0]), msg)))
                    stats["pillow"] += 1
        stats["device"] += len(idx) - len(redo)
        estats["device"] += len(idx) - len(redo)

    s0, ci = 0, 0
    step = chunk if chunk else None
    try:
        while s0 < n_sec:
            if geom is None:
                # no covered frame seen yet: look one frame ahead at a time (each goes to Pillow until one is covered)
                data = first if s0 == 0 else src.read(want[s0])
                rc, info, msg = probe(data)
                if rc == OK:
                    if (info[0], info[1]) != (W, H):
                        raise ValueError(f"Cannot open video file: {src.label(want[s0])} is {info[0]}x{info[1]}, the first frame is {W}x{H}")
                    geom = info
                    bufs = alloc(geom)
                    step = bufs["chunk"]
                    continue
                if rc == MALFORMED:
                    raise ValueError(f"Cannot open video file: {src.label(want[s0])} ({msg})")
                arr = _pillow_rgb(data, src.label(want[s0]))
                if arr.shape != (H, W, 3):
                    raise ValueError(f"Cannot open video file: {src.label(want[s0])} is {arr.shape[1]}x{arr.shape[0]}, the first frame is {W}x{H}")
                store[s0].copy_(torch.from_numpy(arr))
                stats["pillow"] += 1
                s0 += 1
                continue
            idx = want[s0:s0 + step]
            n = len(idx)
            b = ci & 1 if on_gpu else 0
            if dev_entropy:
                datas = [first if (s0 + j == 0) else src.read(fi) for j, fi in enumerate(idx)]
                n = device_entropy_take([len(d) for d in datas])
                idx, datas = idx[:n], datas[:n]
                submit_device(s0, idx, datas, b)          # the host plans the next chunk while this one runs
                if len(pending) > 1:
                    finish_device()
                s0 += n
                ci += 1
                continue
            if on_gpu and done[b] is not None:
                done[b].synchronize()                     # the pinned buffers' previous copy has left
            datas = [first if (s0 + j == 0) else src.read(fi) for j, fi in enumerate(idx)]
            coef, quant = bufs["coef"][b], bufs["quant"][b]
            status, _ = entropy_batch(datas, geom, coef.numpy(), quant.numpy().view(np.uint16), threads)
            fallback = [(int(j), fallback_rgb(datas[int(j)], src.label(idx[int(j)]), int(status[int(j)]))) for j in np.nonzero(status)[0]]
            estats["host"] += n
            if on_gpu:
                with torch.cuda.stream(side):
                    bufs["d_coef"][b][:n].copy_(coef[:n], non_blocking=True)
                    bufs["d_quant"][b][:n].copy_(quant[:n], non_blocking=True)
                    _lib.check(lib.tstar_jpeg_reconstruct(bufs["d_coef"][b].data_ptr(), bufs["d_quant"][b].data_ptr(), n, *geom,
                                                          bufs["planes"].data_ptr(), store[s0:s0 + n].data_ptr(), side.cuda_stream),
                               "tstar_jpeg_reconstruct")
                    done[b] = torch.cuda.Event()
                    done[b].record(side)
                    for j, arr in fallback:               # after the kernels, which wrote whatever the stale coefficients gave into these slots
                        store[s0 + j].copy_(torch.from_numpy(arr))
            else:
                out = store[s0:s0 + n].numpy()
                _lib.check(lib.tstar_jpeg_reconstruct_host(coef.data_ptr(), quant.data_ptr(), n, *geom, out.ctypes.data, threads),
                           "tstar_jpeg_reconstruct_host")
                for j, arr in fallback:
                    out[j] = arr
            stats["device" if on_gpu else "host"] += n - len(fallback)
            stats["pillow"] += len(fallback)
            s0 += n
            ci += 1
        while pending:
            finish_device()
    finally:
        # also on the way out with an error: the side stream may still be writing the previous chunk into the store, the
        # planes and the staged coefficients, and the allocator must not hand those blocks out before it is done
        if side is not None:
            side.synchronize()
    st = FrameStore(store, src.fps, src.n_frames, name=src.name)
    st.decode_stats = stats
    st.entropy_stats = estats
    st.entropy_split_stats = sstats
    return st
