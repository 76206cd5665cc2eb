"""Baseline JPEG encode of resident frames: the bytes ``PIL.Image.fromarray(frame).save(buf, "JPEG", quality=q,
subsampling=s)`` writes, for quality 1..100 and subsampling 4:2:0 / 4:2:2 / 4:4:4 (csrc/jpeg_enc.hip on the device,
csrc/jpeg_enc_host.cpp on the host).  ``restart_rows=`` / ``restart_blocks=`` on every entry are Pillow's
``restart_marker_rows=`` / ``restart_marker_blocks=``: a DRI segment and RSTn markers, which cut a scan into pieces the device
decoder takes one lane each.  ``optimize=True`` on every entry is Pillow's ``optimize=True``: each frame is coded with four Huffman
tables built from its own symbol counts, and its header carries them.

The reference's exits are JPEG: ``encode_image_to_base64`` (TStar/utilites.py:15-37) for the grounding frames and the QA
keyframes, ``.jpg`` files for the keyframes (TStarFramework.py:136-146).  Here the frames never leave HBM as pixels: the
kernels turn them into scans, one read of the lengths per chunk brings the bytes over, the header (the same for every frame
of a call) is joined on the host.  ``save_mjpeg`` writes a store as Motion-JPEG, which ``open_video`` reads back through
the device decode path.
"""
from __future__ import annotations

import base64
import ctypes as C
import operator
import os
import struct
from typing import List, Optional, Sequence

import numpy as np

SUBSAMPLINGS = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:4": (1, 1)}
_PIL_SUBSAMPLING = {0: "4:4:4", 1: "4:2:2", 2: "4:2:0"}
STATUS_OK, STATUS_SHORT, STATUS_BAD_COEF, STATUS_HUFF_OVERFLOW = 0, 1, 2, 3
HUFF_OK, HUFF_CLEN_OVERFLOW, HUFF_EMPTY = 0, 1, 2      # status of one table
SPEC_BYTES = 276               # a table as the ABI hands it out: bits u8 [16], vals u8 [256], nvals u16, status u16
SPEC_DTYPE = np.dtype([("bits", np.uint8, 16), ("vals", np.uint8, 256), ("nvals", np.uint16), ("status", np.uint16)])
HIST_BINS = 257                # 256 symbols and the reserved one (always 0 in a histogram)
DHT_IDS = (0x00, 0x10, 0x01, 0x11)                     # DC 0, AC 0, DC 1, AC 1: the order of the segments and of every [4] here
HEADER_DHT_AT, HEADER_DHT_END = 177, 609               # the four standard DHT segments inside ``header()``'s bytes
COUNTERS = ("zrl", "no_eob", "stuffed", "dummy_right", "dummy_bottom")
RESTART_COUNTERS = ("rst", "pad_free", "pad_ff")        # markers; intervals that ended byte-aligned; padded bytes that became 0xFF
RESTART_LIMIT = 65535          # MCUs per interval: what the 16 bits of DRI hold
AVI_LIMIT = 1 << 30            # a RIFF AVI of this size or more needs OpenDML index segments, which nobody here writes or reads


def sampling(subsampling) -> tuple:
    """"4:2:0" / "4:2:2" / "4:4:4" (or Pillow's 2 / 1 / 0) -> the luma sampling factors (hs, vs)."""
    s = _PIL_SUBSAMPLING.get(subsampling, subsampling)
    if s not in SUBSAMPLINGS:
        raise ValueError(f"JPEG subsampling {subsampling!r}: expected one of {tuple(SUBSAMPLINGS)}")
    return SUBSAMPLINGS[s]


def _quality(quality) -> int:
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality {quality!r}: expected 1..100")
    return q


def restart_interval(W: int, H: int, subsampling="4:2:0", restart_rows=None, restart_blocks=None) -> int:
    """Pillow's ``restart_marker_rows`` / ``restart_marker_blocks`` -> MCUs per restart interval (0: no DRI, no markers).  Rows
    count MCU rows and win over blocks (MCUs) when both are given; 0 / None mean "not given".  A negative or non-integer value,
    and an interval above 65535 MCUs, raise ValueError: DRI holds 16 bits (libjpeg itself clamps rows to 65535 MCUs and writes
    the low 16 bits of a larger block count into DRI while it places the markers by the full count, a file no decoder follows)."""
    rows, blocks = _restart_values(restart_rows, restart_blocks)
    hs, _ = sampling(subsampling)
    interval = rows * ((int(W) + 8 * hs - 1) // (8 * hs)) if rows else blocks
    if interval > RESTART_LIMIT:
        raise ValueError(f"JPEG restart interval of {interval} MCUs: DRI holds at most {RESTART_LIMIT}")
    return interval


def _restart_values(restart_rows, restart_blocks) -> tuple:
    """The two keywords as non-negative ints (None -> 0); what can be refused without knowing the picture is refused here."""
    vals = []
    for name, v in (("restart_rows", restart_rows), ("restart_blocks", restart_blocks)):
        if v is None:
            v = 0
        try:
            if isinstance(v, bool):
                raise TypeError
            v = operator.index(v)
        except TypeError:
            raise ValueError(f"JPEG {name} {v!r}: expected a non-negative integer") from None
        if v < 0:
            raise ValueError(f"JPEG {name} {v!r}: expected a non-negative integer")
        vals.append(v)
    rows, blocks = vals
    if (rows or blocks) > RESTART_LIMIT:               # a row is at least one MCU
        raise ValueError(f"JPEG restart interval of {rows or blocks} MCUs or more: DRI holds at most {RESTART_LIMIT}")
    return rows, blocks


class Plan:
    """tstar_jpeg_encode_plan_opt: sizes and launch shape for n frames of W x H whose scans go into slots of slot_bytes.  With
    ``restart`` (MCUs per interval; 0: none) the bounds hold the markers and the padding, and ``markers`` is their number per
    frame.  With ``optimize`` a block's bound is 1665 bits, ``header_bytes`` is the LONGEST header and the workspace holds the symbol
    counts (at ``off_hist``) and the code tables (at ``off_codes``); without it the values are tstar_jpeg_encode_plan_rst's."""
    FIELDS = ("blocks", "coef_bytes", "max_scan_bytes", "header_bytes", "workspace_bytes", "block_wgs", "entropy_wgs_x", "stuff_wgs_x")

    def __init__(self, W: int, H: int, hs: int, vs: int, n: int = 1, slot_bytes: int = 2, restart: int = 0, optimize: bool = False):
        from . import _lib
        out, out2, out3 = (C.c_size_t * 8)(), (C.c_size_t * 2)(), (C.c_size_t * 3)()
        _lib.check(_lib.load().tstar_jpeg_encode_plan_opt(W, H, hs, vs, n, slot_bytes, restart, 1 if optimize else 0, out, out2, out3),
                   "tstar_jpeg_encode_plan_opt")
        self.optimize, self.off_hist, self.off_codes = bool(optimize), int(out3[1]), int(out3[2])
        self.restart, self.markers = int(restart), int(out2[1])
        for k, v in zip(self.FIELDS, out):
            setattr(self, k, int(v))


def header(W: int, H: int, quality: int = 75, subsampling="4:2:0", restart_rows=None, restart_blocks=None) -> bytes:
    """SOI .. SOS as Pillow writes them from an array (with a restart interval: DRI directly before SOS)."""
    from . import _lib
    hs, vs = sampling(subsampling)
    restart = restart_interval(W, H, subsampling, restart_rows, restart_blocks)
    buf = np.empty(1024, dtype=np.uint8)
    n = C.c_size_t(0)
    _lib.check(_lib.load().tstar_jpeg_encode_header_rst(W, H, _quality(quality), hs, vs, restart, buf.ctypes.data, buf.size, C.byref(n)),
               "tstar_jpeg_encode_header_rst")
    return buf[:n.value].tobytes()


def header_from_tables(W: int, H: int, quant, subsampling="4:2:0", restart: int = 0) -> bytes:
    """SOI .. SOS in the layout of ``header`` with the DQT entries given: ``quant`` [3][64] in natural order (rows Y / Cb / Cr, as
    the decoder reports a file's tables), values 1..65535.  Equal chroma rows share table 1 (what ``header`` writes), else Cr takes a
    table 2 of its own; a table with a value above 255 is written with 16-bit entries and the frame header becomes SOF1, as libjpeg
    writes it.  ``restart``: MCUs per interval (0: no DRI).  For the tables of a Pillow quality q the bytes are ``header(W, H, q,
    subsampling, restart_blocks=restart)``'s: a file re-coded under it keeps its own quantisation, so not a pixel changes."""
    from . import _lib
    hs, vs = sampling(subsampling)
    _, restart = _restart_values(None, restart)
    q = np.ascontiguousarray(quant, dtype=np.int64).reshape(-1)
    if q.size != 192 or q.min() < 1 or q.max() > 65535:
        raise ValueError("header_from_tables: expected quantisation tables [3][64] of values 1..65535")
    q = q.astype(np.uint16)
    buf = np.empty(1024, dtype=np.uint8)
    n = C.c_size_t(0)
    _lib.check(_lib.load().tstar_jpeg_encode_header_tables(W, H, q.ctypes.data, hs, vs, restart, buf.ctypes.data, buf.size, C.byref(n)),
               "tstar_jpeg_encode_header_tables")
    return buf[:n.value].tobytes()


def huff_optimal(freq):
    """tstar_jpeg_huff_optimal: the table libjpeg's jpeg_gen_optimal_table builds from ``freq`` (256 counts, their sum at most 10^9)
    -> dict(bits uint8 [16], vals bytes (huffval), status HUFF_*, code uint16 [256], len uint8 [256], steps of the limiting to 16)."""
    from . import _lib
    f = np.ascontiguousarray(freq, dtype=np.int64).reshape(-1)
    if f.size != 256 or f.min() < 0 or f.sum() > 1_000_000_000:
        raise ValueError("huff_optimal: expected 256 counts >= 0 that sum to at most 1000000000")
    f = f.astype(np.uint32)
    spec = np.zeros(1, dtype=SPEC_DTYPE)
    code, ln, steps = np.zeros(256, dtype=np.uint16), np.zeros(256, dtype=np.uint8), C.c_int32(0)
    _lib.check(_lib.load().tstar_jpeg_huff_optimal(f.ctypes.data, spec.ctypes.data, code.ctypes.data, ln.ctypes.data, C.byref(steps)),
               "tstar_jpeg_huff_optimal")
    return dict(bits=spec["bits"][0].copy(), vals=spec["vals"][0, :int(spec["nvals"][0])].tobytes(), status=int(spec["status"][0]), code=code,
                len=ln, steps=int(steps.value))


def dht_segments(specs) -> bytes:
    """The four DHT segments of one frame from its specs (SPEC_DTYPE [4], DHT_IDS order), each a segment of its own."""
    out = []
    for t, sp in zip(DHT_IDS, specs):
        n = int(sp["nvals"])
        out.append(b"\xff\xc4" + struct.pack(">HB", 19 + n, t) + sp["bits"].tobytes() + sp["vals"][:n].tobytes())
    return b"".join(out)


def header_from_specs(W: int, H: int, specs, quality: int = 75, subsampling="4:2:0", restart: int = 0) -> bytes:
    """tstar_jpeg_encode_header_opt: SOI .. SOS of ONE frame coded with the tables of ``specs`` (SPEC_DTYPE [4]): ``header()``'s
    layout with these tables in its four DHT segments."""
    from . import _lib
    hs, vs = sampling(subsampling)
    _, restart = _restart_values(None, restart)
    sp = np.ascontiguousarray(specs, dtype=SPEC_DTYPE).reshape(4)
    buf = np.empty(2048, dtype=np.uint8)
    n = C.c_size_t(0)
    _lib.check(_lib.load().tstar_jpeg_encode_header_opt(W, H, _quality(quality), hs, vs, restart, sp.ctypes.data, buf.ctypes.data, buf.size,
                                                        C.byref(n)), "tstar_jpeg_encode_header_opt")
    return buf[:n.value].tobytes()


def header_from_tables_specs(W: int, H: int, quant, specs, subsampling="4:2:0", restart: int = 0) -> bytes:
    """tstar_jpeg_encode_header_tables_opt: SOI .. SOS of a file that is RE-CODED with tables of its own: ``header_from_tables``'s
    layout (the source's DQT entries ``quant`` [3][64], SOF0 or SOF1, DRI when ``restart`` > 0) with the four tables of ``specs``
    (SPEC_DTYPE [4]) in its DHT segments.  For the tables of a Pillow quality q the bytes are ``header_from_specs(W, H, specs, q,
    subsampling, restart)``'s."""
    from . import _lib
    hs, vs = sampling(subsampling)
    _, restart = _restart_values(None, restart)
    q = np.ascontiguousarray(quant, dtype=np.int64).reshape(-1)
    if q.size != 192 or q.min() < 1 or q.max() > 65535:
        raise ValueError("header_from_tables_specs: expected quantisation tables [3][64] of values 1..65535")
    q = q.astype(np.uint16)
    sp = np.ascontiguousarray(specs, dtype=SPEC_DTYPE).reshape(4)
    buf = np.empty(2048, dtype=np.uint8)
    n = C.c_size_t(0)
    _lib.check(_lib.load().tstar_jpeg_encode_header_tables_opt(W, H, q.ctypes.data, hs, vs, restart, sp.ctypes.data, buf.ctypes.data, buf.size,
                                                               C.byref(n)), "tstar_jpeg_encode_header_tables_opt")
    return buf[:n.value].tobytes()


def _check_tables(specs) -> None:
    """A table whose code sizes overflow is an error, never a fall-back to the standard tables."""
    if (np.asarray(specs["status"]) != HUFF_OK).any():
        raise ValueError("JPEG encode (optimize): Huffman code length overflow: a code of a frame's optimal table is longer than 32 bits")


def _host_array(frames) -> np.ndarray:
    a = np.ascontiguousarray(frames)
    if a.ndim == 3:
        a = a[None]
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or 0 in a.shape:
        raise ValueError("encode_frames: expected uint8 frames [n,H,W,3] (or one [H,W,3])")
    return a


def blocks_host(frames, quality: int = 75, subsampling="4:2:0", idx: Optional[Sequence[int]] = None, threads: int = 0, counters=None):
    """Block stage of the host twin -> (coef int16 [n, blocks * 64], quant uint16 [3, 64])."""
    from . import _lib
    a = _host_array(frames)
    hs, vs = sampling(subsampling)
    N, H, W, _ = a.shape
    ii = np.ascontiguousarray(np.arange(N) if idx is None else idx, dtype=np.int32)
    p = Plan(W, H, hs, vs, len(ii))
    coef = np.empty((len(ii), p.blocks * 64), dtype=np.int16)
    quant = np.empty((3, 64), dtype=np.uint16)
    _lib.check(_lib.load().tstar_jpeg_encode_blocks_host(a.ctypes.data, N, H, W, ii.ctypes.data, len(ii), _quality(quality), hs, vs,
                                                         coef.ctypes.data, quant.ctypes.data, threads, _counter_ptr(counters)),
               "tstar_jpeg_encode_blocks_host")
    return coef, quant


def scan_host(coef: np.ndarray, W: int, H: int, subsampling="4:2:0", slot_bytes: Optional[int] = None, threads: int = 0, counters=None,
              restart_rows=None, restart_blocks=None, restart_counters=None, optimize: bool = False, tables: Optional[dict] = None):
    """Scan stage of the host twin: coef int16 [n, blocks * 64] -> (list of scans (None where the status is not 0), lengths, status).
    ``restart_counters``: uint64 [3] (RESTART_COUNTERS), added to.  ``optimize``: every frame coded with its own tables; ``tables``
    (optional dict) then receives ``specs`` (SPEC_DTYPE [n, 4]) and ``hist`` (uint32 [n, 4, 257], the symbol counts)."""
    from . import _lib
    hs, vs = sampling(subsampling)
    restart = restart_interval(W, H, subsampling, restart_rows, restart_blocks)
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    n = coef.shape[0]
    p = Plan(W, H, hs, vs, n, restart=restart, optimize=optimize)
    assert coef.size == n * p.blocks * 64, "coefficients do not match the geometry"
    slot = p.max_scan_bytes if slot_bytes is None else int(slot_bytes)
    out = np.empty((n, slot), dtype=np.uint8)
    lengths = np.zeros(n, dtype=np.uint32)
    status = np.full(n, -1, dtype=np.int32)
    entry, own = "tstar_jpeg_encode_scan_host_rst", ()
    if optimize:                                        # the _opt entry takes the frames' tables and counts behind the statuses
        specs = np.zeros((n, 4), dtype=SPEC_DTYPE)
        hist = np.zeros((n, 4, HIST_BINS), dtype=np.uint32)
        entry, own = "tstar_jpeg_encode_scan_host_opt", (specs.ctypes.data, hist.ctypes.data)
    _lib.check(getattr(_lib.load(), entry)(coef.ctypes.data, n, W, H, hs, vs, restart, out.ctypes.data, slot, lengths.ctypes.data,
                                           status.ctypes.data, *own, threads, _counter_ptr(counters),
                                           _counter_ptr(restart_counters, RESTART_COUNTERS)), entry)
    if optimize and tables is not None:
        tables.update(specs=specs, hist=hist)
    return [out[i, :lengths[i]].tobytes() if status[i] == 0 else None for i in range(n)], lengths, status


def _counter_ptr(counters, names=COUNTERS):
    if counters is None:
        return None
    assert isinstance(counters, np.ndarray) and counters.dtype == np.uint64 and counters.size == len(names)
    return counters.ctypes.data


def encode_host(frames, quality: int = 75, subsampling="4:2:0", idx: Optional[Sequence[int]] = None, slot_bytes: Optional[int] = None,
                threads: int = 0, counters=None, out: Optional[np.ndarray] = None, restart_rows=None, restart_blocks=None,
                restart_counters=None, optimize: bool = False):
    """Whole files from the host twin -> (out uint8 [n, slot_bytes], lengths, status).  ``slot_bytes`` defaults to what holds any
    file of the geometry; ``out`` may be a caller's buffer of at least n * slot_bytes bytes (the capacity tests pass one).
    ``optimize``: Pillow's ``optimize=True``; a frame whose tables overflow has status STATUS_HUFF_OVERFLOW."""
    from . import _lib
    a = _host_array(frames)
    hs, vs = sampling(subsampling)
    N, H, W, _ = a.shape
    restart = restart_interval(W, H, subsampling, restart_rows, restart_blocks)
    ii = np.ascontiguousarray(np.arange(N) if idx is None else idx, dtype=np.int32)
    n = len(ii)
    p = Plan(W, H, hs, vs, n, restart=restart, optimize=optimize)
    slot = p.header_bytes + p.max_scan_bytes if slot_bytes is None else int(slot_bytes)
    if out is None:
        out = np.empty((n, slot), dtype=np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= n * slot
    lengths = np.zeros(n, dtype=np.uint32)
    status = np.full(n, -1, dtype=np.int32)
    entry = "tstar_jpeg_encode_host_opt" if optimize else "tstar_jpeg_encode_host_rst"
    _lib.check(getattr(_lib.load(), entry)(a.ctypes.data, N, H, W, ii.ctypes.data, n, _quality(quality), hs, vs, restart,
                                           out.ctypes.data, slot, lengths.ctypes.data, status.ctypes.data, threads,
                                           _counter_ptr(counters), _counter_ptr(restart_counters, RESTART_COUNTERS)), entry)
    return out, lengths, status


def _typical_slot(W: int, H: int, p: Plan) -> int:
    """Slot of the first device pass: 3/4 byte per pixel (a quality-75 photograph takes a third of that), at least 4 KiB, never
    more than what holds any scan.  Frames that do not fit are encoded again into slots of the bound."""
    return min(p.max_scan_bytes, max(4096, (W * H * 3 // 4 + 15) // 16 * 16))


class DeviceEncoder:
    """Buffers and launches of the device path for frames of one geometry, reused chunk after chunk."""

    def __init__(self, W: int, H: int, quality: int, subsampling, chunk: int, slot_bytes: Optional[int] = None, device=None,
                 restart: int = 0, optimize: bool = False):
        import torch
        self.W, self.H, self.quality = W, H, _quality(quality)
        self.hs, self.vs = sampling(subsampling)
        self.chunk = int(chunk)
        self.restart = int(restart)                    # MCUs per restart interval; 0: the launches of a scan without markers
        self.optimize = bool(optimize)                 # every frame coded with tables of its own; False: today's launches
        one = Plan(W, H, self.hs, self.vs, 1, restart=self.restart, optimize=self.optimize)
        self.slot = int(slot_bytes) if slot_bytes else _typical_slot(W, H, one)
        self.plan = Plan(W, H, self.hs, self.vs, self.chunk, self.slot, self.restart, self.optimize)
        self.max_scan_bytes = one.max_scan_bytes
        self.device = device
        u8 = dict(dtype=torch.uint8, device=device)
        self.coef = torch.empty(self.chunk * self.plan.coef_bytes, **u8)
        self.work = torch.empty(self.plan.workspace_bytes, **u8)
        self.out = torch.empty((self.chunk, self.slot), **u8)
        self.meta = torch.empty((2, self.chunk), dtype=torch.int32, device=device)      # lengths (u32 bits), status
        self.rst = torch.zeros((self.chunk, len(RESTART_COUNTERS)), dtype=torch.int32, device=device) if self.restart else None
        self.restart_counts = np.zeros(len(RESTART_COUNTERS), dtype=np.int64)           # summed by collect()
        self.specs = torch.zeros((self.chunk, 4 * SPEC_BYTES), **u8) if self.optimize else None
        self.table_ms = 0.0
        self.block_ms = self.entropy_ms = 0.0
        self.timed = False

    def launch(self, frames, idx) -> None:
        """Both stages for frames[idx] (idx: int32 device tensor, at most ``chunk`` long); nothing is read back."""
        import torch
        from . import _lib
        lib = _lib.load()
        n = int(idx.numel())
        N = int(frames.shape[0])
        s = _lib.stream_ptr()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if self.timed else None
        if ev:
            ev[0].record()
        _lib.check(lib.tstar_jpeg_encode_blocks(frames.data_ptr(), N, self.H, self.W, idx.data_ptr(), n, self.quality, self.hs, self.vs,
                                                self.coef.data_ptr(), None, s), "tstar_jpeg_encode_blocks")
        if ev:
            ev[1].record()
        if self.optimize:
            _lib.check(lib.tstar_jpeg_encode_scan_opt(self.coef.data_ptr(), n, self.W, self.H, self.hs, self.vs, self.restart,
                                                      self.out.data_ptr(), self.slot, self.meta[0].data_ptr(), self.meta[1].data_ptr(),
                                                      self.specs.data_ptr(), self.work.data_ptr(), self.work.numel(), _lib.ptr(self.rst), s),
                       "tstar_jpeg_encode_scan_opt")
        else:
            _lib.check(lib.tstar_jpeg_encode_scan_rst(self.coef.data_ptr(), n, self.W, self.H, self.hs, self.vs, self.restart,
                                                      self.out.data_ptr(), self.slot, self.meta[0].data_ptr(), self.meta[1].data_ptr(),
                                                      self.work.data_ptr(), self.work.numel(), _lib.ptr(self.rst), s),
                       "tstar_jpeg_encode_scan_rst")
        if ev:
            ev[2].record()
            ev[2].synchronize()
            self.block_ms += ev[0].elapsed_time(ev[1])
            self.entropy_ms += ev[1].elapsed_time(ev[2])

    def collect(self, n: int):
        """ONE device -> host read of lengths and status (with a restart interval a second one, of the counters; with optimised tables
        one more, of the frames' specs, kept in ``last_specs``), then the used bytes of the slots in one copy -> (list of scans (None
        where the slot was short), status)."""
        import torch
        meta = self.meta[:, :n].cpu().numpy()
        lengths, status = meta[0].view(np.uint32).astype(np.int64), meta[1]
        if (status == STATUS_BAD_COEF).any():
            raise ValueError("JPEG encode: a coefficient outside 8-bit baseline JPEG")
        if self.optimize:
            self.last_specs = self.specs[:n].cpu().numpy().view(SPEC_DTYPE).reshape(n, 4)
            _check_tables(self.last_specs)
        if self.rst is not None:                       # the frames that were written: a short frame is counted when it is encoded again
            self.restart_counts += self.rst[:n].cpu().numpy().astype(np.int64)[status == STATUS_OK].sum(axis=0)
        take = np.where(status == STATUS_OK, lengths, 0)
        cols = torch.arange(self.slot, device=self.out.device)[None, :]
        used = self.out[:n][cols < torch.as_tensor(take, device=self.out.device)[:, None]].cpu().numpy()
        ends = np.cumsum(take)
        return [used[e - t:e].tobytes() if st == STATUS_OK else None for e, t, st in zip(ends, take, status)], status


def encode_chunk_size(blocks: int, n_frames: int, chunk: Optional[int] = None) -> int:
    """Frames per chunk: the coefficient buffer's budget and frame limit of the decoder's device entropy path."""
    from . import jpeg
    return jpeg.device_entropy_chunk(blocks, n_frames, chunk)


def _encode_device(frames, idx, quality, subsampling, chunk=None, slot_bytes=None, stats=None, restart: int = 0,
                   optimize: bool = False) -> List[bytes]:
    """frames: cuda uint8 [N,H,W,3]; idx: int32 cuda tensor of frame numbers -> the JPEG files.  restart: MCUs per interval.
    optimize: every frame's header is joined from the shared bytes in front of the DHT segments, the frame's four segments and the
    shared DRI / SOS behind them."""
    import torch
    N, H, W, _ = (int(v) for v in frames.shape)
    hs, vs = sampling(subsampling)
    n = int(idx.numel())
    if n == 0:
        return []
    head = header(W, H, quality, subsampling, restart_blocks=restart)
    one = Plan(W, H, hs, vs, 1, restart=restart, optimize=optimize)
    counts = np.zeros(len(RESTART_COUNTERS), dtype=np.int64)
    dhts: List[Optional[bytes]] = [None] * n           # optimize: every frame's four DHT segments
    with torch.cuda.device(frames.device):
        enc = DeviceEncoder(W, H, quality, subsampling, encode_chunk_size(one.blocks, n, chunk), slot_bytes, frames.device, restart, optimize)
        enc.timed = stats is not None
        out: List[Optional[bytes]] = []
        short: List[int] = []
        for s0 in range(0, n, enc.chunk):
            part = idx[s0:s0 + enc.chunk]
            enc.launch(frames, part)
            scans, status = enc.collect(int(part.numel()))
            short += [s0 + int(i) for i in np.nonzero(status == STATUS_SHORT)[0]]
            out += scans
            if optimize:
                dhts[s0:s0 + len(scans)] = [dht_segments(sp) for sp in enc.last_specs]
        if stats is not None:
            stats["block_ms"] = stats.get("block_ms", 0.0) + enc.block_ms
            stats["entropy_ms"] = stats.get("entropy_ms", 0.0) + enc.entropy_ms
            stats["retried"] = stats.get("retried", 0) + len(short)
        counts += enc.restart_counts
        if short:
            if enc.slot >= enc.max_scan_bytes:
                raise RuntimeError("JPEG encode: a scan did not fit the bound of its geometry")
            del enc
            # frames the typical slot was short of: once more into slots that hold any scan, a few at a time
            step = max(1, min(len(short), (256 << 20) // one.max_scan_bytes))
            big = DeviceEncoder(W, H, quality, subsampling, step, one.max_scan_bytes, frames.device, restart, optimize)
            for s0 in range(0, len(short), step):
                ids = short[s0:s0 + step]
                big.launch(frames, idx[torch.as_tensor(ids, device=idx.device, dtype=torch.long)])
                scans, status = big.collect(len(ids))
                if (status != STATUS_OK).any():
                    raise RuntimeError("JPEG encode: a scan did not fit the bound of its geometry")
                for j, (i, sc) in enumerate(zip(ids, scans)):
                    out[i] = sc
                    if optimize:
                        dhts[i] = dht_segments(big.last_specs[j])
            counts += big.restart_counts
    if stats is not None and restart:
        for k, v in zip(RESTART_COUNTERS, counts):
            stats[k] = stats.get(k, 0) + int(v)
    if not optimize:
        return [head + sc for sc in out]
    if stats is not None:
        stats["optimized"] = stats.get("optimized", 0) + n
        stats["table_bytes"] = stats.get("table_bytes", 0) + sum(len(d) for d in dhts)
    return [head[:HEADER_DHT_AT] + d + head[HEADER_DHT_END:] + sc for d, sc in zip(dhts, out)]


def encode_frames(frames, quality: int = 75, subsampling="4:2:0", device: bool = True, chunk: Optional[int] = None,
                  slot_bytes: Optional[int] = None, stats: Optional[dict] = None, threads: int = 0, restart_rows=None,
                  restart_blocks=None, optimize: bool = False) -> List[bytes]:
    """One JPEG file per frame, byte for byte Pillow's ``Image.fromarray(frame).save(buf, "JPEG", quality=, subsampling=,
    restart_marker_rows=restart_rows, restart_marker_blocks=restart_blocks, optimize=optimize)``.

    ``frames``: a cuda uint8 tensor [n,H,W,3], or ``(store, secs)`` -- a FrameStore (RGB or NV12) and the logical seconds wanted,
    read straight from the store through the index list.  ``device=False``: the host twin on a numpy array [n,H,W,3] (the
    fallback a caller without a device can choose; there is no silent one).  ``chunk`` / ``slot_bytes`` override the device
    path's frames per chunk and per-frame scan capacity (frames a slot is short of are encoded again at the bound).
    ``restart_rows`` / ``restart_blocks``: a restart interval of that many MCU rows / MCUs (``restart_interval``; default none);
    with ``stats`` the device path adds the RESTART_COUNTERS of the files it wrote.  ``optimize=True``: Huffman tables built from each
    frame's own symbol counts (smaller files, the same pixels); ``stats`` then gains ``optimized`` (frames) and ``table_bytes`` (bytes
    of their DHT segments).  A table whose code sizes overflow raises ValueError; there is no fall-back to the standard tables."""
    quality = _quality(quality)
    optimize = bool(optimize)
    sampling(subsampling)
    _restart_values(restart_rows, restart_blocks)      # the values themselves, before anything is touched
    if isinstance(frames, tuple) and len(frames) == 2 and hasattr(frames[0], "fmt"):
        store, secs = frames
        restart = restart_interval(store.shape[2], store.shape[1], subsampling, restart_rows, restart_blocks)
        if not device:
            return encode_frames(store.host_frames(secs), quality, subsampling, device=False, threads=threads, restart_blocks=restart,
                                 optimize=optimize)
        return _encode_store(store, secs, quality, subsampling, chunk, slot_bytes, stats, restart, optimize)
    if not device:
        a = _host_array(frames)
        out, lengths, status = encode_host(a, quality, subsampling, threads=threads, restart_rows=restart_rows, restart_blocks=restart_blocks,
                                           optimize=optimize)
        if (status == STATUS_HUFF_OVERFLOW).any():
            raise ValueError("JPEG encode (optimize): Huffman code length overflow: a code of a frame's optimal table is longer than 32 bits")
        if (status != STATUS_OK).any():
            raise RuntimeError(f"JPEG encode (host): status {status.tolist()}")
        return [out[i, :lengths[i]].tobytes() for i in range(len(a))]
    import torch
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4
            and frames.shape[3] == 3):
        raise ValueError("encode_frames: expected a cuda uint8 tensor [n,H,W,3] or (store, secs); pass device=False for numpy frames")
    if 0 in frames.shape[1:]:
        raise ValueError("encode_frames: empty frames")
    restart = restart_interval(int(frames.shape[2]), int(frames.shape[1]), subsampling, restart_rows, restart_blocks)
    frames = frames.contiguous()
    idx = torch.arange(frames.shape[0], dtype=torch.int32, device=frames.device)
    return _encode_device(frames, idx, quality, subsampling, chunk, slot_bytes, stats, restart, optimize)


def _encode_store(store, secs, quality, subsampling, chunk, slot_bytes, stats, restart: int = 0, optimize: bool = False) -> List[bytes]:
    import torch
    from . import _lib
    N, H, W, _ = store.shape
    secs = [int(s) for s in secs]
    for s in secs:
        if not 0 <= s < N:
            raise IndexError(f"second {s} outside the store's 0..{N - 1}")
    dev = store.device
    if store.fmt == "rgb":
        # a compressed-resident store hands out at most its pool per lease: encode pool-sized runs
        step = max(1, min(len(secs), store.lease_frames or len(secs)))
        out: List[bytes] = []
        for s0 in range(0, len(secs), step):
            lease = store.lease(secs[s0:s0 + step])
            try:
                out += _encode_device(lease.frames, lease.idx, quality, subsampling, chunk, slot_bytes, stats, restart, optimize)
            finally:
                lease.done()
        return out
    idx = torch.as_tensor(secs, dtype=torch.int32, device=dev)
    # NV12: converted chunk by chunk with the kernel host_frames uses, so the bytes are Pillow's encode of host_frames(secs)
    out = []
    step = max(1, min(len(secs), 256, (256 << 20) // (H * W * 3)))
    with torch.cuda.device(dev):
        rgb = torch.empty((step, H, W, 3), dtype=torch.uint8, device=dev)
        for s0 in range(0, len(secs), step):
            part = idx[s0:s0 + step]
            m = int(part.numel())
            _lib.check(_lib.load().tstar_nv12_to_rgb(store.frames.data_ptr(), N, H, W, part.data_ptr(), m, rgb.data_ptr(),
                                                      _lib.stream_ptr()), "tstar_nv12_to_rgb")
            out += _encode_device(rgb, torch.arange(m, dtype=torch.int32, device=dev), quality, subsampling, chunk, slot_bytes, stats, restart,
                                  optimize)
    return out


def frames_to_base64(store, secs=None, quality: int = 75, subsampling="4:2:0", restart_rows=None, restart_blocks=None,
                     optimize: bool = False) -> List[str]:
    """The reference's ``encode_image_to_base64`` (TStar/utilites.py:15-37: Pillow's default JPEG, base64, utf-8) for frames that
    never left HBM as pixels.  ``store``: a FrameStore with ``secs``, or frames as ``encode_frames`` takes them (a numpy array
    goes through the host twin).  ``optimize=True`` (Pillow's ``optimize=True``) makes the payloads smaller, not different in a pixel."""
    rst = dict(restart_rows=restart_rows, restart_blocks=restart_blocks, optimize=optimize)
    if secs is not None:
        files = encode_frames((store, secs), quality, subsampling, **rst)
    elif isinstance(store, np.ndarray):
        files = encode_frames(store, quality, subsampling, device=False, **rst)
    else:
        files = encode_frames(store, quality, subsampling, **rst)
    return [base64.b64encode(f).decode("utf-8") for f in files]


# ------------------------------------------------------------------------------------------------ containers
def avi_bytes(frame_lengths: Sequence[int]) -> int:
    """Size of the RIFF AVI ``write_avi`` makes of frames of these lengths (no file is written)."""
    movi = 4 + sum(8 + n + (n & 1) for n in frame_lengths)
    return 12 + (8 + _HDRL_BYTES) + (8 + movi) + (8 + 16 * len(frame_lengths))


_HDRL_BYTES = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))


def check_avi_size(frame_lengths: Sequence[int], path: str = "") -> int:
    total = avi_bytes(frame_lengths)
    if total >= AVI_LIMIT:
        raise ValueError(f"save_mjpeg: {path or 'the file'} would take {total} bytes; a RIFF AVI of 1 GiB or more needs OpenDML "
                         "segments, which are not written (nor read) here: save it as .mjpeg instead")
    return total


def _fps_fraction(fps: float):
    from fractions import Fraction
    fr = Fraction(float(fps)).limit_denominator(1_000_000)
    if fr <= 0 or fr.numerator >= 1 << 31:
        raise ValueError(f"save_mjpeg: frame rate {fps!r} cannot be written")
    return fr.numerator, fr.denominator            # dwRate, dwScale


def write_avi(path: str, files: Sequence[bytes], W: int, H: int, fps: float = 1.0) -> None:
    """A RIFF AVI with one ``MJPG`` video stream: ``hdrl`` (``avih``, ``strl`` = ``strh`` + ``strf``), ``movi`` with one ``00dc``
    chunk per frame, ``idx1`` -- what ``jpeg.avi_mjpeg`` parses."""
    lens = [len(f) for f in files]
    total = check_avi_size(lens, path)
    n = len(files)
    rate, scale = _fps_fraction(fps)
    biggest = max(lens) if lens else 0
    avih = struct.pack("<14I", int(round(1e6 * scale / rate)), 0, 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)       # AVIF_HASINDEX
    strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh \
        + b"strf" + struct.pack("<I", len(strf)) + strf
    hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
    assert len(hdrl) == _HDRL_BYTES, len(hdrl)
    movi_size = 4 + sum(8 + m + (m & 1) for m in lens)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI ")
        f.write(b"LIST" + struct.pack("<I", len(hdrl)) + hdrl)
        f.write(b"LIST" + struct.pack("<I", movi_size) + b"movi")
        index, off = [], 4                                         # idx1 offsets count from the 'movi' fourcc
        for data in files:
            f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b""))
            index.append(struct.pack("<4sIII", b"00dc", 0x10, off, len(data)))                          # AVIIF_KEYFRAME
            off += 8 + len(data) + (len(data) & 1)
        f.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(index))


def write_mjpeg_file(path: str, files: Sequence[bytes], W: int, H: int, fps: float = 1.0) -> None:
    """``.avi`` -> ``write_avi``; ``.mjpeg`` / ``.mjpg`` -> the frames one after another (``jpeg.mjpeg_stream`` reads them; such a
    stream carries no frame rate)."""
    low = os.fspath(path).lower()
    if not files:
        raise ValueError("save_mjpeg: no frames")
    if low.endswith(".avi"):
        write_avi(path, files, W, H, fps)
    elif low.endswith((".mjpeg", ".mjpg")):
        with open(path, "wb") as f:
            for data in files:
                f.write(data)
    else:
        raise ValueError(f"save_mjpeg: {path}: expected .avi, .mjpeg or .mjpg")


def save_mjpeg(store, path: str, quality: int = 90, subsampling="4:2:0", fps: Optional[float] = None, device: bool = True,
               piece: int = 1024, restart_rows=None, restart_blocks=None, optimize: bool = False) -> int:
    """Write a FrameStore (or, with ``device=False``, a numpy array [n,H,W,3]) as Motion-JPEG at its LOGICAL rate (1 frame per
    second unless ``fps`` is given), so that ``open_video(path)`` gives back a store of the same seconds.  Returns the frames
    written.  ``restart_rows`` / ``restart_blocks`` (default: none) cut every frame's scan into restart intervals, which the
    device entropy decoder of ``open_video`` takes one lane each instead of splitting one long scan.  ``optimize=True`` writes every
    frame with Huffman tables of its own; the decoders build their tables from whatever DHT a file carries."""
    rst = dict(restart_rows=restart_rows, restart_blocks=restart_blocks, optimize=optimize)
    if hasattr(store, "fmt"):
        N, H, W, _ = store.shape
        files: List[bytes] = []
        for s0 in range(0, N, piece):
            files += encode_frames((store, range(s0, min(N, s0 + piece))), quality, subsampling, device=device, **rst)
    else:
        a = _host_array(store)
        N, H, W, _ = a.shape
        files = encode_frames(a, quality, subsampling, device=False, **rst) if not device else encode_frames(store, quality, subsampling, **rst)
    write_mjpeg_file(path, files, W, H, 1.0 if fps is None else float(fps))
    return len(files)


# ------------------------------------------------------------------------------------------------ lossless re-coding
def recode_frames(files: Sequence, restart_blocks: int = 8, device: bool = True, stats: Optional[dict] = None,
                  chunk: Optional[int] = None, optimize: bool = False) -> List[bytes]:
    """Every JPEG of ``files`` (bytes or paths) with a restart interval of ``restart_blocks`` MCUs (1..65535), LOSSLESSLY: the
    quantised coefficients and the quantisation tables are the file's own, only the entropy coding is new (DRI / RSTn), so every
    decoder gives the pixels it gave before.  A file that is not re-coded comes back as it is: grayscale, progressive, arithmetic,
    CMYK, a sampling the kernels do not cover, a file the decoder does not return OK for, or a coefficient beyond the standard
    tables' size categories.  ``stats`` (optional dict) is added to: ``recoded``, ``kept``, ``bytes_in``, ``bytes_out``.
    ``optimize=False`` writes the standard Huffman tables: a source with optimised tables grows by what the optimisation had saved.
    ``optimize=True`` is ``jpegtran -optimize -restart N``: every re-coded frame is coded with four tables built from ITS OWN symbol
    counts (the procedure of ``encode_frames(optimize=True)`` on the file's coefficients) and carries them in its header; for a
    Pillow-written source the result is byte for byte Pillow's ``optimize=True, restart_marker_blocks=N`` file.  ``restart_blocks=0``
    is then allowed and means no DRI and no markers (``jpegtran -optimize``).  A frame whose optimal table would need a code longer
    than 32 bits is kept and counted, as a lossless tool returns its input.  ``stats`` then gains ``optimized`` (frames coded with
    tables of their own) and ``table_bytes`` (bytes of their DHT segments).  ``device=False``: the host twin, which needs no GPU and
    gives the same bytes."""
    from . import jpeg_recode
    optimize = bool(optimize)
    restart = jpeg_recode.recode_restart(restart_blocks, optimize)
    datas = []
    for f in files:
        if isinstance(f, (bytes, bytearray, memoryview)):
            datas.append(bytes(f))
        else:
            with open(f, "rb") as fh:
                datas.append(fh.read())
    if not optimize:
        if not device:
            return jpeg_recode.recode_host(datas, restart, stats)
        return jpeg_recode.recode_device(datas, restart, chunk=chunk, stats=stats)
    if not device:
        return jpeg_recode.recode_host(datas, restart, stats, optimize=True)
    return jpeg_recode.recode_device(datas, restart, chunk=chunk, stats=stats, optimize=True)


def recode_mjpeg(src, dst: str, restart_blocks: int = 8, device: bool = True, stats: Optional[dict] = None, piece: int = 1024,
                 optimize: bool = False) -> int:
    """``src`` (a Motion-JPEG .avi, a .mjpeg / .mjpg stream or a folder of JPEG frames) re-coded losslessly (``recode_frames``) into
    ``dst`` (.avi, .mjpeg or .mjpg; an AVI of 1 GiB or more is refused, as ``save_mjpeg`` refuses it).  EVERY raw frame is carried
    over, at the source's frame rate.  ``optimize``: ``recode_frames``' (per-frame tables; the output does not depend on ``piece``).
    Returns the frames written."""
    from . import jpeg, jpeg_recode
    optimize = bool(optimize)
    jpeg_recode.recode_restart(restart_blocks, optimize)
    s = jpeg.open_source(src)
    if s is None:
        raise ValueError(f"recode_mjpeg: {src!r}: expected a Motion-JPEG .avi, a .mjpeg / .mjpg stream or a folder of JPEG frames")
    more = dict(optimize=True) if optimize else {}
    try:
        if s.n_frames < 1:
            raise ValueError(f"recode_mjpeg: {src!r} holds no frame")
        rc, info, msg = jpeg.probe(s.read(0))              # a container wants the picture size: the first frame's own header says it
        if rc == jpeg.MALFORMED:
            raise ValueError(f"recode_mjpeg: {s.label(0)}: {msg}")
        W, H = int(info[0]), int(info[1])
        files: List[bytes] = []
        for k0 in range(0, s.n_frames, piece):
            files += recode_frames([s.read(i) for i in range(k0, min(s.n_frames, k0 + piece))], restart_blocks, device, stats, **more)
        fps = s.fps
    finally:
        s.close()
    write_mjpeg_file(dst, files, W, H, fps)
    return len(files)
