"""Compressed-resident Motion-JPEG store: the file's wanted frames stay in HBM as they are on disk and are decoded on demand.

``load_resident`` opens a JPEG source with the pieces ``jpeg.load_jpeg(entropy="device")`` opens it with (``jpeg.JpegOpen``,
``jpeg.EntropyRunner``) -- every wanted frame is planned, uploaded, entropy-decoded on the device and status-checked once, so a broken
file fails at open with the same messages -- but keeps the compressed bytes (the ARENA) and the planner's records instead of the
pixels.  A ``video.JpegFrameStore`` then serves ``lease(secs)``:
frames that are not in its small pool of RGB slots are gathered from the arena into one batch buffer (tstar_jpeg_gather), entropy-
decoded (tstar_jpeg_entropy_split_device) and reconstructed into their slots (tstar_jpeg_reconstruct_slots) on the current stream,
just before the ingest kernel reads them.  Frames the device decoder does not vouch for (progressive, arithmetic, CMYK, another
sampling, or a device status that is not OK) are decoded once at open by the host decoder / Pillow and kept as RGB in permanent
slots behind the pool.  ``SlotPool`` is the pool's bookkeeping as pure Python (no torch, no GPU).
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict
from typing import Optional

import numpy as np

from . import jpeg

DESC_DTYPE = np.dtype([("id", "<u4"), ("dst", "<u4"), ("len", "<u4"), ("first_segment", "<u4"), ("n_segments", "<u4"), ("reserved", "<u4")])
POOL_FRAMES = 512              # default pool_frames
FETCH_COEF_BUDGET = 128 << 20  # bytes of coefficient scratch a fetch works in: larger fetches run in pieces
RESIDENT_MODES = ("jpeg",)


def resident_mode(resident: Optional[str] = None) -> Optional[str]:
    """The keyword when given, else "jpeg" under TSTAR_JPEG_RESIDENT=1, else None (the decoded store)."""
    if resident is None:
        resident = "jpeg" if os.environ.get("TSTAR_JPEG_RESIDENT", "") not in ("", "0") else None
    if resident is not None and resident not in RESIDENT_MODES:
        raise ValueError(f"resident={resident!r}: expected one of {RESIDENT_MODES} or None")
    return resident


def pool_size(pool_frames: Optional[int] = None) -> int:
    """The keyword when given, else TSTAR_JPEG_POOL, else POOL_FRAMES."""
    v = pool_frames if pool_frames is not None else (os.environ.get("TSTAR_JPEG_POOL") or POOL_FRAMES)
    try:
        n = int(v)
    except (TypeError, ValueError):
        n = 0
    if n < 1:
        raise ValueError(f"pool_frames={v!r}: expected a frame count >= 1")
    return n


def gather_layout(total_bytes: int, m: int, n_segments: int):
    """(buffer bytes, offsets of the quant rows, the frame records, the segments) of a batch (tstar_jpeg_gather_bytes)."""
    from . import _lib
    out3 = (C.c_size_t * 3)()
    n = int(_lib.load().tstar_jpeg_gather_bytes(total_bytes, m, n_segments, out3))
    if n == 0:
        raise ValueError(f"gather_layout: not a batch (total_bytes={total_bytes}, m={m}, n_segments={n_segments}); a fetch holds below 2^32 bytes")
    return n, int(out3[0]), int(out3[1]), int(out3[2])


def gather_descriptor(ids, lens: np.ndarray, nsegs: np.ndarray):
    """The descriptor of a fetch of arena frames ``ids`` from the per-frame counts kept at open -> (DESC_DTYPE [m], total bytes,
    segments)."""
    ids = np.asarray(ids, dtype=np.int64)
    if ids.size and (ids.min() < 0 or ids.max() >= len(lens)):
        raise ValueError(f"gather_descriptor: a frame id outside the arena's 0..{len(lens) - 1}")
    ln, ns = lens[ids].astype(np.int64), nsegs[ids].astype(np.int64)
    padded = (ln + 15) & ~15
    total, nseg = int(padded.sum()), int(ns.sum())
    if total >= 1 << 32:
        raise ValueError(f"gather_descriptor: {total} bytes in one fetch; the segments address a batch with 32 bits")
    desc = np.zeros(len(ids), dtype=DESC_DTYPE)
    desc["id"], desc["len"], desc["n_segments"] = ids, ln, ns
    desc["dst"] = np.cumsum(padded) - padded
    desc["first_segment"] = np.cumsum(ns) - ns
    return desc, total, nseg


class Arena:
    """A file's wanted frames and what the planner said about each, as numpy arrays:
    bytes uint8, off uint64 [E], len uint32 [E], quant uint16 [E,192], frames FRAME_DTYPE [E] (first_segment into ``segments``),
    segments SEGMENT_DTYPE [S] (begin / end from the frame's first byte), table_sets uint8 [n_sets, TABLE_SET_BYTES]."""

    def __init__(self, off, lens, quant, frames, segments, table_sets, bytes_=None):
        self.bytes, self.off, self.len, self.quant = bytes_, off, lens, quant
        self.frames, self.segments, self.table_sets = frames, segments, table_sets

    @property
    def n_entries(self) -> int:
        return len(self.len)

    def gather_host(self, ids, buf: Optional[np.ndarray] = None, arena_bytes: Optional[int] = None):
        """The host mirror of the gather kernel (tstar_jpeg_gather_host) -> (batch uint8, SegmentPlan over it)."""
        from . import _lib
        desc, total, nseg = gather_descriptor(ids, self.len, self.frames["n_segments"])
        nbytes, q_at, f_at, s_at = gather_layout(total, len(desc), nseg)
        if buf is None:
            buf = np.empty(nbytes, dtype=np.uint8)
        _lib.check(_lib.load().tstar_jpeg_gather_host(
            self.bytes.ctypes.data, self.bytes.size if arena_bytes is None else arena_bytes, self.off.ctypes.data, self.len.ctypes.data,
            self.quant.ctypes.data, self.frames.ctypes.data, self.segments.ctypes.data, self.n_entries, len(self.segments), desc.ctypes.data,
            len(desc), total, nseg, buf.ctypes.data, buf.size), "tstar_jpeg_gather_host")
        m = len(desc)
        plan = jpeg.SegmentPlan(np.zeros(m, dtype=np.int32), buf[f_at:f_at + 16 * m].view(jpeg.FRAME_DTYPE),
                                buf[q_at:q_at + 384 * m].view(np.uint16).reshape(m, 192), self.table_sets,
                                buf[s_at:s_at + 24 * nseg].view(jpeg.SEGMENT_DTYPE), desc["dst"].astype(np.uint64), total)
        return buf, plan


class ArenaBuilder:
    """Collects the plans of an open's chunks into one Arena: segments rebased to their frame, table sets deduplicated over the file."""

    def __init__(self):
        self.off, self.len, self.quant, self.frames, self.segments = [], [], [], [], []
        self.sets, self.set_ids = [], {}
        self.total, self.n_segments = 0, 0

    def add(self, plan: jpeg.SegmentPlan, lens, base: Optional[int] = None) -> None:
        """One chunk: its frames sit at ``base`` + plan.offsets of the arena (default: behind what is there)."""
        base = self.total if base is None else int(base)
        remap = np.empty(max(1, len(plan.table_sets)), dtype=np.int32)
        for k, ts in enumerate(plan.table_sets):
            key = ts.tobytes()
            if key not in self.set_ids:
                self.set_ids[key] = len(self.sets)
                self.sets.append(np.array(ts, dtype=np.uint8))
            remap[k] = self.set_ids[key]
        fr = plan.frames.copy()
        routed = fr["table_set"] >= 0
        fr["table_set"][routed] = remap[fr["table_set"][routed]]
        fr["first_segment"][routed] += self.n_segments
        seg = plan.segments.copy()
        rel = plan.offsets[seg["frame"]].astype(np.int64)
        seg["begin"] = seg["begin"].astype(np.int64) - rel
        seg["end"] = seg["end"].astype(np.int64) - rel
        seg["frame"] += sum(len(x) for x in self.len)                  # the arena frame (the gather writes the batch's own)
        self.off.append(plan.offsets.astype(np.uint64) + np.uint64(base))
        self.len.append(np.asarray(lens, dtype=np.uint32))
        self.quant.append(plan.quant.copy())
        self.frames.append(fr)
        self.segments.append(seg)
        self.n_segments += len(seg)
        self.total = max(self.total, base + plan.total_bytes)

    def finish(self, bytes_=None) -> Arena:
        cat = np.concatenate
        sets = np.stack(self.sets) if self.sets else np.zeros((1, jpeg.TABLE_SET_BYTES), dtype=np.uint8)
        return Arena(cat(self.off), cat(self.len), np.ascontiguousarray(cat(self.quant)), cat(self.frames), cat(self.segments), sets, bytes_)


class SlotPool:
    """Bookkeeping of ``pool_frames`` RGB slots (pure Python).  An ENTRY (an arena frame) sits in at most one slot; a slot that a
    live lease holds is never handed out; of the others the least recently released goes first.  ``exceptions``: entries with a
    permanent slot pool_frames + k, never evicted.  Streams and events are opaque here: ``key`` names the stream a call is made
    on, tokens stand for events recorded on it, and acquire() returns the tokens the caller's stream has to wait for."""

    def __init__(self, pool_frames: int, exceptions=()):
        self.pool_frames = int(pool_frames)
        self.permanent = {int(e): self.pool_frames + k for k, e in enumerate(exceptions)}
        self.slot_of = {}
        self.entry_of = [None] * self.pool_frames
        self.refs = [0] * self.pool_frames
        self.idle = OrderedDict((s, None) for s in range(self.pool_frames))      # no live lease; least recently released first
        self.readers = [dict() for _ in range(self.pool_frames)]                 # stream key -> token of its last done()
        self.ready = [None] * self.pool_frames                                   # (stream key, token) of the fetch that filled it
        self.hits = self.misses = self.evictions = 0

    def acquire(self, entries, key=None):
        """-> (slot of every entry in the order asked, [(entry, slot)] to fill, tokens to wait for).  Raises ValueError, before
        anything changes, when the distinct entries that are not resident outnumber the slots no lease holds."""
        entries = [int(e) for e in entries]
        normal = [e for e in dict.fromkeys(entries) if e not in self.permanent]
        hit = [e for e in normal if e in self.slot_of]
        miss = [e for e in normal if e not in self.slot_of]
        free = len(self.idle) - sum(1 for e in hit if self.refs[self.slot_of[e]] == 0)
        if len(miss) > free:
            raise ValueError(f"{len(miss)} frames to decode, {free} of the pool_frames={self.pool_frames} slots are free "
                             f"({self.pool_frames - len(self.idle)} held by leases that are not done): open the store with a larger pool_frames")
        waits = []
        for e in hit:
            s = self.slot_of[e]
            if self.refs[s] == 0:
                del self.idle[s]
            self.refs[s] += 1
            if self.ready[s] is not None and self.ready[s][0] != key:
                waits.append(self.ready[s][1])
        fill = []
        for e in miss:
            s, _ = self.idle.popitem(last=False)
            if self.entry_of[s] is not None:
                del self.slot_of[self.entry_of[s]]
                self.evictions += 1
            waits += [t for k, t in self.readers[s].items() if k != key]
            if self.ready[s] is not None and self.ready[s][0] != key:
                waits.append(self.ready[s][1])
            self.readers[s], self.ready[s] = {}, None
            self.entry_of[s], self.slot_of[e], self.refs[s] = e, s, 1
            fill.append((e, s))
        self.hits += len(hit)
        self.misses += len(miss)
        return [self.permanent[e] if e in self.permanent else self.slot_of[e] for e in entries], fill, waits

    def filled(self, slots, key, token) -> None:
        for s in slots:
            self.ready[s] = (key, token)

    def release(self, slots, key=None, token=None) -> None:
        """A lease is done: ``token`` stands for everything queued on stream ``key`` so far (its readers of the slots)."""
        for s in dict.fromkeys(slots):
            if s >= self.pool_frames:
                continue
            self.refs[s] -= 1
            if token is not None:
                self.readers[s][key] = token
            if self.refs[s] == 0:
                self.idle[s] = None

    def flush(self) -> int:
        """Drop every resident entry no live lease holds -> how many.  Their slots stay ordered behind their readers."""
        n = 0
        for s in self.idle:
            if self.entry_of[s] is not None:
                del self.slot_of[self.entry_of[s]]
                self.entry_of[s] = None
                n += 1
        return n

    def forget(self, fill) -> None:
        """A fetch failed before its kernels were queued: the slots it was to fill hold nothing."""
        for e, s in fill:
            del self.slot_of[e]
            self.entry_of[s] = None


def _entry_keys(src, want):
    """Arena entry of every wanted frame: frames that are the same byte range of a mapped file (an AVI dropped frame repeats the
    previous chunk) share one.  -> (entry per second, raw frame of every entry)."""
    ranges = getattr(src, "ranges", None)
    seen, sec_entry, raw = {}, [], []
    for fi in want:
        key = tuple(ranges[fi]) if ranges is not None else fi
        if key not in seen:
            seen[key] = len(raw)
            raw.append(fi)
        sec_entry.append(seen[key])
    return np.asarray(sec_entry, dtype=np.int64), raw


def load_resident(src: jpeg.JpegFrames, device: str = "cuda", pool_frames: Optional[int] = None, chunk: Optional[int] = None,
                  scale: int = 1, recode_blocks: Optional[int] = None, recode_optimize: bool = False, group_frames: Optional[int] = None):
    """Open ``src`` as a ``video.JpegFrameStore`` (see the module text).  The open is ``load_jpeg``'s device mode with another
    destination: the same ``jpeg.JpegOpen`` (prelude, host verdict, counters, messages) and the same ``jpeg.EntropyRunner`` (one upload
    per chunk carries the bytes and the records, the entropy kernels check every frame); here the bytes move on into the arena, and a
    frame the device did not return OK for becomes an exception: RGB in a permanent slot.  ``scale`` 2, 4, 8: pool slots and permanent
    slots hold the frames at 1/scale size; the arena and the gather are those of the full-size store.  ``recode_blocks`` (MCUs, 1..65535;
    default: none): every chunk is re-coded losslessly with that restart interval while its coefficients are in HBM
    (``jpeg_recode.DeviceRecoder``), and the arena holds the re-coded bytes only: a fetch then decodes one lane per interval and
    cuts nothing, whatever the file on disk looks like.  The store's ``recode_stats`` says how many frames were re-coded and kept.
    ``recode_optimize`` (with ``recode_blocks``): the re-coded frames carry optimised Huffman tables, ONE set per group of the OK frames of
    a chunk (``jpeg_recode``, shared mode; ``group_frames``: frames per group, default the most the count bound allows), so the arena
    is smaller than the standard-table one and holds one decoder table set per group and quantisation set; ``recode_stats`` gains
    ``optimized`` and ``table_sets``."""
    import torch
    from . import jpeg_recode
    from .video import JpegFrameStore
    restart = jpeg_recode.recode_interval(recode_blocks) if recode_blocks else 0
    optimize = bool(recode_optimize)
    if optimize and not restart:
        raise ValueError("load_resident: recode_optimize optimises the tables of a re-coded arena: it needs recode_blocks")
    if str(device).startswith("cpu"):
        raise ValueError("resident='jpeg' needs a GPU store (device='cpu' was asked for)")
    P = pool_size(pool_frames)
    want = jpeg.wanted_frames(src.n_frames, src.fps)
    if not want:
        raise ValueError(f"Cannot open video file: {src.name} (shorter than one second)")
    sec_entry, raw = _entry_keys(src, want)
    E = len(raw)
    # the counters are per logical second, as load_jpeg's: an entry counts once for every second that shares it
    ctx = jpeg.JpegOpen(src, raw, device, seconds=np.bincount(sec_entry, minlength=E), scale=scale)
    min_split = jpeg.split_min_bytes()
    sizes = [src.ranges[fi][1] for fi in raw] if getattr(src, "ranges", None) is not None and not restart else None
    rstats = (jpeg_recode.new_stats(True) if optimize else jpeg_recode.new_stats()) if restart else None
    rec, long_segments = None, False                    # long_segments: a fetch will cut intervals whose rounds no open has counted
    builder = ArenaBuilder()
    d_parts = []                                        # the arena's bytes, chunk by chunk, when the sizes are not known up front
    d_arena = torch.empty(sum(sizes), dtype=torch.uint8, device=device) if sizes is not None else None
    exceptions = {}                                     # entry -> RGB uint8 [H,W,3] (numpy), or a cuda tensor

    def place(d_bytes):
        """A chunk's bytes (a tensor, host or device) into the arena, behind what is there."""
        if d_arena is not None:
            d_arena[builder.total:builder.total + d_bytes.numel()].copy_(d_bytes)
        else:
            d_parts.append(d_bytes.to(device, copy=True))

    e0 = 0
    while e0 < E and ctx.geom is None:
        data = ctx.read(e0)
        arr = ctx.prelude(e0, data)
        if arr is None:
            break
        exceptions[e0] = arr
        jpeg_recode._count(rstats, True, len(data), len(data))
        place(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        builder.add(jpeg.SegmentPlan(np.ones(1, np.int32), np.array([(-1, 0, 0, 0)], dtype=jpeg.FRAME_DTYPE), np.zeros((1, 192), np.uint16),
                                     np.zeros((0, jpeg.TABLE_SET_BYTES), np.uint8), np.zeros(0, jpeg.SEGMENT_DTYPE),
                                     np.zeros(1, np.uint64), len(data)), [len(data)])
        e0 += 1
    run = jpeg.EntropyRunner(ctx, chunk, min_split) if e0 < E else None
    # a clip whose covered frames are grayscale (or of a sampling the scan stage does not code) is kept whole: its chunks take the
    # plain open's way and are counted
    recoding = bool(restart) and jpeg_recode.recodable(ctx.geom)
    if recoding:
        rec = (jpeg_recode.DeviceRecoder(ctx.geom, device, restart, rstats, optimize=True, shared=True, group_frames=group_frames) if optimize
               else jpeg_recode.DeviceRecoder(ctx.geom, device, restart, rstats))
    stream = torch.cuda.current_stream()
    while e0 < E:
        datas = run.read(e0)
        ticket = run.submit(e0, datas, stream)
        batch = ticket[1]
        if not recoding:
            place(run.d_buf[:batch.total])
            builder.add(batch.plan, [len(d) for d in datas])
            for d in datas:
                jpeg_recode._count(rstats, True, len(d), len(d))
        bad = run.collect(ticket, split_stats=not recoding)     # waits for the chunk: the statuses decide what the arena may serve
        if recoding:
            kept, n_cut = np.zeros(len(datas), dtype=bool), 0
            for p in rec.recode_chunk(batch, run.d_buf, run.d_coef, bad):
                d_parts.append(p.d_bytes)
                builder.add(p.plan, p.lens)
                kept[p.first:p.first + len(p.lens)] = p.kept
                seg = p.plan.segments
                if min_split:                            # intervals long enough for a fetch to cut: none at a sensible interval
                    n_cut += int(((seg["end"].astype(np.int64) - seg["begin"] >= min_split) & ~p.kept[seg["frame"]]).sum())
            # the split counters describe the arena the store serves: a kept frame's segments as this open decoded them, and the
            # intervals of re-coded frames a fetch will cut; the open's own rounds on a frame that was re-coded are not the store's
            jpeg.count_split(ctx.sstats, run.seg_info(ticket)[kept[batch.plan.segments["frame"]]])
            ctx.sstats["split"] += n_cut
            long_segments |= n_cut > 0
        for j in bad:
            verdict = ctx.host_verdict(e0 + j, datas[j])
            if isinstance(verdict, tuple):
                rgb = torch.empty((1, ctx.oh, ctx.ow, 3), dtype=torch.uint8, device=device)
                ctx.reconstruct_one(*verdict, rgb)
                stream.synchronize()
                verdict = rgb[0]
            exceptions[e0 + j] = verdict
        e0 += len(datas)
    stream.synchronize()
    run = None                                          # its buffers go back before the store allocates the pool
    if d_arena is None:
        d_arena = torch.cat(d_parts) if len(d_parts) > 1 else d_parts[0]
        del d_parts
    arena = builder.finish()
    assert arena.n_entries == E and builder.total == d_arena.numel()
    st = JpegFrameStore(arena, d_arena, sec_entry, ctx.geom, (ctx.oh, ctx.ow), exceptions, P, src.fps, src.n_frames, name=src.name,
                        min_split_bytes=min_split, max_rounds=None if long_segments else ctx.sstats["rounds_max"], jpeg_scale=ctx.scale)
    st.recode_stats = rstats
    return ctx.attach(st)
