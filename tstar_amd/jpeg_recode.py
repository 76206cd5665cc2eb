"""Lossless re-coding of baseline JPEG frames with a restart interval: the JPEG counterpart of ``jpegtran -restart``.

A frame without restart markers is one long segment to the device entropy decoder, which cuts it into sub-sequences and pays the
latency of the self-synchronising rounds on every fetch of a compressed-resident store.  A frame with a restart interval is one lane
per interval and nothing is cut.  Cameras, ffmpeg and Pillow write no markers, so this module puts them in without touching a pixel:
the entropy decoder's quantised coefficients go straight back through the encoder's scan stage (standard Huffman tables, DRI /
RSTn every ``restart`` MCUs) under a header that carries the SOURCE's quantisation tables (``jpeg_encode.header_from_tables``).

``recode_host`` is the host twin (``jpeg.entropy_batch`` + ``jpeg_encode.scan_host``; no GPU).  ``DeviceRecoder`` is the device
path for one chunk of an ``jpeg.EntropyRunner``: tstar_jpeg_encode_scan_rst on the coefficients the runner left in HBM, one read of
the lengths and statuses, then tstar_jpeg_recode_assemble builds the piece of the new arena and its records on the device
(csrc/jpeg_recode.hip) -- no compressed byte goes to the host.  ``jpeg_resident.load_resident(recode_blocks=)`` drives it at open;
``jpeg_encode.recode_frames`` / ``recode_mjpeg`` drive it file to file.

A frame is KEPT (its source bytes, not re-coded) and counted when the decoder routes it to the host or to Pillow (grayscale,
progressive, arithmetic, CMYK, uncovered sampling, a device status that is not OK) or when the encoder's walk meets a coefficient or
DC difference beyond the standard tables' categories.  A scan that does not fit its slot is coded again into the plan's worst-case
slot: never dropped, never truncated.  The output always carries the standard Huffman tables, so a source with optimised tables grows.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import jpeg
from . import jpeg_encode as JE

RECODE_DESC_DTYPE = np.dtype([("kind", "<u4"), ("hdr", "<u4"), ("src", "<u4"), ("src_off", "<u4"), ("src_len", "<u4"), ("table_set", "<i4"),
                              ("first_segment", "<u4"), ("n_segments", "<u4")])
NEW, KEPT = 0, 1
HEADER_PITCH = 1024
STATS = ("recoded", "kept", "bytes_in", "bytes_out")
PIECE_LIMIT = (1 << 32) - 16       # a piece addresses its bytes with 32 bits, like every batch of the entropy launchers
RETRY_BYTES = 256 << 20            # slots of the worst case a retry holds at a time
_SUBSAMPLING = {(2, 2): "4:2:0", (2, 1): "4:2:2", (1, 1): "4:4:4"}
_HUFF_BYTES = 6 * 1424             # the six flat Huffman tables lead a table set (csrc/jpeg_entropy_core.h)


def recode_interval(recode_blocks) -> int:
    """``recode_blocks`` / ``restart_blocks`` of a re-code: MCUs per interval, 1..65535 (what DRI holds); ValueError otherwise."""
    _, blocks = JE._restart_values(None, recode_blocks)
    if blocks < 1:
        raise ValueError(f"JPEG re-code interval {recode_blocks!r}: expected 1..{JE.RESTART_LIMIT} MCUs")
    return blocks


def recode_mode(recode_blocks=None) -> int:
    """The keyword when given, else TSTAR_JPEG_RECODE, else 0 (no re-coding)."""
    if recode_blocks is None:
        v = os.environ.get("TSTAR_JPEG_RECODE", "")
        if v in ("", "0"):
            return 0
        try:
            recode_blocks = int(v)
        except ValueError:
            raise ValueError(f"TSTAR_JPEG_RECODE={v!r}: expected 1..{JE.RESTART_LIMIT} MCUs") from None
    return recode_interval(recode_blocks)


def new_stats() -> dict:
    return {k: 0 for k in STATS}


def _count(stats: Optional[dict], kept: bool, n_in: int, n_out: int) -> None:
    if stats is not None:
        stats["kept" if kept else "recoded"] = stats.get("kept" if kept else "recoded", 0) + 1
        stats["bytes_in"] = stats.get("bytes_in", 0) + int(n_in)
        stats["bytes_out"] = stats.get("bytes_out", 0) + int(n_out)


def recodable(geom) -> bool:
    """Whether frames of geometry (W, H, ncomp, hs, vs) are re-coded: three components at a sampling the encoder's scan stage covers.
    Frames of any other geometry (grayscale among them) are kept."""
    return geom is not None and int(geom[2]) == 3 and (int(geom[3]), int(geom[4])) in _SUBSAMPLING


def covered(data: bytes):
    """The geometry (W, H, 3, hs, vs) when the re-coder takes the file: three components the decoder's kernels and the encoder's scan
    stage cover; None for a file that is kept."""
    rc, info, _ = jpeg.probe(data)
    if rc != jpeg.OK or not recodable(info):
        return None
    return tuple(int(v) for v in info)


# ------------------------------------------------------------------------------------------------ host twin
def recode_host(datas: Sequence[bytes], restart: int, stats: Optional[dict] = None) -> List[bytes]:
    """Every file of ``datas`` re-coded with an interval of ``restart`` MCUs, or kept; files may differ in geometry."""
    restart = recode_interval(restart)
    out = []
    for data in datas:
        data = bytes(data)
        new = _recode_one_host(data, restart)
        _count(stats, new is None, len(data), len(data if new is None else new))
        out.append(data if new is None else new)
    return out


def _recode_one_host(data: bytes, restart: int) -> Optional[bytes]:
    geom = covered(data)
    if geom is None:
        return None
    blocks, _ = jpeg._sizes(geom)
    coef = np.empty((1, blocks * 64), dtype=np.int16)
    quant = np.empty((1, 192), dtype=np.uint16)
    status, _ = jpeg.entropy_batch([data], geom, coef, quant, 1)
    if status[0] != jpeg.OK:
        return None
    return code_host(coef, quant, geom, restart)


def code_host(coef: np.ndarray, quant: np.ndarray, geom, restart: int) -> Optional[bytes]:
    """The second half of the host twin: one frame's quantised coefficients (int16 [1, blocks * 64], the decoder's layout) and its
    quant rows (uint16 [192]) -> the file with the interval, or None when the encoder's walk meets a coefficient or DC difference of
    a size category the standard tables have no code for (the frame is then kept)."""
    W, H, _, hs, vs = geom
    sub = _SUBSAMPLING[(hs, vs)]
    scans, _, st = JE.scan_host(coef, W, H, sub, threads=1, restart_blocks=restart)
    if st[0] == JE.STATUS_BAD_COEF:
        return None
    if st[0] != JE.STATUS_OK:
        raise RuntimeError("JPEG re-code (host): a scan did not fit the bound of its geometry")
    return JE.header_from_tables(W, H, np.asarray(quant).reshape(3, 64), sub, restart) + scans[0]


# ------------------------------------------------------------------------------------------------ table sets
_std_huffman_bytes = None


def _std_huffman() -> np.ndarray:
    """The six flat Huffman tables of a table set whose file carries the standard tables (what the planner makes of them)."""
    global _std_huffman_bytes
    if _std_huffman_bytes is None:
        f = JE.encode_frames(np.zeros((1, 8, 8, 3), dtype=np.uint8), 75, "4:4:4", device=False)[0]
        plan = jpeg.plan_segments([f], (8, 8, 3, 1, 1))
        assert plan.route[0] == jpeg.ROUTE_DEVICE and plan.table_sets.shape == (1, jpeg.TABLE_SET_BYTES)
        _std_huffman_bytes = plan.table_sets[0, :_HUFF_BYTES].copy()
    return _std_huffman_bytes


def recoded_table_set(src_set: np.ndarray) -> np.ndarray:
    """The table set of a re-coded frame: the standard Huffman tables; quantisation rows, zigzag order and energy limits (computed in
    double by the planner) are the source frame's."""
    ts = np.array(src_set, dtype=np.uint8).reshape(jpeg.TABLE_SET_BYTES)
    ts[:_HUFF_BYTES] = _std_huffman()
    return ts


def recode_layout(m: int, n_segments: int):
    """(bytes of the record buffer, offsets of off / len / quant / frame records / segments) (tstar_jpeg_recode_layout)."""
    from . import _lib
    out5 = (C.c_size_t * 5)()
    n = int(_lib.load().tstar_jpeg_recode_layout(m, n_segments, out5))
    if n == 0:
        raise ValueError(f"recode_layout: not a piece (m={m}, n_segments={n_segments})")
    return n, tuple(int(v) for v in out5)


def parse_records(rec: np.ndarray, m: int, n_segments: int):
    """A record buffer (uint8) -> (off uint64 [m + 1], len uint32 [m], quant uint16 [m,192], frames FRAME_DTYPE [m], segments)."""
    _, (o_at, l_at, q_at, f_at, s_at) = recode_layout(m, n_segments)
    return (rec[o_at:o_at + 8 * (m + 1)].view(np.uint64), rec[l_at:l_at + 4 * m].view(np.uint32),
            rec[q_at:q_at + 384 * m].view(np.uint16).reshape(m, 192), rec[f_at:f_at + 16 * m].view(jpeg.FRAME_DTYPE),
            rec[s_at:s_at + 24 * n_segments].view(jpeg.SEGMENT_DTYPE))


class PieceDesc:
    """What the host knows about a piece [a, b) of a source batch once the scan stage's lengths and statuses are read: the descriptor
    (RECODE_DESC_DTYPE [m]), the header table, the output's table sets (in the planner's order: first appearance) and every frame's
    output length."""

    def __init__(self, plan: jpeg.SegmentPlan, src_lens, a: int, b: int, kept: np.ndarray, scan_len: np.ndarray, geom, restart: int):
        W, H, _, hs, vs = geom
        m = b - a
        self.m, self.restart = m, restart
        self.n_mcu = ((W + 8 * hs - 1) // (8 * hs)) * ((H + 8 * vs - 1) // (8 * vs))
        n_int = (self.n_mcu + restart - 1) // restart
        desc = np.zeros(m, dtype=RECODE_DESC_DTYPE)
        headers, sets, out_len = {}, {}, np.zeros(m, dtype=np.int64)
        self.header_bytes = []
        for j in range(m):
            s = a + j
            ts = int(plan.frames["table_set"][s])
            d = desc[j]
            d["src"] = s
            if kept[j]:
                d["kind"], d["src_off"], d["src_len"] = KEPT, int(plan.offsets[s]), int(src_lens[s])
                key = plan.table_sets[ts].tobytes() if ts >= 0 else None
                d["n_segments"] = int(plan.frames["n_segments"][s]) if ts >= 0 else 0
                out_len[j] = int(src_lens[s])
            else:
                qkey = plan.quant[s].tobytes()
                if qkey not in headers:
                    headers[qkey] = len(self.header_bytes)
                    self.header_bytes.append(JE.header_from_tables(W, H, plan.quant[s].reshape(3, 64), _SUBSAMPLING[(hs, vs)], restart))
                d["kind"], d["hdr"], d["n_segments"] = NEW, headers[qkey], n_int
                key = recoded_table_set(plan.table_sets[ts]).tobytes()
                out_len[j] = len(self.header_bytes[d["hdr"]]) + int(scan_len[j])
            d["table_set"] = -1 if key is None else sets.setdefault(key, len(sets))
        desc["first_segment"] = np.cumsum(desc["n_segments"], dtype=np.int64) - desc["n_segments"]
        self.desc, self.out_len, self.total = desc, out_len, int(out_len.sum())
        self.n_segments = int(desc["n_segments"].sum())
        self.table_sets = (np.stack([np.frombuffer(k, dtype=np.uint8) for k in sets]) if sets
                           else np.zeros((0, jpeg.TABLE_SET_BYTES), dtype=np.uint8))
        nh = max(1, len(self.header_bytes))
        self.headers = np.zeros((nh, HEADER_PITCH), dtype=np.uint8)
        self.header_len = np.zeros(nh, dtype=np.uint32)
        for k, h in enumerate(self.header_bytes):
            self.headers[k, :len(h)] = np.frombuffer(h, dtype=np.uint8)
            self.header_len[k] = len(h)

    def plan_of(self, rec: np.ndarray) -> jpeg.SegmentPlan:
        """The SegmentPlan of the output from a record buffer (device-built or the mirror's), checked against what the host knows:
        the lengths, the table sets, and that every interval of a re-coded frame got its byte range."""
        off, ln, quant, frames, segments = parse_records(rec, self.m, self.n_segments)
        new = self.desc["kind"] == NEW
        good = (int(off[self.m]) == self.total and np.array_equal(ln.astype(np.int64), self.out_len)
                and np.array_equal(frames["table_set"], self.desc["table_set"]))
        seg_new = new[np.minimum(segments["frame"], self.m - 1)] & (segments["frame"] < self.m)
        good = good and bool((segments["frame"] < self.m).all()) and bool((segments["begin"][seg_new] < segments["end"][seg_new]).all())
        if not good:
            raise RuntimeError("JPEG re-code: the assembled piece disagrees with the scan stage's lengths or its markers")
        route = np.where(frames["table_set"] >= 0, jpeg.ROUTE_DEVICE, jpeg.ROUTE_HOST).astype(np.int32)
        return jpeg.SegmentPlan(route, frames.copy(), quant.copy(), self.table_sets, segments.copy(), off[:self.m].copy(), self.total)


def assemble_host(pd: PieceDesc, slots: np.ndarray, scan_len: np.ndarray, src_bytes: np.ndarray, plan: jpeg.SegmentPlan):
    """The host mirror of the assembly (tstar_jpeg_recode_assemble_host) -> (output bytes uint8 [total], record buffer uint8)."""
    from . import _lib
    nrec, _ = recode_layout(pd.m, pd.n_segments)
    rec = _aligned16(np.zeros(nrec, dtype=np.uint8))
    out = np.zeros(max(16, pd.total), dtype=np.uint8)
    slots = np.ascontiguousarray(slots, dtype=np.uint8)
    scan_len = np.ascontiguousarray(scan_len, dtype=np.uint32)
    segs = plan.segments if len(plan.segments) else np.zeros(1, dtype=jpeg.SEGMENT_DTYPE)
    quant = _aligned16(plan.quant)
    _lib.check(_lib.load().tstar_jpeg_recode_assemble_host(
        pd.desc.ctypes.data, pd.m, pd.n_segments, _aligned16(pd.headers).ctypes.data, pd.header_len.ctypes.data, len(pd.header_len),
        _aligned16(slots).ctypes.data, slots.shape[1], scan_len.ctypes.data, pd.restart, pd.n_mcu, src_bytes.ctypes.data, plan.total_bytes,
        quant.ctypes.data, plan.frames.ctypes.data, segs.ctypes.data, len(plan.frames), len(plan.segments), rec.ctypes.data, rec.size,
        out.ctypes.data, pd.total), "tstar_jpeg_recode_assemble_host")
    return out[:pd.total], rec


def _aligned16(a: np.ndarray) -> np.ndarray:
    """A C-contiguous copy of ``a`` at a 16-byte-aligned address."""
    a = np.ascontiguousarray(a)
    if a.ctypes.data % 16 == 0:
        return a
    raw = np.empty(a.nbytes + 16, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16
    b = raw[at:at + a.nbytes].view(a.dtype).reshape(a.shape)
    b[...] = a
    return b


# ------------------------------------------------------------------------------------------------ device path
class Piece:
    """A piece of the new arena: d_bytes (uint8 cuda tensor, the frames end to end), its SegmentPlan, the frames' lengths, which of
    them were kept, and the first source frame it covers."""

    def __init__(self, d_bytes, plan, lens, kept, first):
        self.d_bytes, self.plan, self.lens, self.kept, self.first = d_bytes, plan, lens, kept, first


class DeviceRecoder:
    """Re-codes the chunks of one ``jpeg.EntropyRunner`` (frames of one geometry) on the current stream.  Owns the scan stage's
    buffers, reused chunk after chunk.  ``alloc(nbytes)`` hands out the output and record buffers (uint8 cuda tensors at 16-byte-
    aligned addresses); the default is torch.empty."""

    def __init__(self, geom, device, restart: int, stats: Optional[dict] = None, alloc=None, slot_bytes: Optional[int] = None):
        self.geom, self.device, self.restart = tuple(int(v) for v in geom), device, recode_interval(restart)
        if not recodable(self.geom):
            raise ValueError(f"JPEG re-code: geometry {self.geom} is not re-coded (three components at 4:2:0, 4:2:2 or 4:4:4 are); its frames are kept")
        self.stats = stats
        W, H, _, hs, vs = self.geom
        one = JE.Plan(W, H, hs, vs, 1, restart=self.restart)
        self.blocks = one.blocks
        self.max_slot = (one.max_scan_bytes + 15) // 16 * 16
        self.first_slot = None if slot_bytes is None else min(self.max_slot, max(16, (int(slot_bytes) + 15) // 16 * 16))
        self.alloc = alloc if alloc is not None else self._alloc
        self.bufs = None
        self.retried = 0

    def _alloc(self, nbytes: int):
        import torch
        return torch.empty(max(16, nbytes), dtype=torch.uint8, device=self.device)

    def _buffers(self, m: int, slot: int):
        import torch
        if self.bufs is None or self.bufs[0] < m or self.bufs[1] != slot:
            self.bufs = None
            W, H, _, hs, vs = self.geom
            p = JE.Plan(W, H, hs, vs, m, slot, self.restart)
            self.bufs = (m, slot, torch.empty(p.workspace_bytes, dtype=torch.uint8, device=self.device),
                         torch.empty((m, slot), dtype=torch.uint8, device=self.device),
                         torch.empty((2, m), dtype=torch.int32, device=self.device))
        return self.bufs[2:]

    def recode_chunk(self, batch: jpeg.DeviceBatch, d_buf, d_coef, bad) -> List[Piece]:
        """The chunk ``batch`` (uploaded into ``d_buf``, its coefficients in ``d_coef``; ``bad``: the frames the device did not
        return OK for) -> the pieces of the new arena, in order."""
        n = len(batch.datas)
        src_lens = np.fromiter((len(d) for d in batch.datas), dtype=np.int64, count=n)
        bad_mask = np.zeros(n, dtype=bool)
        bad_mask[list(bad)] = True
        # the first pass: twice the longest source file (the standard tables cost a source with optimised ones a few per cent, a
        # marker with its padding at most 3 bytes per interval); frames it is short of are coded again at the bound
        slot = self.first_slot or min(self.max_slot, (2 * int(src_lens.max()) + 4096 + 15) // 16 * 16)
        return self._pieces(batch, d_buf, d_coef, bad_mask, src_lens, 0, n, slot)

    def _pieces(self, batch, d_buf, d_coef, bad_mask, src_lens, a: int, b: int, slot: int) -> List[Piece]:
        import torch
        from . import _lib
        lib = _lib.load()
        W, H, _, hs, vs = self.geom
        m = b - a
        work, out, meta = self._buffers(m, slot)
        s = _lib.stream_ptr()
        _lib.check(lib.tstar_jpeg_encode_scan_rst(d_coef.data_ptr() + a * self.blocks * 128, m, W, H, hs, vs, self.restart, out.data_ptr(), slot,
                                                  meta[0].data_ptr(), meta[1].data_ptr(), work.data_ptr(), work.numel(), None, s),
                   "tstar_jpeg_encode_scan_rst")
        meta_h = meta[:, :m].cpu().numpy()               # ONE read: lengths (u32 bits) and statuses
        scan_len, status = meta_h[0].view(np.uint32).astype(np.int64), meta_h[1]
        kept = bad_mask[a:b] | (status == JE.STATUS_BAD_COEF)
        short = (status == JE.STATUS_SHORT) & ~kept
        if short.any():
            if slot >= self.max_slot:
                raise RuntimeError("JPEG re-code: a scan did not fit the bound of its geometry")
            self.retried += int(short.sum())
            step = max(1, min(m, RETRY_BYTES // self.max_slot))
            return [p for s0 in range(a, b, step)
                    for p in self._pieces(batch, d_buf, d_coef, bad_mask, src_lens, s0, min(b, s0 + step), self.max_slot)]
        pd = PieceDesc(batch.plan, src_lens, a, b, kept, scan_len, self.geom, self.restart)
        if pd.total >= PIECE_LIMIT:
            if m == 1:
                raise RuntimeError("JPEG re-code: one frame of 4 GiB")
            mid = a + m // 2
            return (self._pieces(batch, d_buf, d_coef, bad_mask, src_lens, a, mid, slot)
                    + self._pieces(batch, d_buf, d_coef, bad_mask, src_lens, mid, b, slot))
        nrec, _ = recode_layout(m, pd.n_segments)
        d_out, d_rec = self.alloc(pd.total), self.alloc(nrec)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(self.device)      # noqa: E731
        d_desc, d_headers, d_hlen = up(pd.desc), up(pd.headers), up(pd.header_len)
        base, parts, plan = d_buf.data_ptr(), batch.parts, batch.plan
        _lib.check(lib.tstar_jpeg_recode_assemble(
            pd.desc.ctypes.data, d_desc.data_ptr(), m, pd.n_segments, d_headers.data_ptr(), d_hlen.data_ptr(), len(pd.header_len),
            out.data_ptr(), slot, meta[0].data_ptr(), self.restart, pd.n_mcu, base, batch.total, base + parts["quant"][0],
            base + parts["frames"][0], base + parts["segments"][0], len(plan.frames), len(plan.segments), d_rec.data_ptr(), nrec,
            d_out.data_ptr(), pd.total, int(pd.out_len.max()), s), "tstar_jpeg_recode_assemble")
        rec = d_rec[:nrec].cpu().numpy()                 # the records only: the bytes stay on the device
        for j in range(m):
            _count(self.stats, bool(kept[j]), src_lens[a + j], pd.out_len[j])
        return [Piece(d_out[:pd.total], pd.plan_of(rec), pd.out_len.astype(np.uint32), kept, a)]


def runner_for(datas: Sequence[bytes], geom, device, chunk: Optional[int] = None):
    """An ``jpeg.EntropyRunner`` over ``datas`` (files of geometry ``geom``) outside an open."""
    ctx = jpeg.JpegOpen.for_geometry(jpeg.JpegList(list(datas)), list(range(len(datas))), device, geom)
    return jpeg.EntropyRunner(ctx, chunk, jpeg.split_min_bytes())


def recode_device(datas: Sequence[bytes], restart: int, device="cuda", chunk: Optional[int] = None, stats: Optional[dict] = None,
                  alloc=None, slot_bytes: Optional[int] = None, pieces_out: Optional[list] = None) -> List[bytes]:
    """``recode_host`` through the device path: files of one geometry are entropy-decoded, re-coded and assembled together, chunk by
    chunk, and only the finished pieces are read back.  ``pieces_out``: a list that receives (source files, Piece) of every piece."""
    import torch
    restart = recode_interval(restart)
    datas = [bytes(d) for d in datas]
    out: List[Optional[bytes]] = [None] * len(datas)
    groups = {}
    for i, d in enumerate(datas):
        geom = covered(d)
        if geom is None:
            out[i] = d
            _count(stats, True, len(d), len(d))
        else:
            groups.setdefault(geom, []).append(i)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream()
        for geom, ids in groups.items():
            files = [datas[i] for i in ids]
            run = runner_for(files, geom, device, chunk)
            rec = DeviceRecoder(geom, device, restart, stats, alloc, slot_bytes)
            k0 = 0
            while k0 < len(files):
                part = run.read(k0)
                ticket = run.submit(k0, part, stream)
                bad = run.collect(ticket)
                for p in rec.recode_chunk(ticket[1], run.d_buf, run.d_coef, bad):
                    host = p.d_bytes.cpu().numpy()
                    for j, (o, n) in enumerate(zip(p.plan.offsets, p.lens)):
                        out[ids[k0 + p.first + j]] = host[int(o):int(o) + int(n)].tobytes()
                    if pieces_out is not None:
                        pieces_out.append((part[p.first:p.first + len(p.lens)], p))
                k0 += len(part)
    return out
