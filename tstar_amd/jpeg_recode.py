"""Lossless re-coding of baseline JPEG frames with a restart interval: the JPEG counterpart of ``jpegtran -restart``.

A frame without restart markers is one long segment to the device entropy decoder, which cuts it into sub-sequences and pays the
latency of the self-synchronising rounds on every fetch of a compressed-resident store.  A frame with a restart interval is one lane
per interval and nothing is cut.  Cameras, ffmpeg and Pillow write no markers, so this module puts them in without touching a pixel:
the entropy decoder's quantised coefficients go straight back through the encoder's scan stage (standard Huffman tables, DRI /
RSTn every ``restart`` MCUs) under a header that carries the SOURCE's quantisation tables (``jpeg_encode.header_from_tables``).

``recode_host`` is the host twin (``jpeg.entropy_batch`` + ``jpeg_encode.scan_host``; no GPU).  ``DeviceRecoder`` is the device
path for one chunk of an ``jpeg.EntropyRunner``: tstar_jpeg_encode_scan_rst on the coefficients the runner left in HBM, one read of
the lengths and statuses, then tstar_jpeg_recode_assemble_opt builds the piece of the new arena and its records on the device
(csrc/jpeg_recode.hip) -- no compressed byte goes to the host.  ``jpeg_resident.load_resident(recode_blocks=)`` drives it at open;
``jpeg_encode.recode_frames`` / ``recode_mjpeg`` drive it file to file.

A frame is KEPT (its source bytes, not re-coded) and counted when the decoder routes it to the host or to Pillow (grayscale,
progressive, arithmetic, CMYK, uncovered sampling, a device status that is not OK) or when the encoder's walk meets a coefficient or
DC difference beyond the standard tables' categories.  A scan that does not fit its slot is coded again into the plan's worst-case
slot: never dropped, never truncated.  By default the output carries the standard Huffman tables, so a source with optimised tables
grows.

``optimize=True`` is the counterpart of ``jpegtran -optimize``: the output is coded with tables built from its own symbol counts by the
procedure of ``jpeg_encode``.  PER FRAME (the file-to-file entries): tstar_jpeg_encode_scan_opt on the decoder's
coefficients, every frame under a header with its own four DHT segments; an interval of 0 (no DRI, no marker) is then allowed.  SHARED
(the compressed-resident arena, ``shared=True``): the OK frames of a chunk are cut, in order, into GROUPS of at most ``group_frames``
frames; a group's counts are the sum of its frames' counts, its four tables come from that sum, and every frame of the group is coded
with them and carries them (tstar_jpeg_encode_scan_grp) -- a decoder table set is 9016 bytes, more than tables of its own save a
20 KB frame, and the arena needs one per group and quantisation set only.  A frame, or every frame of a group, whose optimal table
would need a code longer than 32 bits is kept.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np

from . import jpeg
from . import jpeg_encode as JE

RECODE_DESC_DTYPE = np.dtype([("kind", "<u4"), ("hdr", "<u4"), ("src", "<u4"), ("src_off", "<u4"), ("src_len", "<u4"), ("table_set", "<i4"),
                              ("first_segment", "<u4"), ("n_segments", "<u4")])
NEW, KEPT = 0, 1
HEADER_PITCH = 1024
HEADER_PITCH_OPT = 1568            # rows of headers with tables of their own: at most 1566 bytes (csrc/jpeg_recode_core.h)
STATS = ("recoded", "kept", "bytes_in", "bytes_out")
GROUP_COUNT_LIMIT = 1_000_000_000  # what tstar_jpeg_huff_optimal and libjpeg's procedure are defined for
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


def recode_restart(restart_blocks, optimize: bool = False) -> int:
    """The interval of a file-to-file re-code: 1..65535 MCUs; 0 (no DRI, no marker) only together with ``optimize``."""
    _, blocks = JE._restart_values(None, restart_blocks)
    if blocks == 0 and optimize:
        return 0
    return recode_interval(restart_blocks)


def recode_optimize_mode(recode_optimize=None) -> bool:
    """The keyword when given, else TSTAR_JPEG_RECODE_OPTIMIZE ("1": on; "", "0": off)."""
    if recode_optimize is not None:
        return bool(recode_optimize)
    v = os.environ.get("TSTAR_JPEG_RECODE_OPTIMIZE", "")
    if v not in ("", "0", "1"):
        raise ValueError(f"TSTAR_JPEG_RECODE_OPTIMIZE={v!r}: expected 0 or 1")
    return v == "1"


def group_limit(blocks: int) -> int:
    """Frames a group holds at most: a block emits at most 64 symbols, so the group's counts stay within 10^9 (and within u32)."""
    return max(1, GROUP_COUNT_LIMIT // (int(blocks) * 64))


def make_groups(ok: np.ndarray, group_frames: int):
    """The frames of a chunk with ``ok`` set, in order, cut into consecutive groups of at most ``group_frames`` -> (group int32 [n],
    -1 where ``ok`` is not set; the number of groups)."""
    ok = np.asarray(ok, dtype=bool)
    group = np.full(len(ok), -1, dtype=np.int32)
    rank = np.cumsum(ok) - 1
    group[ok] = (rank[ok] // int(group_frames)).astype(np.int32)
    return group, int(group.max()) + 1 if ok.any() else 0


def _group_frames(group_frames, blocks: int) -> int:
    limit = group_limit(blocks)
    if group_frames is None:
        return limit
    g = int(group_frames)
    if not 1 <= g <= limit:
        raise ValueError(f"JPEG re-code: group_frames={group_frames!r}: expected 1..{limit} frames of {blocks} blocks")
    return g


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


def new_stats(optimize: bool = False) -> dict:
    """The counters of a re-code; ``optimize`` (the shared mode of an arena): ``optimized`` and ``table_sets`` too."""
    return {k: 0 for k in STATS + (("optimized", "table_sets") if optimize else ())}


def _count(stats: Optional[dict], kept: bool, n_in: int, n_out: int, optimize: bool = False, table_bytes: Optional[int] = None) -> None:
    """One frame into ``stats``.  ``optimize``: ``optimized`` counts the re-coded frames too.  ``table_bytes`` (the per-frame mode
    alone; the shared mode counts its ``table_sets`` instead): the bytes of the frame's DHT segments, 0 for a kept frame."""
    if stats is not None:
        stats["kept" if kept else "recoded"] = stats.get("kept" if kept else "recoded", 0) + 1
        stats["bytes_in"] = stats.get("bytes_in", 0) + int(n_in)
        stats["bytes_out"] = stats.get("bytes_out", 0) + int(n_out)
        if optimize:
            stats["optimized"] = stats.get("optimized", 0) + (0 if kept else 1)
        if table_bytes is not None:
            stats["table_bytes"] = stats.get("table_bytes", 0) + int(table_bytes)


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
def recode_host(datas: Sequence[bytes], restart: int, stats: Optional[dict] = None, optimize: bool = False, shared: bool = False,
                group_frames: Optional[int] = None, chunk: Optional[int] = None) -> List[bytes]:
    """Every file of ``datas`` re-coded with an interval of ``restart`` MCUs, or kept; files may differ in geometry.  ``optimize``:
    tables of the frame's own.  ``shared`` (with ``optimize``): the tables of its group, as the device path forms the groups -- the
    files of one geometry, in order, in chunks of ``chunk`` frames (default: the entropy runner's), each chunk through
    ``recode_host_chunk``."""
    restart = recode_restart(restart, optimize)
    if shared and not optimize:
        raise ValueError("JPEG re-code: shared tables are optimised tables: shared=True needs optimize=True")
    datas = [bytes(d) for d in datas]
    if not shared:
        out = []
        for data in datas:
            new = _recode_one_host(data, restart, optimize)
            _count(stats, new is None, len(data), len(data if new is None else new), optimize, _table_bytes(new) if optimize else None)
            out.append(data if new is None else new)
        return out
    out: List[Optional[bytes]] = [None] * len(datas)
    for geom, ids in _by_geometry(datas, out, stats, True, True).items():
        blocks, _ = jpeg._sizes(geom)
        step = jpeg.device_entropy_chunk(blocks, len(ids), chunk)
        k0 = 0
        while k0 < len(ids):
            part = ids[k0:k0 + step]
            part = part[:jpeg.device_entropy_take([len(datas[i]) for i in part])]
            for i, f in zip(part, recode_host_chunk([datas[i] for i in part], geom, restart, group_frames, stats)):
                out[i] = f
            k0 += len(part)
    return out


def _by_geometry(datas: Sequence[bytes], out: list, stats: Optional[dict], optimize: bool, shared: bool) -> dict:
    """The files the re-coder takes -> {geometry: their indices, in order}.  The others go into ``out`` as they are and are counted as
    kept, with the keys of the mode: ``table_sets`` (shared) or ``table_bytes`` (optimised tables per frame)."""
    if shared and stats is not None:
        stats.setdefault("table_sets", 0)
    by_geom: dict = {}
    for i, d in enumerate(datas):
        geom = covered(d)
        if geom is None:
            out[i] = d
            _count(stats, True, len(d), len(d), optimize, 0 if optimize and not shared else None)
        else:
            by_geom.setdefault(geom, []).append(i)
    return by_geom


def _table_bytes(new: Optional[bytes]) -> int:
    """Bytes of the four DHT segments of a file this module wrote (they follow each other in front of DRI / SOS); 0 for a kept frame."""
    if new is None:
        return 0
    at = new.index(b"\xff\xc4")
    n = 0
    for _ in range(4):
        n += 2 + int.from_bytes(new[at + n + 2:at + n + 4], "big")
    return n


def _decode_one_host(data: bytes, geom):
    """(coef int16 [1, blocks * 64], quant uint16 [1, 192]) of a covered file, or None when the decoder does not return OK."""
    blocks, _ = jpeg._sizes(geom)
    coef = np.empty((1, blocks * 64), dtype=np.int16)
    quant = np.empty((1, 192), dtype=np.uint16)
    status, _ = jpeg.entropy_batch([data], geom, coef, quant, 1)
    return (coef, quant) if status[0] == jpeg.OK else None


def _recode_one_host(data: bytes, restart: int, optimize: bool = False) -> Optional[bytes]:
    geom = covered(data)
    if geom is None:
        return None
    dec = _decode_one_host(data, geom)
    if dec is None:
        return None
    return code_host(dec[0], dec[1], geom, restart, optimize)


def code_host(coef: np.ndarray, quant: np.ndarray, geom, restart: int, optimize: bool = False) -> Optional[bytes]:
    """The second half of the host twin: one frame's quantised coefficients (int16 [1, blocks * 64], the decoder's layout) and its
    quant rows (uint16 [192]) -> the file with the interval, or None when the encoder's walk meets a coefficient or DC difference of
    a size category the standard tables have no code for, or (``optimize``) when a table of the frame's own overflows: the frame is
    then kept."""
    W, H, _, hs, vs = geom
    sub = _SUBSAMPLING[(hs, vs)]
    tables = {}
    scans, _, st = JE.scan_host(coef, W, H, sub, threads=1, restart_blocks=restart, optimize=optimize, tables=tables)
    if st[0] == JE.STATUS_BAD_COEF or (optimize and st[0] == JE.STATUS_HUFF_OVERFLOW):
        return None
    if st[0] != JE.STATUS_OK:
        raise RuntimeError("JPEG re-code (host): a scan did not fit the bound of its geometry")
    return _header(geom, quant, restart, tables["specs"][0] if optimize else None) + scans[0]


def _header(geom, quant, restart: int, sp=None) -> bytes:
    """SOI .. SOS of a re-coded frame: the source's quantisation rows and the tables the frame is coded with -- ``sp`` (SPEC_DTYPE
    [4]) in its four DHT segments, or the standard ones (None)."""
    W, H, _, hs, vs = geom
    q, sub = np.asarray(quant).reshape(3, 64), _SUBSAMPLING[(hs, vs)]
    return JE.header_from_tables(W, H, q, sub, restart) if sp is None else JE.header_from_tables_specs(W, H, q, sp, sub, restart)


def code_host_shared(coef: np.ndarray, geom, restart: int, group: np.ndarray, n_groups: int, counts: Optional[np.ndarray] = None):
    """The group-coding step of the host twin (tstar_jpeg_encode_scan_host_grp): coef int16 [m, blocks * 64], ``group`` int32 [m]
    (-1: not coded) -> (scans: bytes, or None for a frame that is kept; status int32 [m]; specs SPEC_DTYPE [n_groups, 4]; the groups'
    counts uint32 [n_groups, 4, 257]).  ``counts``: counts to build the tables from INSTEAD of the frames' own sums (a seam for
    tests: the overflow needs counts no picture of a testable size has)."""
    from . import _lib
    W, H, _, hs, vs = geom
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    m = coef.shape[0]
    p = JE.Plan(W, H, hs, vs, m, restart=restart, optimize=True)
    assert coef.size == m * p.blocks * 64, "coefficients do not match the geometry"
    group = np.ascontiguousarray(group, dtype=np.int32)
    slot = p.max_scan_bytes
    out = np.empty((m, slot), dtype=np.uint8)
    lengths, status = np.zeros(m, dtype=np.uint32), np.full(m, -1, dtype=np.int32)
    specs = np.zeros((n_groups, 4), dtype=JE.SPEC_DTYPE)
    hist = np.zeros((n_groups, 4, JE.HIST_BINS), dtype=np.uint32)
    stages = 7
    if counts is not None:
        hist[...] = np.asarray(counts, dtype=np.uint32).reshape(n_groups, 4, JE.HIST_BINS)
        stages = 6
    _lib.check(_lib.load().tstar_jpeg_encode_scan_host_grp(coef.ctypes.data, m, W, H, hs, vs, restart, group.ctypes.data, n_groups, stages,
                                                           hist.ctypes.data, specs.ctypes.data, out.ctypes.data, slot, lengths.ctypes.data,
                                                           status.ctypes.data, 1), "tstar_jpeg_encode_scan_host_grp")
    if (status == JE.STATUS_SHORT).any():
        raise RuntimeError("JPEG re-code (host): a scan did not fit the bound of its geometry")
    return [out[i, :lengths[i]].tobytes() if status[i] == JE.STATUS_OK else None for i in range(m)], status, specs, hist


def recode_host_chunk(datas: Sequence[bytes], geom, restart: int, group_frames: Optional[int] = None, stats: Optional[dict] = None,
                      counts: Optional[np.ndarray] = None, info: Optional[dict] = None) -> List[bytes]:
    """ONE chunk of the shared mode on the host: ``datas`` are the chunk's files (those of another geometry, or that the decoder does
    not return OK for, are kept and belong to no group); the others, in order, form groups of at most ``group_frames`` (default: the
    most the count bound allows).  ``info`` (optional dict) receives ``group``, ``specs``, ``hist`` and ``kept``."""
    geom = tuple(int(v) for v in geom)
    restart = recode_restart(restart, True)
    W, H, _, hs, vs = geom
    blocks, _ = jpeg._sizes(geom)
    gf = _group_frames(group_frames, blocks)
    if stats is not None:
        stats.setdefault("table_sets", 0)
    m = len(datas)
    coef = np.zeros((m, blocks * 64), dtype=np.int16)
    quant = np.zeros((m, 192), dtype=np.uint16)
    ok = np.zeros(m, dtype=bool)
    for j, d in enumerate(datas):
        dec = _decode_one_host(d, geom) if covered(d) == geom else None
        if dec is not None:
            coef[j], quant[j], ok[j] = dec[0][0], dec[1][0], True
    group, n_groups = make_groups(ok, gf)
    out = [bytes(d) for d in datas]
    kept = np.ones(m, dtype=bool)
    specs = np.zeros((0, 4), dtype=JE.SPEC_DTYPE)
    hist = np.zeros((0, 4, JE.HIST_BINS), dtype=np.uint32)
    if n_groups:
        scans, _, specs, hist = code_host_shared(coef, geom, restart, group, n_groups, counts)
        for j, sc in enumerate(scans):
            if sc is not None:
                out[j] = _header(geom, quant[j], restart, specs[group[j]]) + sc
                kept[j] = False
    for j, d in enumerate(datas):
        _count(stats, bool(kept[j]), len(d), len(out[j]), True)
    if stats is not None:
        stats["table_sets"] += len({(int(group[j]), quant[j].tobytes()) for j in range(m) if not kept[j]})
    if info is not None:
        info.update(group=group, specs=specs, hist=hist, kept=kept)
    return out


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
    return optimized_table_set(src_set, None)


_huffman_cache: dict = {}


def huffman_of_specs(specs) -> np.ndarray:
    """The six flat Huffman tables the planner makes of a file whose four DHT segments carry ``specs`` (SPEC_DTYPE [4]): planned from
    a smallest file with exactly those segments, so they are ``jpeg.plan_segments``' of any output file that carries them."""
    sp = np.ascontiguousarray(specs, dtype=JE.SPEC_DTYPE).reshape(4)
    key = sp.tobytes()
    if key not in _huffman_cache:
        if len(_huffman_cache) >= 4096:
            _huffman_cache.clear()
        f = JE.header_from_specs(8, 8, sp, 75, "4:4:4") + b"\x00\xff\xd9"
        plan = jpeg.plan_segments([f], (8, 8, 3, 1, 1))
        if plan.route[0] != jpeg.ROUTE_DEVICE or plan.table_sets.shape != (1, jpeg.TABLE_SET_BYTES):
            raise RuntimeError("JPEG re-code: the planner does not take the optimised tables of a group")
        _huffman_cache[key] = plan.table_sets[0, :_HUFF_BYTES].copy()
    return _huffman_cache[key]


def optimized_table_set(src_set: np.ndarray, specs) -> np.ndarray:
    """``recoded_table_set`` for a frame coded with the tables of ``specs`` (None: the standard ones)."""
    ts = np.array(src_set, dtype=np.uint8).reshape(jpeg.TABLE_SET_BYTES)
    ts[:_HUFF_BYTES] = _std_huffman() if specs is None else huffman_of_specs(specs)
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

    def __init__(self, plan: jpeg.SegmentPlan, src_lens, a: int, b: int, kept: np.ndarray, scan_len: np.ndarray, geom, restart: int,
                 specs: Optional[np.ndarray] = None, spec_of: Optional[np.ndarray] = None):
        """specs (SPEC_DTYPE [k, 4]) and spec_of (int [m]: the row of ``specs`` frame j is coded with): optimised tables; a header
        row is then one per (tables, quantisation set), and rows are HEADER_PITCH_OPT bytes."""
        W, H, _, hs, vs = geom
        m = b - a
        self.m, self.restart = m, restart
        self.n_mcu = ((W + 8 * hs - 1) // (8 * hs)) * ((H + 8 * vs - 1) // (8 * vs))
        n_int = (self.n_mcu + restart - 1) // restart if restart else 1
        self.pitch = HEADER_PITCH_OPT
        if specs is None:                                   # the standard tables: one row, None, that every frame is coded with
            specs, spec_of, self.pitch = [None], np.zeros(m, dtype=np.int64), HEADER_PITCH
        self.table_bytes = np.zeros(m, dtype=np.int64)
        self.table_keys = set()                             # (tables, quantisation set) of the re-coded frames
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
                sp = specs[int(spec_of[j])]
                qkey = (int(spec_of[j]), plan.quant[s].tobytes())
                if sp is not None:
                    self.table_keys.add(qkey)
                    self.table_bytes[j] = 4 * 21 + int(sp["nvals"].sum())
                if qkey not in headers:
                    headers[qkey] = len(self.header_bytes)
                    self.header_bytes.append(_header(geom, plan.quant[s], restart, sp))
                d["kind"], d["hdr"], d["n_segments"] = NEW, headers[qkey], n_int
                key = optimized_table_set(plan.table_sets[ts], sp).tobytes()
                out_len[j] = len(self.header_bytes[d["hdr"]]) + int(scan_len[j])
            d["table_set"] = -1 if key is None else sets.setdefault(key, len(sets))
        desc["first_segment"] = np.cumsum(desc["n_segments"], dtype=np.int64) - desc["n_segments"]
        self.desc, self.out_len, self.total = desc, out_len, int(out_len.sum())
        self.n_segments = int(desc["n_segments"].sum())
        self.table_sets = (np.stack([np.frombuffer(k, dtype=np.uint8) for k in sets]) if sets
                           else np.zeros((0, jpeg.TABLE_SET_BYTES), dtype=np.uint8))
        nh = max(1, len(self.header_bytes))
        self.headers = np.zeros((nh, self.pitch), dtype=np.uint8)
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
    """The host mirror of the assembly (tstar_jpeg_recode_assemble_host_opt) -> (output bytes uint8 [total], record buffer uint8)."""
    from . import _lib
    nrec, _ = recode_layout(pd.m, pd.n_segments)
    rec = _aligned16(np.zeros(nrec, dtype=np.uint8))
    out = np.zeros(max(16, pd.total), dtype=np.uint8)
    slots = np.ascontiguousarray(slots, dtype=np.uint8)
    scan_len = np.ascontiguousarray(scan_len, dtype=np.uint32)
    segs = plan.segments if len(plan.segments) else np.zeros(1, dtype=jpeg.SEGMENT_DTYPE)
    quant = _aligned16(plan.quant)
    _lib.check(_lib.load().tstar_jpeg_recode_assemble_host_opt(
        pd.desc.ctypes.data, pd.m, pd.n_segments, _aligned16(pd.headers).ctypes.data, pd.pitch, pd.header_len.ctypes.data, len(pd.header_len),
        _aligned16(slots).ctypes.data, slots.shape[1], scan_len.ctypes.data, pd.restart, pd.n_mcu, src_bytes.ctypes.data, plan.total_bytes,
        quant.ctypes.data, plan.frames.ctypes.data, segs.ctypes.data, len(plan.frames), len(plan.segments), rec.ctypes.data, rec.size,
        out.ctypes.data, pd.total), "tstar_jpeg_recode_assemble_host_opt")
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
    aligned addresses); the default is torch.empty.  ``optimize``: every frame coded with tables of its own
    (tstar_jpeg_encode_scan_opt); with ``shared`` with the tables of its group of at most ``group_frames`` frames
    (tstar_jpeg_encode_scan_grp).  Without ``optimize`` the launches, reads and bytes are those of the standard tables."""

    def __init__(self, geom, device, restart: int, stats: Optional[dict] = None, alloc=None, slot_bytes: Optional[int] = None,
                 optimize: bool = False, shared: bool = False, group_frames: Optional[int] = None):
        self.optimize, self.shared = bool(optimize), bool(shared)
        if self.shared and not self.optimize:
            raise ValueError("JPEG re-code: shared tables are optimised tables: shared=True needs optimize=True")
        self.geom, self.device, self.restart = tuple(int(v) for v in geom), device, recode_restart(restart, self.optimize)
        if not recodable(self.geom):
            raise ValueError(f"JPEG re-code: geometry {self.geom} is not re-coded (three components at 4:2:0, 4:2:2 or 4:4:4 are); its frames are kept")
        self.stats = stats
        W, H, _, hs, vs = self.geom
        one = JE.Plan(W, H, hs, vs, 1, restart=self.restart, optimize=self.optimize)
        self.blocks = one.blocks
        self.max_slot = (one.max_scan_bytes + 15) // 16 * 16
        self.first_slot = None if slot_bytes is None else min(self.max_slot, max(16, (int(slot_bytes) + 15) // 16 * 16))
        self.alloc = alloc if alloc is not None else self._alloc
        self.bufs = None                                    # m, slot, work, out, meta, specs (per-frame tables only)
        self.retried = 0
        self.group_frames = _group_frames(group_frames, self.blocks) if self.shared else None
        self.groups = None                                  # shared: group (int32 [n]), n, d_hist, d_specs of the chunk in work
        self.last_specs = None                              # optimize: the specs of the last piece (per frame) or chunk (per group)
        self.table_keys = set()
        if self.shared and stats is not None:
            stats.setdefault("table_sets", 0)

    def _alloc(self, nbytes: int):
        import torch
        return torch.empty(max(16, nbytes), dtype=torch.uint8, device=self.device)

    def _buffers(self, m: int, slot: int):
        import torch
        if self.bufs is None or self.bufs.m < m or self.bufs.slot != slot:
            self.bufs = None
            W, H, _, hs, vs = self.geom
            p = JE.Plan(W, H, hs, vs, m, slot, self.restart, self.optimize)
            new = lambda *shape, dtype=torch.uint8: torch.empty(shape, dtype=dtype, device=self.device)          # noqa: E731
            self.bufs = SimpleNamespace(m=m, slot=slot, work=new(p.workspace_bytes), out=new(m, slot), meta=new(2, m, dtype=torch.int32),
                                        specs=new(m, 4 * JE.SPEC_BYTES) if self.optimize and not self.shared else None)
        return self.bufs

    def recode_chunk(self, batch: jpeg.DeviceBatch, d_buf, d_coef, bad) -> List[Piece]:
        """The chunk ``batch`` (uploaded into ``d_buf``, its coefficients in ``d_coef``; ``bad``: the frames the device did not
        return OK for) -> the pieces of the new arena, in order."""
        import torch
        n = len(batch.datas)
        src_lens = np.fromiter((len(d) for d in batch.datas), dtype=np.int64, count=n)
        bad_mask = np.zeros(n, dtype=bool)
        bad_mask[list(bad)] = True
        # the first pass: twice the longest source file (the standard tables cost a source with optimised ones a few per cent, a
        # marker with its padding at most 3 bytes per interval); frames it is short of are coded again at the bound
        slot = self.first_slot or min(self.max_slot, (2 * int(src_lens.max()) + 4096 + 15) // 16 * 16)
        if self.shared:
            group, n_groups = make_groups(~bad_mask, self.group_frames)
            k = max(1, n_groups)
            self.groups = SimpleNamespace(group=group, n=n_groups,
                                          d_hist=torch.empty((k, 4 * JE.HIST_BINS), dtype=torch.int32, device=self.device),
                                          d_specs=torch.empty((k, 4 * JE.SPEC_BYTES), dtype=torch.uint8, device=self.device))
            self.last_specs = None
        self.table_keys = set()                             # (group, quantisation set) of the chunk's re-coded frames, counted once
        return self._pieces(batch, d_buf, d_coef, bad_mask, src_lens, 0, n, slot, True)

    def _scan(self, d_coef, a: int, m: int, slot: int, bufs, first: bool):
        """The scan stage of the mode for frames [a, a + m) of the chunk, into ``bufs`` -> spec_of: the row of the mode's specs
        (``_specs``) every frame is coded with (int [m], -1: none; None with the standard tables)."""
        import torch
        from . import _lib
        lib = _lib.load()
        W, H, _, hs, vs = self.geom
        head = (d_coef.data_ptr() + a * self.blocks * 128, m, W, H, hs, vs, self.restart)
        tail = (bufs.out.data_ptr(), slot, bufs.meta[0].data_ptr(), bufs.meta[1].data_ptr())
        work = (bufs.work.data_ptr(), bufs.work.numel())
        s = _lib.stream_ptr()
        if not self.optimize:
            _lib.check(lib.tstar_jpeg_encode_scan_rst(*head, *tail, *work, None, s), "tstar_jpeg_encode_scan_rst")
            return None
        if not self.shared:
            _lib.check(lib.tstar_jpeg_encode_scan_opt(*head, *tail, bufs.specs.data_ptr(), *work, None, s), "tstar_jpeg_encode_scan_opt")
            return np.arange(m)
        g = self.groups
        sub = g.group[a:a + m]
        if not (sub >= 0).any():
            return sub                                      # no frame of these has a group: all are kept, nothing is coded
        g0, g1 = int(sub[sub >= 0].min()), int(sub.max()) + 1
        local = np.where(sub >= 0, sub - g0, -1).astype(np.int32)
        span = np.zeros((g1 - g0, 2), dtype=np.int32)
        _lib.check(lib.tstar_jpeg_encode_group_spans(local.ctypes.data, m, g1 - g0, W, H, hs, vs, span.ctypes.data),
                   "tstar_jpeg_encode_group_spans")
        d_gs = torch.from_numpy(np.concatenate([local, span.reshape(-1)])).to(self.device)
        # the first pass covers the whole chunk: counts, sums, tables, scans.  A later pass (a larger slot, or a part of the chunk)
        # keeps the sums of the first: a group's tables do not depend on how the chunk is cut
        stages = 7 if first else 6
        _lib.check(lib.tstar_jpeg_encode_scan_grp(*head, local.ctypes.data, span.ctypes.data, d_gs.data_ptr(), d_gs.data_ptr() + 4 * m, g1 - g0,
                                                  stages, g.d_hist.data_ptr() + g0 * 16 * JE.HIST_BINS,
                                                  g.d_specs.data_ptr() + g0 * 4 * JE.SPEC_BYTES, *tail, *work, s), "tstar_jpeg_encode_scan_grp")
        return sub

    def _specs(self, bufs, m: int):
        """The tables of the mode, read back behind a scan stage that coded something (SPEC_DTYPE [k, 4]; None: the standard ones):
        one more small read per piece for the frames' own, one per chunk for the groups'."""
        if self.optimize and not self.shared:
            self.last_specs = bufs.specs[:m].cpu().numpy().view(JE.SPEC_DTYPE).reshape(m, 4)
        elif self.shared and self.last_specs is None:
            self.last_specs = self.groups.d_specs[:self.groups.n].cpu().numpy().view(JE.SPEC_DTYPE).reshape(self.groups.n, 4)
        return self.last_specs

    def _pieces(self, batch, d_buf, d_coef, bad_mask, src_lens, a: int, b: int, slot: int, first: bool = False) -> List[Piece]:
        import torch
        from . import _lib
        m = b - a
        bufs = self._buffers(m, slot)
        spec_of = self._scan(d_coef, a, m, slot, bufs, first)
        coded = not self.shared or bool((spec_of >= 0).any())
        if coded:
            meta_h = bufs.meta[:, :m].cpu().numpy()      # ONE read: lengths (u32 bits) and statuses
            scan_len, status = meta_h[0].view(np.uint32).astype(np.int64), meta_h[1]
        else:
            scan_len, status = np.zeros(m, dtype=np.int64), np.full(m, JE.STATUS_HUFF_OVERFLOW, dtype=np.int32)
        kept = bad_mask[a:b] | (status == JE.STATUS_BAD_COEF)
        if self.optimize:
            kept |= status == JE.STATUS_HUFF_OVERFLOW
        short = (status == JE.STATUS_SHORT) & ~kept
        if short.any():
            if slot >= self.max_slot:
                raise RuntimeError("JPEG re-code: a scan did not fit the bound of its geometry")
            self.retried += int(short.sum())
            step = max(1, min(m, RETRY_BYTES // self.max_slot))
            return [p for s0 in range(a, b, step)
                    for p in self._pieces(batch, d_buf, d_coef, bad_mask, src_lens, s0, min(b, s0 + step), self.max_slot)]
        specs = self._specs(bufs, m) if coded else None
        pd = PieceDesc(batch.plan, src_lens, a, b, kept, scan_len, self.geom, self.restart, specs, spec_of if specs is not None else None)
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
        _lib.check(_lib.load().tstar_jpeg_recode_assemble_opt(
            pd.desc.ctypes.data, d_desc.data_ptr(), m, pd.n_segments, d_headers.data_ptr(), pd.pitch, d_hlen.data_ptr(), len(pd.header_len),
            bufs.out.data_ptr(), slot, bufs.meta[0].data_ptr(), self.restart, pd.n_mcu, base, batch.total, base + parts["quant"][0],
            base + parts["frames"][0], base + parts["segments"][0], len(plan.frames), len(plan.segments), d_rec.data_ptr(), nrec,
            d_out.data_ptr(), pd.total, int(pd.out_len.max()), _lib.stream_ptr()), "tstar_jpeg_recode_assemble_opt")
        rec = d_rec[:nrec].cpu().numpy()                 # the records only: the bytes stay on the device
        per_frame = self.optimize and not self.shared       # tables of the frames' own are counted in bytes, shared ones in sets
        for j in range(m):
            _count(self.stats, bool(kept[j]), src_lens[a + j], pd.out_len[j], self.optimize, int(pd.table_bytes[j]) if per_frame else None)
        if self.shared and self.stats is not None:
            self.stats["table_sets"] += len(pd.table_keys - self.table_keys)
            self.table_keys |= pd.table_keys
        return [Piece(d_out[:pd.total], pd.plan_of(rec), pd.out_len.astype(np.uint32), kept, a)]


def runner_for(datas: Sequence[bytes], geom, device, chunk: Optional[int] = None):
    """An ``jpeg.EntropyRunner`` over ``datas`` (files of geometry ``geom``) outside an open."""
    ctx = jpeg.JpegOpen.for_geometry(jpeg.JpegList(list(datas)), list(range(len(datas))), device, geom)
    return jpeg.EntropyRunner(ctx, chunk, jpeg.split_min_bytes())


def recode_device(datas: Sequence[bytes], restart: int, device="cuda", chunk: Optional[int] = None, stats: Optional[dict] = None,
                  alloc=None, slot_bytes: Optional[int] = None, pieces_out: Optional[list] = None, optimize: bool = False,
                  shared: bool = False, group_frames: Optional[int] = None) -> List[bytes]:
    """``recode_host`` through the device path: files of one geometry are entropy-decoded, re-coded and assembled together, chunk by
    chunk, and only the finished pieces are read back.  ``pieces_out``: a list that receives (source files, Piece) of every piece.
    ``optimize`` / ``shared`` / ``group_frames``: ``recode_host``'s."""
    import torch
    restart = recode_restart(restart, optimize)
    datas = [bytes(d) for d in datas]
    out: List[Optional[bytes]] = [None] * len(datas)
    by_geom = _by_geometry(datas, out, stats, optimize, shared)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream()
        for geom, ids in by_geom.items():
            files = [datas[i] for i in ids]
            run = runner_for(files, geom, device, chunk)
            rec = DeviceRecoder(geom, device, restart, stats, alloc, slot_bytes, optimize, shared, group_frames)
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
