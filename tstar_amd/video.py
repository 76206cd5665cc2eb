"""Decoded-frame store resident in HBM.

The reference re-opens the file with decord on every read
(/root/reference/TStar/interface_searcher.py:157-169) and asks OpenCV for fps /
frame count (:60-65).  Here a video is decoded ONCE into a uint8 tensor
[N,H,W,3] (RGB) on the GPU and every later gather/resize is a HIP kernel
(tstar_frames_to_grid / tstar_frames_resize).  Decode itself (FFmpeg/VCN) is
outside the hot path (SURVEY.md 8f "next" row 3): raw 4:2:0 files (YUV4MPEG2) are
read and repacked on the device here (``load_y4m``); the compressed sequences Pillow
decodes in this image (animated GIF / WebP, AVIF sequences = AV1) go through
``load_pillow_sequence``; Motion-JPEG (.avi / .mjpeg) and folders or lists of JPEG frames are
entropy-decoded on the host and reconstructed by HIP kernels (``tstar_amd.jpeg``); other compressed
files need decord or cv2 on the host (rocDecode / FFmpeg are not in this build), synthetic videos
need nothing.
"""
from __future__ import annotations

import re
from typing import Optional

import numpy as np


def synthetic_lowres(n_frames: int, seed: int = 0) -> np.ndarray:
    """uint8 [N,10,17,3] noise lattice, one frozen RandomState stream."""
    return np.random.RandomState(seed).randint(0, 256, size=(n_frames, 10, 17, 3)).astype(np.uint8)


def _planted(n_frames: int, seed: int):
    """Seeded 5 % of frames get 1-2 solid rectangles: (frame, y0, y1, x0, x1, rgb) in 9x16 lattice units."""
    rs = np.random.RandomState(seed + 1)
    frames = np.nonzero(rs.random_sample(n_frames) < 0.05)[0]
    out = []
    for f in frames:
        for _ in range(1 + int(rs.randint(0, 2))):
            y0, x0 = int(rs.randint(0, 7)), int(rs.randint(0, 13))
            h, w = int(rs.randint(2, 4)), int(rs.randint(2, 5))
            rgb = tuple(int(v) for v in rs.randint(0, 256, 3))
            out.append((int(f), y0, min(y0 + h, 9), x0, min(x0 + w, 16), rgb))
    return out


def synthetic_frames_numpy(idx, n_frames: int, H: int = 360, W: int = 640, seed: int = 0) -> np.ndarray:
    """CPU statement of the synthetic video (integer arithmetic only): frames ``idx`` as uint8 [n,H,W,3].

    Frame = integer bilinear upsampling of the 10x17 lattice (cell size H/9 x W/16)
    + planted rectangles.  ``synthetic_video`` computes the same bytes on the GPU.
    """
    low = synthetic_lowres(n_frames, seed).astype(np.int32)
    cy, cx = H // 9, W // 16
    ys, xs = np.arange(H), np.arange(W)
    y0, fy = ys // cy, (ys % cy).astype(np.int32)
    x0, fx = xs // cx, (xs % cx).astype(np.int32)
    out = np.empty((len(idx), H, W, 3), dtype=np.uint8)
    rects = _planted(n_frames, seed)
    for k, i in enumerate(idx):
        L = low[int(i)]
        # separable form of the 4-term integer bilinear sum (identical integers, half the gathers)
        rows = L[:, x0] * (cx - fx)[None, :, None] + L[:, x0 + 1] * fx[None, :, None]          # [10, W, 3]
        fr = ((rows[y0] * (cy - fy)[:, None, None] + rows[y0 + 1] * fy[:, None, None]) // (cy * cx)).astype(np.uint8)
        for (f, ry0, ry1, rx0, rx1, rgb) in rects:
            if f == int(i):
                fr[ry0 * cy:ry1 * cy, rx0 * cx:rx1 * cx] = rgb
        out[k] = fr
    return out


class Lease:
    """Frames of a store that a kernel may read: ``frames`` (the tensor to pass), ``N`` (its frame count), ``idx`` (int32 tensor on
    the store's device: where the asked seconds sit in ``frames``, in the order asked).  ``done()`` is called once the kernels that
    read them are queued on the current stream; the positions may be given to other frames afterwards."""

    __slots__ = ("frames", "N", "idx", "_release")

    def __init__(self, frames, N: int, idx, release=None):
        self.frames, self.N, self.idx, self._release = frames, int(N), idx, release

    def done(self) -> None:
        release, self._release = self._release, None
        if release is not None:
            release()


class FrameStore:
    """A decoded video in HBM at the searcher's logical rate (1 frame per second):
    ``frames`` uint8 cuda tensor [N,H,W,3] with frames[s] = raw frame int(s * raw_fps)
    (the index map of interface_searcher.py:360), plus the raw stream's fps / frame count."""

    def __init__(self, frames, raw_fps: float, raw_total_frames: Optional[int] = None, name: str = "<frames>",
                 fmt: str = "rgb"):
        """``fmt``: "rgb" -> frames u8 [N,H,W,3]; "nv12" -> frames u8 [N, H*3/2, W] (luma plane + interleaved
        half-resolution UV plane), converted to RGB inside the ingest kernels (half the bytes per frame)."""
        if fmt not in ("rgb", "nv12"):
            raise ValueError("FrameStore fmt must be 'rgb' or 'nv12'")
        self.fmt = fmt
        self.frames = frames
        self.raw_fps = float(raw_fps)
        self.raw_total_frames = int(raw_total_frames if raw_total_frames is not None
                                    else round(frames.shape[0] * self.raw_fps))
        self.name = name
        self.decode_stats = None      # JPEG sources: {"device": n, "host": n, "pillow": n} frames decoded by each path
        self.entropy_stats = None     # JPEG sources: {"device": n, "host": n} frames run through each side's entropy decoder
        self.entropy_split_stats = None   # JPEG sources: {"split": n, "abandoned": n, "rounds_max": r} segments cut into sub-sequences
        self.jpeg_scale = 1               # JPEG sources: the frames are the file's pictures decoded at 1/jpeg_scale size ...
        self.source_size = None           # ... and (W, H) is the file's own picture size

    @property
    def num_seconds(self) -> int:
        return int(self.frames.shape[0])

    @property
    def device(self):
        return self.frames.device

    lease_frames = None      # the most distinct seconds one lease may name (None: any number)

    def lease(self, secs, d_idx=None) -> Lease:
        """The frames of the logical seconds ``secs`` for a kernel to read (see ``Lease``).  ``d_idx``: the same seconds as an int32
        tensor already on the device, when the caller has one.  A decoded store leases its whole tensor, the positions are the
        seconds themselves and ``done()`` does nothing."""
        if d_idx is None:
            import torch
            d_idx = torch.as_tensor([int(s) for s in secs], dtype=torch.int32, device=self.frames.device)
        return Lease(self.frames, self.frames.shape[0], d_idx)

    @property
    def shape(self):
        """(N, H, W, 3) of the RGB view, whatever the storage format."""
        if self.fmt == "nv12":
            n, h32, w = self.frames.shape
            return (int(n), int(h32) * 2 // 3, int(w), 3)
        return tuple(self.frames.shape)

    def host_frames(self, secs) -> np.ndarray:
        """Native-resolution RGB frames of the given logical seconds -> uint8 numpy [n,H,W,3]."""
        import torch
        secs = [int(i) for i in secs]
        if self.fmt == "nv12":
            from . import _lib
            N, H, W, _ = self.shape
            lease = self.lease(secs)
            out = torch.empty((len(secs), H, W, 3), dtype=torch.uint8, device=self.device)
            _lib.check(_lib.load().tstar_nv12_to_rgb(lease.frames.data_ptr(), lease.N, H, W, lease.idx.data_ptr(), len(secs),
                                                      out.data_ptr(), _lib.stream_ptr()), "tstar_nv12_to_rgb")
            lease.done()
            return out.cpu().numpy()
        step = self.lease_frames or max(1, len(secs))
        parts = []
        for s0 in range(0, len(secs), step):
            lease = self.lease(secs[s0:s0 + step])
            parts.append(lease.frames.index_select(0, lease.idx.long()))
            lease.done()
        if len(parts) == 1:
            return parts[0].cpu().numpy()
        _, H, W, _ = self.shape
        return torch.cat(parts).cpu().numpy() if parts else np.empty((0, H, W, 3), dtype=np.uint8)

    def jpeg_frames(self, secs, quality: int = 75, subsampling: str = "4:2:0", restart_rows=None, restart_blocks=None,
                    optimize: bool = False):
        """The given logical seconds as JPEG files (list of bytes), encoded on the device straight from the store: byte for
        byte Pillow's ``Image.fromarray(frame).save(buf, "JPEG", quality=, subsampling=)`` of ``host_frames(secs)``;
        ``restart_rows`` / ``restart_blocks`` are Pillow's ``restart_marker_rows`` / ``restart_marker_blocks``, ``optimize`` its
        ``optimize`` (Huffman tables built from each frame's own statistics: smaller files, the same pixels)."""
        from . import jpeg_encode
        return jpeg_encode.encode_frames((self, secs), quality, subsampling, restart_rows=restart_rows, restart_blocks=restart_blocks,
                                         optimize=optimize)

    def save_mjpeg(self, path: str, quality: int = 90, subsampling: str = "4:2:0", fps: Optional[float] = None, restart_rows=None,
                   restart_blocks=None, optimize: bool = False) -> int:
        """Write the store as Motion-JPEG (.avi: RIFF with one MJPG stream; .mjpeg / .mjpg: concatenated frames) at its logical
        rate, 1 frame per second unless ``fps`` is given, so that ``open_video(path)`` returns a store of the same seconds.  A
        file that would need OpenDML (1 GiB and above) is refused with a ValueError that names .mjpeg as the way out.
        ``restart_rows`` / ``restart_blocks`` (default: no markers) write every frame with restart intervals of that many MCU
        rows / MCUs; ``optimize=True`` writes every frame with optimised Huffman tables."""
        from . import jpeg_encode
        return jpeg_encode.save_mjpeg(self, path, quality, subsampling, fps, restart_rows=restart_rows, restart_blocks=restart_blocks,
                                      optimize=optimize)


class JpegFrameStore(FrameStore):
    """A Motion-JPEG video kept COMPRESSED in HBM (``open_video(..., resident="jpeg")``; built by ``jpeg_resident.load_resident``):
    the wanted frames' file bytes and the decode plan stay on the device, and ``lease(secs)`` decodes the frames that are not in
    the pool of ``pool_frames`` RGB slots on the current stream, without a host synchronisation.  Frames the device decoder does not
    cover sit decoded in permanent slots behind the pool.  There is no ``frames`` tensor: every reader goes through ``lease`` or
    ``host_frames``."""

    def __init__(self, arena, d_arena, sec_entry, geom, hw, exceptions, pool_frames: int, raw_fps: float,
                 raw_total_frames: Optional[int] = None, name: str = "<jpeg frames>", min_split_bytes: Optional[int] = None,
                 max_rounds: Optional[int] = None, jpeg_scale: int = 1):
        """``max_rounds``: rounds of the split path a fetch queues (default jpeg.SPLIT_MAX_ROUNDS).  Sub-sequences are cut from a
        segment's own first byte, so a segment converges in the round it converged in at open, wherever a fetch puts it: an open
        passes the most rounds any segment took, and a fetch queues that many launches instead of 48 (same coefficients).
        ``jpeg_scale``: the slots hold the frames decoded at 1/jpeg_scale size, ``hw`` is that size."""
        import torch
        from . import jpeg, jpeg_resident as JR
        self.fmt = "rgb"
        self.raw_fps = float(raw_fps)
        self.raw_total_frames = int(raw_total_frames if raw_total_frames is not None else round(len(sec_entry) * self.raw_fps))
        self.name = name
        self.decode_stats = self.entropy_stats = self.entropy_split_stats = None
        self.jpeg_scale, self.source_size = int(jpeg_scale), None
        self.arena, self.d_arena = arena, d_arena
        self._sec_entry = np.asarray(sec_entry, dtype=np.int64)
        self._geom = tuple(int(v) for v in geom) if geom is not None else None
        H, W = hw
        self._shape = (len(self._sec_entry), int(H), int(W), 3)
        dev = d_arena.device
        exc = sorted(exceptions)
        normal = arena.n_entries - len(exc)
        self.pool_frames = max(1, min(int(pool_frames), max(1, normal)))
        self._pool = JR.SlotPool(self.pool_frames, exc)
        self._slots = torch.empty((self.pool_frames + len(exc), H, W, 3), dtype=torch.uint8, device=dev)
        for k, e in enumerate(exc):
            self._slots[self.pool_frames + k].copy_(torch.as_tensor(exceptions[e]))
        self._min_split = jpeg.split_min_bytes() if min_split_bytes is None else int(min_split_bytes)
        self._max_rounds = jpeg.SPLIT_MAX_ROUNDS if max_rounds is None else max(1, min(int(max_rounds), jpeg.SPLIT_MAX_ROUNDS))
        self._err = torch.zeros((), dtype=torch.int32, device=dev)
        self._last_fetch = None                     # (stream key, event) of the last fetch: the next one reuses its workspace
        self._len = arena.len.astype(np.int64)
        self._nseg = arena.frames["n_segments"].astype(np.int64)
        seg_len = arena.segments["end"].astype(np.int64) - arena.segments["begin"]
        self._seg_longest = np.zeros(arena.n_entries, dtype=np.int64)
        np.maximum.at(self._seg_longest, arena.segments["frame"].astype(np.int64), seg_len)
        if self._geom is None or normal == 0:
            return
        # device copies of the arena's records (torch has no unsigned 32 / 64-bit tensors: same bits, signed types)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1)).to(dev)       # noqa: E731
        self._d_off, self._d_len = up(arena.off, np.int64), up(arena.len, np.int32)
        self._d_quant, self._d_frames = up(arena.quant, np.int16), up(arena.frames, np.int32)
        self._d_segments = up(arena.segments, np.int32) if len(arena.segments) else torch.zeros(6, dtype=torch.int32, device=dev)
        self._d_sets = up(arena.table_sets, np.uint8)
        # a fetch's workspace, sized once for the largest piece a fetch can be (never reallocated: fetches on several streams share
        # it, ordered by events)
        blocks, plane_bytes = jpeg._sizes(self._geom)
        if self.jpeg_scale > 1:
            plane_bytes = jpeg.scaled_sizes(self._geom, self.jpeg_scale)[2]
        c = self._piece = max(1, min(self.pool_frames, JR.FETCH_COEF_BUDGET // (blocks * 128)))
        keep = np.ones(arena.n_entries, dtype=bool)
        keep[exc] = False
        top = lambda a: int(np.sort(a[keep])[::-1][:c].sum())                                            # noqa: E731
        self._cap_bytes, self._cap_segments = top((self._len + 15) & ~15), top(self._nseg)
        self._d_batch = torch.empty(JR.gather_layout(self._cap_bytes, c, self._cap_segments)[0], dtype=torch.uint8, device=dev)
        self._d_coef = torch.empty((c, blocks * 64), dtype=torch.int16, device=dev)
        self._d_planes = torch.empty((c, plane_bytes), dtype=torch.uint8, device=dev)
        self._d_status = torch.empty(2 * self._cap_segments, dtype=torch.int32, device=dev)
        self._ws_bytes = jpeg.split_workspace_bytes(self._cap_bytes, self._cap_segments)
        self._d_ws = torch.empty(self._ws_bytes // 8 + 1, dtype=torch.int64, device=dev)

    @property
    def frames(self):
        raise AttributeError(f"{type(self).__name__} keeps {self.name} compressed and has no 'frames' tensor: read frames through "
                             "lease(secs) (device) or host_frames(secs)")

    @property
    def num_seconds(self) -> int:
        return self._shape[0]

    @property
    def shape(self):
        return self._shape

    @property
    def device(self):
        return self.d_arena.device

    @property
    def lease_frames(self):
        return self.pool_frames

    def _entries(self, secs):
        secs = [int(s) for s in secs]
        n = self._shape[0]
        for s in secs:
            if not 0 <= s < n:
                raise IndexError(f"second {s} outside the store's 0..{n - 1}")
        return self._sec_entry[secs] if secs else np.zeros(0, dtype=np.int64)

    def lease(self, secs, d_idx=None) -> Lease:
        """Slots of the pool that hold the frames ``secs`` until ``done()``: missing frames are decoded on the current stream first.
        ``d_idx`` (the seconds on the device) is of no use here: ``idx`` names slots.  ValueError when the request needs more free
        slots than the pool has."""
        import torch
        entries = self._entries(secs)
        stream = torch.cuda.current_stream(self.device)
        key = stream.cuda_stream
        slots, fill, waits = self._pool.acquire(entries, key)
        try:
            for ev in waits:
                stream.wait_event(ev)
            # ONE pinned staging tensor and one copy: the positions of the asked frames, then per piece the descriptor and the slots
            words = len(slots) + 7 * len(fill)
            h = torch.empty(max(1, words), dtype=torch.int32, pin_memory=True)
            hn = h.numpy()
            hn[:len(slots)] = slots
            d = torch.empty(max(1, words), dtype=torch.int32, device=self.device)
            pieces, at = [], len(slots)
            for c0 in range(0, len(fill), getattr(self, "_piece", 1)):
                part = fill[c0:c0 + self._piece]
                pieces.append(self._describe(part, hn, at))
                at += 7 * len(part)
            d.copy_(h, non_blocking=True)
            if fill:
                if self._last_fetch is not None and self._last_fetch[0] != key:
                    stream.wait_event(self._last_fetch[1])
                for piece in pieces:
                    self._fetch(piece, h, d, stream)
                ev = torch.cuda.Event()
                ev.record(stream)
                self._last_fetch = (key, ev)
                self._pool.filled([s for _, s in fill], key, ev)
        except Exception:
            self._pool.forget(fill)
            self._pool.release(slots)
            raise

        def release():
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._pool.release(slots, torch.cuda.current_stream(self.device).cuda_stream, ev)

        return Lease(self._slots, self._slots.shape[0], d[:len(slots)], release)

    def _describe(self, part, hn, at):
        """One piece of a fetch, [(entry, slot)]: its descriptor and slots into the staging words at ``at`` -> what _fetch needs."""
        from . import jpeg_resident as JR
        ids = [e for e, _ in part]
        desc, total, nseg = JR.gather_descriptor(ids, self._len, self._nseg)
        m = len(part)
        if total > self._cap_bytes or nseg > self._cap_segments:
            raise ValueError("JpegFrameStore: a fetch larger than the workspace sized at open")
        hn[at:at + 6 * m] = desc.view(np.int32)
        hn[at + 6 * m:at + 7 * m] = [s for _, s in part]
        longest = int(self._seg_longest[ids].max())
        return at, m, total, nseg, longest

    def _fetch(self, piece, h, d, stream) -> None:
        """Gather, entropy-decode and reconstruct one piece into its slots on ``stream``: three launchers, no synchronisation."""
        from . import _lib, jpeg, jpeg_resident as JR
        lib = _lib.load()
        at, m, total, nseg, longest = piece
        nbytes, q_at, f_at, s_at = JR.gather_layout(total, m, nseg)
        ws = jpeg.split_workspace_bytes(total, nseg)
        if nbytes > self._d_batch.numel() or ws > self._ws_bytes:
            raise ValueError("JpegFrameStore: a fetch larger than the workspace sized at open")
        a, base, sp = self.arena, self._d_batch.data_ptr(), stream.cuda_stream
        _lib.check(lib.tstar_jpeg_gather(self.d_arena.data_ptr(), self.d_arena.numel(), self._d_off.data_ptr(), self._d_len.data_ptr(),
                                         self._d_quant.data_ptr(), self._d_frames.data_ptr(), self._d_segments.data_ptr(), a.n_entries,
                                         len(a.segments), h.data_ptr() + 4 * at, d.data_ptr() + 4 * at, m, total, nseg, base,
                                         self._d_batch.numel(), sp), "tstar_jpeg_gather")
        st = self._d_status
        jpeg.split_launch((base, total, base + s_at, self._d_sets.data_ptr(), len(a.table_sets), base + f_at, m, nseg, *self._geom), longest,
                          self._min_split, self._max_rounds, self._d_ws.data_ptr(), self._ws_bytes, self._d_coef.data_ptr(), st.data_ptr(),
                          st.data_ptr() + 4 * self._cap_segments, sp)
        if self.jpeg_scale == 1:
            _lib.check(lib.tstar_jpeg_reconstruct_slots(self._d_coef.data_ptr(), base + q_at, m, *self._geom, self._d_planes.data_ptr(),
                                                        self._slots.data_ptr(), self.pool_frames, d.data_ptr() + 4 * (at + 6 * m), sp),
                       "tstar_jpeg_reconstruct_slots")
        else:
            _lib.check(lib.tstar_jpeg_reconstruct_slots_scaled(self._d_coef.data_ptr(), base + q_at, m, *self._geom, self.jpeg_scale,
                                                               self._d_planes.data_ptr(), self._slots.data_ptr(), self.pool_frames,
                                                               d.data_ptr() + 4 * (at + 6 * m), sp), "tstar_jpeg_reconstruct_slots_scaled")
        self._err.bitwise_or_(st[:nseg].max())

    def fetch_errors(self) -> int:
        """OR of the largest segment status of every fetch so far (0: every fetched frame decoded as it did at open).  Reads a device
        word: this call synchronises, the fetch path never does."""
        return int(self._err.item())

    def flush(self) -> int:
        """Forget every decoded frame no live lease holds (the next lease decodes again) -> how many."""
        return self._pool.flush()

    def source_frames(self, secs):
        """The original file bytes of the given seconds (list of bytes), copied from the arena."""
        out = []
        for e in self._entries(secs):
            o, n = int(self.arena.off[e]), int(self.arena.len[e])
            out.append(self.d_arena[o:o + n].cpu().numpy().tobytes())
        return out

    def pool_stats(self) -> dict:
        p = self._pool
        return {"hits": p.hits, "misses": p.misses, "evictions": p.evictions, "exceptions": len(p.permanent),
                "arena_bytes": int(self.d_arena.numel()), "pool_bytes": int(self._slots.numel())}


def synthetic_video(n_frames: int = 3600, H: int = 360, W: int = 640, seed: int = 0, raw_fps: float = 1.0,
                    device: str = "cuda", chunk: int = 256) -> FrameStore:
    """Build the synthetic video directly in HBM (torch integer ops = tensor plumbing; the
    bytes equal ``synthetic_frames_numpy``)."""
    import torch
    if H % 9 or W % 16:
        raise ValueError("synthetic video needs H % 9 == 0 and W % 16 == 0")
    low = torch.from_numpy(synthetic_lowres(n_frames, seed)).to(device).to(torch.int32)
    cy, cx = H // 9, W // 16
    ys = torch.arange(H, device=device)
    xs = torch.arange(W, device=device)
    y0, fy = ys // cy, (ys % cy).to(torch.int32)
    x0, fx = xs // cx, (xs % cx).to(torch.int32)
    wy0, wy1 = (cy - fy)[None, :, None, None], fy[None, :, None, None]
    wx0, wx1 = (cx - fx)[None, None, :, None], fx[None, None, :, None]
    frames = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, device=device)
    for s in range(0, n_frames, chunk):
        L = low[s:s + chunk]
        top = L[:, y0]
        bot = L[:, y0 + 1]
        v = top[:, :, x0] * (wy0 * wx0) + top[:, :, x0 + 1] * (wy0 * wx1) \
            + bot[:, :, x0] * (wy1 * wx0) + bot[:, :, x0 + 1] * (wy1 * wx1)
        frames[s:s + chunk] = torch.div(v, cy * cx, rounding_mode="floor").to(torch.uint8)
    for (f, ry0, ry1, rx0, rx1, rgb) in _planted(n_frames, seed):
        frames[f, ry0 * cy:ry1 * cy, rx0 * cx:rx1 * cx] = torch.tensor(rgb, dtype=torch.uint8, device=device)
    return FrameStore(frames, raw_fps, None, name=f"synthetic://n={n_frames},h={H},w={W},seed={seed}")


def synthetic_nv12_numpy(idx, n_frames: int, H: int = 360, W: int = 640, seed: int = 0) -> np.ndarray:
    """NV12 variant of the synthetic video (same lattice; channel 0 -> luma, channels 1,2 -> 4:2:0 chroma):
    uint8 [n, H*3/2, W].  Integer arithmetic only."""
    rgbish = synthetic_frames_numpy(idx, n_frames, H, W, seed)
    out = np.empty((len(idx), H * 3 // 2, W), dtype=np.uint8)
    out[:, :H, :] = 16 + (rgbish[..., 0].astype(np.int32) * 219 // 255).astype(np.uint8)         # limited-range luma
    uv = rgbish[:, ::2, ::2, 1:3].astype(np.int32)
    out[:, H:, :] = (16 + uv * 224 // 255).astype(np.uint8).reshape(len(idx), H // 2, W)          # interleaved U,V
    return out


def synthetic_video_nv12(n_frames: int = 3600, H: int = 360, W: int = 640, seed: int = 0, raw_fps: float = 1.0,
                         device: str = "cuda") -> FrameStore:
    """NV12 synthetic video in HBM (same bytes as ``synthetic_nv12_numpy``)."""
    import torch
    rgb = synthetic_video(n_frames, H, W, seed, raw_fps, device).frames
    out = torch.empty((n_frames, H * 3 // 2, W), dtype=torch.uint8, device=device)
    out[:, :H, :] = (16 + torch.div(rgb[..., 0].to(torch.int32) * 219, 255, rounding_mode="floor")).to(torch.uint8)
    uv = rgb[:, ::2, ::2, 1:3].to(torch.int32)
    out[:, H:, :] = (16 + torch.div(uv * 224, 255, rounding_mode="floor")).to(torch.uint8).reshape(n_frames, H // 2, W)
    return FrameStore(out, raw_fps, None, name=f"synthetic://n={n_frames},h={H},w={W},seed={seed},fmt=nv12", fmt="nv12")


def load_video_frames(video, num_frames: int = 8, fps: Optional[float] = None) -> np.ndarray:
    """The grounder's uniform frame loader (/root/reference/TStar/utilites.py:40-81): frames at raw
    indices floor(i * total / num_frames), RGB uint8 [n,H,W,3] -- served from the resident store (the
    stored frame nearest in time to each raw index when raw_fps != 1).  ``fps``: as ``open_video``."""
    import math
    st = open_video(video) if fps is None else open_video(video, fps=fps)
    total = st.raw_total_frames
    if total == 0:
        raise ValueError("Video has zero frames or could not retrieve frame count.")
    n = min(num_frames, total)
    step = total / n
    raw = [int(math.floor(i * step)) for i in range(n)]
    last = st.num_seconds - 1
    return st.host_frames([min(last, max(0, int(round(r / st.raw_fps)))) for r in raw])


def parse_y4m_header(path: str):
    """YUV4MPEG2 stream header -> dict(w, h, fps (float), fps_frac (num, den), chroma, data_offset, frame_bytes,
    frame_header_bytes, n_frames).  8-bit 4:2:0 only (C420, C420jpeg, C420mpeg2, C420paldv or no C tag)."""
    import os
    with open(path, "rb") as f:
        head = f.readline(4096)
        if not head.startswith(b"YUV4MPEG2 ") or not head.endswith(b"\n"):
            raise ValueError(f"Cannot open video file: {path} (not a YUV4MPEG2 stream)")
        tags = head[len(b"YUV4MPEG2 "):-1].split(b" ")
        kv = {t[:1].decode(): t[1:].decode() for t in tags if t}
        try:
            w, h = int(kv["W"]), int(kv["H"])
            num, den = (int(v) for v in kv.get("F", "25:1").split(":"))
        except (KeyError, ValueError):
            raise ValueError(f"Cannot open video file: {path} (malformed YUV4MPEG2 header)")
        chroma = kv.get("C", "420jpeg")
        if chroma not in ("420", "420jpeg", "420mpeg2", "420paldv"):
            raise ValueError(f"Cannot open video file: {path} (only 8-bit 4:2:0 YUV4MPEG2 is supported, got C{chroma})")
        if w % 2 or h % 2 or den <= 0 or num <= 0:
            raise ValueError(f"Cannot open video file: {path} (odd dimensions or bad frame rate)")
        off = f.tell()
        fh = f.readline(256)
        if not fh.startswith(b"FRAME"):
            raise ValueError(f"Cannot open video file: {path} (no FRAME marker)")
    fb = w * h * 3 // 2
    size = os.path.getsize(path)
    # every frame header of the streams we accept is the plain marker read above (parameters would change its length)
    n = (size - off) // (len(fh) + fb)
    return dict(w=w, h=h, fps=num / den, fps_frac=(num, den), chroma=chroma, data_offset=off, frame_bytes=fb,
                frame_header_bytes=len(fh), n_frames=int(n))


def load_y4m(path: str, device: str = "cuda", chunk: int = 64) -> FrameStore:
    """Decode front end for raw 4:2:0 video: a YUV4MPEG2 file is read ONCE, the frames the searcher can ever
    ask for (raw frame int(sec * fps) for every logical second, interface_searcher.py:360) are staged through two pinned
    host buffers, copied to HBM on a side stream and repacked I420 -> NV12 by a HIP kernel (tstar_i420_to_nv12) straight into
    the resident store, the host read of the next chunk overlapping the copy of the previous one.  Replaces the
    reopen-and-seek-per-call decord reader (:157-169) for such files; compressed streams would need rocDecode / FFmpeg,
    which this build does not have."""
    import torch
    from . import _lib
    hd = parse_y4m_header(path)
    w, h, fb = hd["w"], hd["h"], hd["frame_bytes"]
    if (w * h) % 64:          # before any store / pinned buffer is allocated (tstar_i420_to_nv12 moves 64-byte units)
        raise ValueError(f"Cannot open video file: {path} ({w}x{h}: the device repack needs W*H to be a multiple of 64)")
    n_sec = int(hd["n_frames"] / hd["fps"])
    if n_sec < 1:
        raise ValueError(f"Cannot open video file: {path} (shorter than one second)")
    want = [int(sec * hd["fps"]) for sec in range(n_sec)]
    lib = _lib.load()
    store = torch.empty((n_sec, h * 3 // 2, w), dtype=torch.uint8, device=device)
    pinned = [torch.empty((chunk, fb), dtype=torch.uint8).pin_memory() for _ in range(2)]
    staged = [torch.empty((chunk, fb), dtype=torch.uint8, device=device) for _ in range(2)]
    done = [None, None]
    side = torch.cuda.Stream()
    stride = hd["frame_header_bytes"] + fb
    with open(path, "rb") as f:
        for ci, s0 in enumerate(range(0, n_sec, chunk)):
            b = ci & 1
            if done[b] is not None:
                done[b].synchronize()                     # the pinned buffer's previous copy has left
            idx = want[s0:s0 + chunk]
            host = pinned[b].numpy()
            for j, fi in enumerate(idx):
                f.seek(hd["data_offset"] + fi * stride)
                if f.read(hd["frame_header_bytes"])[:5] != b"FRAME":       # per-frame parameters would shift every later frame
                    raise ValueError(f"Cannot open video file: {path} (no FRAME marker where frame {fi} should start: "
                                     f"frame headers of varying length are not supported)")
                got = f.readinto(memoryview(host[j]))
                if got != fb:
                    raise ValueError(f"Cannot open video file: {path} (truncated at frame {fi})")
            with torch.cuda.stream(side):
                staged[b][:len(idx)].copy_(pinned[b][:len(idx)], non_blocking=True)
                _lib.check(lib.tstar_i420_to_nv12(staged[b].data_ptr(), len(idx), h, w, store[s0:s0 + len(idx)].data_ptr(),
                                                  side.cuda_stream), "tstar_i420_to_nv12")
                done[b] = torch.cuda.Event()
                done[b].record(side)
    side.synchronize()
    return FrameStore(store, hd["fps"], hd["n_frames"], name=path, fmt="nv12")


def write_y4m(path: str, nv12_frames: np.ndarray, fps=(1, 1)) -> None:
    """uint8 [n, H*3/2, W] NV12 frames -> a YUV4MPEG2 file (planar I420 payload).  Test / example helper."""
    n, h32, w = nv12_frames.shape
    h = h32 * 2 // 3
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F{fps[0]}:{fps[1]} Ip A1:1 C420mpeg2\n".encode())
        for fr in nv12_frames:
            uv = fr[h:].reshape(h // 2, w // 2, 2)
            f.write(b"FRAME\n")
            f.write(fr[:h].tobytes())
            f.write(np.ascontiguousarray(uv[..., 0]).tobytes())
            f.write(np.ascontiguousarray(uv[..., 1]).tobytes())


_PIL_SEQUENCE_EXT = (".gif", ".webp", ".avif", ".avifs", ".apng", ".png")


def load_pillow_sequence(path: str, device: str = "cuda", chunk: int = 64) -> FrameStore:
    """Decode front end for the compressed multi-frame containers Pillow reads in this image -- animated GIF (LZW), WebP
    (VP8 / VP8L) and AVIF image sequences (AV1 through libavif) -- the only compressed "video" decoders available here
    (no FFmpeg, rocDecode, decord or cv2).  The stream's rate comes from the frame durations (frames / total duration);
    the frames the searcher can ever ask for (raw frame int(sec * fps) for every logical second,
    interface_searcher.py:360) are decoded once on the host, converted to RGB and copied to HBM in chunks -- the role
    decord's CPU reader plays in the reference (:157-169), without the reopen per call."""
    import torch
    from PIL import Image
    try:
        im = Image.open(path)
    except Exception as e:
        raise ValueError(f"Cannot open video file: {path} ({e})")
    with im:
        n = int(getattr(im, "n_frames", 1))
        w, h = im.size

        def frame(i):
            """RGB frame i and its duration in ms (WebP / AVIF report the duration only once the frame is decoded)."""
            im.seek(i)
            im.load()
            return np.asarray(im.convert("RGB"), dtype=np.uint8), float(im.info.get("duration", 0) or 0)

        def wanted(fps):
            """Raw frame of every logical second (non-decreasing; a stream slower than 1 fps names a frame repeatedly)."""
            n_sec = int(n / fps)
            return n_sec, [int(sec * fps) for sec in range(n_sec)]

        # One decode pass under the hypothesis that every frame lasts as long as the first (the usual case); the pass also
        # collects the real durations, and only a stream with varying durations is decoded a second time at its true rate.
        f0, d0 = frame(0)
        if n < 1 or d0 <= 0:
            raise ValueError(f"Cannot open video file: {path} (no frame durations: not an animated sequence)")
        fps = 1000.0 / d0
        for attempt in range(2):
            n_sec, want = wanted(fps)
            if n_sec < 1:
                raise ValueError(f"Cannot open video file: {path} (shorter than one second)")
            store = torch.empty((n_sec, h, w, 3), dtype=torch.uint8, device=device)
            host = np.empty((min(chunk, n_sec), h, w, 3), dtype=np.uint8)
            total_ms, filled, base, sec = 0.0, 0, 0, 0
            for i in range(n):
                fr, d = (f0, d0) if i == 0 else frame(i)
                total_ms += d
                while sec < n_sec and want[sec] == i:       # every second that maps to raw frame i, in order
                    host[filled] = fr
                    filled += 1
                    sec += 1
                    if filled == len(host) or sec == n_sec:
                        store[base:base + filled].copy_(torch.from_numpy(host[:filled]))
                        base, filled = base + filled, 0
            if base != n_sec:
                raise ValueError(f"Cannot open video file: {path} (decoded {base} of {n_sec} seconds)")
            true_fps = n * 1000.0 / total_ms
            if abs(true_fps - fps) <= 1e-9 * fps:
                break
            fps = true_fps                                  # varying durations: decode again at the stream's real rate
    return FrameStore(store, fps, n, name=path)


_SYN = re.compile(r"^synthetic://")


def open_video(video, device: str = "cuda", fps: Optional[float] = None, jpeg_entropy: Optional[str] = None,
               resident: Optional[str] = None, pool_frames: Optional[int] = None, jpeg_scale: Optional[int] = None,
               recode_blocks: Optional[int] = None, recode_optimize: Optional[bool] = None) -> FrameStore:
    """``video``: a FrameStore, a ``synthetic://n=..,h=..,w=..,seed=..,fps=..`` URL, a folder of .jpg / .jpeg frames or a
    list of JPEG paths / bytes (``fps`` frames per second, default 1), a .mjpeg / .mjpg stream (``fps`` default 25), a
    Motion-JPEG .avi, or another file path (.y4m, the Pillow sequences; else decoded at native rate through decord, else
    cv2; both absent -> ValueError like the reference's ``Cannot open video file`` at interface_searcher.py:61-62).
    ``jpeg_entropy``: where JPEG sources are entropy-decoded, "host" (default; TSTAR_JPEG_ENTROPY when absent) or "device".
    ``resident="jpeg"`` (TSTAR_JPEG_RESIDENT=1 when absent): a JPEG source stays compressed in HBM and its frames are decoded on
    demand into a pool of ``pool_frames`` slots (default 512; TSTAR_JPEG_POOL) -> a ``JpegFrameStore``.  The keyword on a source
    that is not JPEG is a ValueError; the variable alone leaves such a source as it is.
    ``jpeg_scale`` 2, 4 or 8 (TSTAR_JPEG_SCALE when absent; default 1): a JPEG source is decoded at 1/2, 1/4 or 1/8 size, byte for
    byte what Pillow's ``Image.draft`` gives, so the store -- decoded or compressed-resident -- holds [N, ceil(H / s), ceil(W / s), 3]
    and records ``jpeg_scale`` and ``source_size``.  Boxes of a search on it are in pixels of the stored frame.  The keyword on a
    source that is not JPEG, and any other value, is a ValueError; the variable alone leaves a source that is not JPEG as it is.
    ``recode_blocks`` N (1..65535 MCUs; TSTAR_JPEG_RECODE when absent; default: none) with ``resident="jpeg"``: the arena is re-coded
    losslessly at open with a restart interval of N MCUs (``jpeg_recode``), so that a fetch decodes one lane per interval instead of
    cutting one long scan; pixels, ``jpeg_scale`` and every reader are unchanged, ``store.recode_stats`` counts the frames.  The
    keyword without ``resident="jpeg"`` is a ValueError; the variable alone leaves a store that is not compressed-resident as it is.
    ``recode_optimize=True`` (TSTAR_JPEG_RECODE_OPTIMIZE=1 when absent) with a re-coding open: the re-coded frames carry optimised
    Huffman tables, one set per group of frames, so the arena shrinks instead of growing; ``store.recode_stats`` gains ``optimized``
    and ``table_sets``.  The keyword without a re-coding open (``recode_blocks`` or TSTAR_JPEG_RECODE) is a ValueError; the variable
    alone is then ignored."""
    if isinstance(video, FrameStore):
        return video
    from . import jpeg, jpeg_recode, jpeg_resident
    mode = jpeg_resident.resident_mode(resident)
    scale = jpeg.scale_mode(jpeg_scale)
    if recode_blocks is not None and mode != "jpeg":
        raise ValueError(f"open_video: recode_blocks={recode_blocks!r} re-codes the arena of a compressed-resident store: it needs resident=\"jpeg\"")
    recode = jpeg_recode.recode_mode(recode_blocks) if mode == "jpeg" else 0
    if recode_optimize and not recode:
        raise ValueError(f"open_video: recode_optimize={recode_optimize!r} optimises the tables of a re-coded arena: it needs recode_blocks "
                         "(or TSTAR_JPEG_RECODE) with resident=\"jpeg\"")
    optimize = bool(recode) and jpeg_recode.recode_optimize_mode(recode_optimize)
    other_codec = None
    if not (isinstance(video, str) and _SYN.match(video)):
        try:
            src = jpeg.open_source(video, fps)
        except jpeg.NotMotionJpeg as e:               # an AVI with another codec: decord / cv2 below, where a host has them
            src, other_codec = None, e
        if src is not None:
            try:
                if mode == "jpeg" and (resident is not None or not str(device).startswith("cpu")):
                    if optimize:
                        return jpeg_resident.load_resident(src, device, pool_frames, scale=scale, recode_blocks=recode, recode_optimize=True)
                    return jpeg_resident.load_resident(src, device, pool_frames, scale=scale, recode_blocks=recode or None)
                return jpeg.load_jpeg(src, device, entropy=jpeg_entropy, scale=scale)
            finally:
                src.close()
    if recode_blocks is not None:
        raise ValueError(f"open_video: recode_blocks={recode_blocks!r} needs a Motion-JPEG .avi, a .mjpeg stream or JPEG frames; {video!r} is none of them")
    if resident is not None:
        raise ValueError(f"open_video: resident={resident!r} needs a Motion-JPEG .avi, a .mjpeg stream or JPEG frames; {video!r} is none of them")
    if jpeg_scale is not None:
        raise ValueError(f"open_video: jpeg_scale={jpeg_scale!r} needs a Motion-JPEG .avi, a .mjpeg stream or JPEG frames; {video!r} is none of them")
    if fps is not None:
        raise ValueError("open_video: fps= applies to JPEG frame folders / lists and .mjpeg streams only")
    if isinstance(video, str) and _SYN.match(video):
        kv = dict(p.split("=") for p in video[len("synthetic://"):].split(",") if p)
        if kv.get("fmt", "rgb") == "nv12":
            return synthetic_video_nv12(int(kv.get("n", 3600)), int(kv.get("h", 360)), int(kv.get("w", 640)),
                                        int(kv.get("seed", 0)), float(kv.get("fps", 1.0)), device)
        return synthetic_video(int(kv.get("n", 3600)), int(kv.get("h", 360)), int(kv.get("w", 640)),
                               int(kv.get("seed", 0)), float(kv.get("fps", 1.0)), device)
    import torch
    if isinstance(video, str) and video.lower().endswith(".y4m"):
        import os
        if not os.path.isfile(video):
            raise ValueError(f"Cannot open video file: {video}")
        return load_y4m(video, device)
    if isinstance(video, str) and video.lower().endswith(_PIL_SEQUENCE_EXT):
        import os
        if not os.path.isfile(video):
            raise ValueError(f"Cannot open video file: {video}")
        return load_pillow_sequence(video, device)
    try:
        from decord import VideoReader, cpu  # type: ignore
        vr = VideoReader(video, ctx=cpu(0))
        fps = float(vr.get_avg_fps())
        total = len(vr)
        want = [int(sec * fps) for sec in range(int(total / fps))]
        parts = [torch.from_numpy(vr.get_batch(want[s:s + 256]).asnumpy()).to(device)
                 for s in range(0, len(want), 256)]
        return FrameStore(torch.cat(parts), fps, total, name=video)
    except ImportError:
        pass
    try:
        import cv2  # type: ignore
    except ImportError:
        if other_codec is not None:
            raise other_codec
        raise ValueError(f"Cannot open video file: {video} (neither decord nor cv2 is importable; "
                         "pass a tstar_amd.video.FrameStore or a synthetic:// URL)")
    cap = cv2.VideoCapture(video)
    if not cap.isOpened():
        raise ValueError(f"Cannot open video file: {video}")
    fps = cap.get(cv2.CAP_PROP_FPS)
    total = int(cap.get(cv2.CAP_PROP_FRAME_COUNT))
    want = [int(sec * fps) for sec in range(int(total / fps))]
    out, i, sec = [], 0, 0
    while sec < len(want):
        ok, fr = cap.read()
        if not ok:
            break
        if want[sec] == i:
            dev = torch.from_numpy(fr[:, :, ::-1].copy()).to(device)
            while sec < len(want) and want[sec] == i:       # a stream slower than 1 fps names a frame repeatedly
                out.append(dev)
                sec += 1
        i += 1
    cap.release()
    return FrameStore(torch.stack(out), fps, total, name=video)
