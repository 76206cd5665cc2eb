"""Host wrapper of the HIP YOLO-World detector (tstar_yolo_* in include/tstar_hip.h).

PyTorch is used for device memory and streams only; the network is executed by the hand-written f32 VALU kernels of
csrc/yolo.hip and csrc/yolo_conv.hip from the layer program tstar_amd.yolo_world.build_program emits.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from . import yolo_world as Y


# kernel forms of a conv op (TSTAR_YOLO_FORM_* in include/tstar_hip.h)
FORM_NAMES = ("tile64", "tile128", "wide", "sw8", "sw4", "halo_a16", "halo_a8", "halo_b16", "halo_b8", "direct")


def conv_plan(cin, src_ld, src_off, H, W, cout, dst_ld, dst_off, ks, stride, mode, B, max_batch, env_policy=False):
    """(form name, mt, nt) the conv launcher plans for one op (tstar_yolo_conv_plan; pure, needs no GPU).  ``env_policy``: apply
    this process's TSTAR_YOLO_* overrides instead of the default policy."""
    out = (C.c_int * 3)()
    rc = _lib.load().tstar_yolo_conv_plan(int(cin), int(src_ld), int(src_off), int(H), int(W), int(cout), int(dst_ld), int(dst_off), int(ks),
                                          int(stride), int(mode), int(B), int(max_batch), int(bool(env_policy)), out)
    _lib.check(rc, "tstar_yolo_conv_plan")
    return FORM_NAMES[out[0]], out[1], out[2]


def _program_args(prog, max_batch):
    """(arrays to keep alive, the arguments of tstar_yolo_create behind ``out``) of a program dict."""
    keep = [np.ascontiguousarray(prog[k], dtype=np.float32 if k == "blob" else np.int32) for k in ("blob", "ops", "bufs", "guides", "levels")]
    blob, ops, bufs, guides, levels = keep
    return keep, (blob.ctypes.data, blob.size, ops.ctypes.data, ops.shape[0], ops.shape[1], bufs.ctypes.data, bufs.shape[0], guides.ctypes.data,
                  guides.shape[0], levels.ctypes.data, levels.shape[0], int(prog["input_buf"]), int(max_batch))


def check_program(prog, max_batch: int = 16) -> None:
    """Every check tstar_yolo_create makes of a layer program (tstar_yolo_check_program; pure, needs no GPU).  Raises
    ``TStarHipError`` with the message create would give."""
    keep, args = _program_args(prog, max_batch)
    _lib.check(_lib.load().tstar_yolo_check_program(*args), "tstar_yolo_check_program")


@dataclass
class YoloResult:
    """Device tensors of one tstar_yolo_detect call (detections are sorted by descending score, padded to max_dets)."""
    scores: "object"        # f32 [B,max_dets]   (0 beyond n_det)
    labels: "object"        # i32 [B,max_dets]   (-1 beyond n_det)
    boxes: "object"         # f32 [B,max_dets,4] xyxy pixels of the passed image
    n_kept: "object"        # i32 [B]
    cell_conf: "object" = None   # f64 [B,rows*cols]
    cell_mask: "object" = None   # i32 view of u32 [B,rows*cols]
    dense_scores: "object" = None
    dense_boxes: "object" = None


class YoloDetector:
    """One YOLO-World-v2 detector resident on the current HIP device."""

    def __init__(self, state_dict, scale: str = "l", max_batch: int = 16):
        import torch
        if not torch.cuda.is_available():
            raise _lib.TStarHipError("YoloDetector needs a HIP device (torch.cuda.is_available() is False); tstar_amd has no CPU path")
        self._torch = torch
        self._lib = _lib.load()
        prog = state_dict if scale is None else Y.build_program(state_dict, scale)
        self.arch = prog.get("arch")
        self.conv_flops_per_image = Y.conv_flops(prog)
        keep, args = _program_args(prog, max_batch)                  # keep: the arrays args points into, alive across the call
        ops, bufs = keep[1], keep[2]
        h = C.c_void_p()
        _lib.check(self._lib.tstar_yolo_create(C.byref(h), *args), "tstar_yolo_create")
        self._h = h
        self.max_batch = int(max_batch)
        self.n_anchor = int(self._lib.tstar_yolo_num_anchors(h))
        self.Qs = {}
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.bufs = [tuple(int(v) for v in b) for b in bufs]
        self.n_ops = int(ops.shape[0])

    @classmethod
    def from_program(cls, prog, max_batch: int = 16) -> "YoloDetector":
        """A detector over a ready layer program: the dict ``yolo_world.build_program`` returns (blob, ops, bufs, guides, levels,
        input_buf), e.g. one assembled with ``yolo_world.program_from_builder`` from crafted ops (diagnostics and tests)."""
        return cls(prog, None, max_batch)

    # ---- diagnostics: the layer ops on caller data (tstar_yolo_buffer_copy / tstar_yolo_run_ops)
    def write_buffer(self, buf: int, data, B: int):
        """Images 0 .. B-1 of activation buffer ``buf`` <- data (cuda float32, B * H * W * C elements, NHWC)."""
        self._copy(buf, data, B, 1)

    def read_buffer(self, buf: int, B: int):
        """Images 0 .. B-1 of activation buffer ``buf`` as a cuda float32 tensor [B, H, W, C]."""
        if not 0 <= int(buf) < len(self.bufs):
            raise ValueError("read_buffer: no such activation buffer")
        out = self._torch.empty((max(int(B), 0),) + self.bufs[int(buf)], dtype=self._torch.float32, device=self.device)
        self._copy(buf, out, B, 0)
        return out

    def _copy(self, buf, t, B, to_buffer):
        torch = self._torch
        if not 0 <= int(buf) < len(self.bufs):
            raise ValueError("buffer copy: no such activation buffer")
        H, W, Cc = self.bufs[int(buf)]
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != int(B) * H * W * Cc:
            raise ValueError("buffer copy: data must be a contiguous cuda float32 tensor of B * H * W * C elements")
        _lib.check(self._lib.tstar_yolo_buffer_copy(self._h, int(buf), t.data_ptr(), int(B), int(to_buffer), _lib.stream_ptr()),
                   "tstar_yolo_buffer_copy")

    def run_ops(self, B: int, image_sets: Optional[Sequence[int]] = None) -> np.ndarray:
        """Run the op table on the buffers as they stand for images 0 .. B-1 (no preprocessing, no tail).  Returns int32 [n_ops]:
        per conv op the kernel form launched (``FORM_NAMES``), -1 for the other ops."""
        sets = None
        if image_sets is not None:
            sets = np.ascontiguousarray(image_sets, dtype=np.int32)
            if sets.shape != (int(B),):
                raise ValueError("run_ops: image_sets needs one slot per image")
        forms = np.full(self.n_ops, -2, dtype=np.int32)
        _lib.check(self._lib.tstar_yolo_run_ops(self._h, int(B), None if sets is None else sets.ctypes.data, forms.ctypes.data,
                                                _lib.stream_ptr()), "tstar_yolo_run_ops")
        return forms

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tstar_yolo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_text_feats(self, text_feats: np.ndarray, class_weight: Sequence[float], slot: int = 0):
        t = np.ascontiguousarray(text_feats, dtype=np.float32)
        w = np.ascontiguousarray(class_weight, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != Y.TEXT_DIM or w.shape != (t.shape[0],):
            raise ValueError("set_text_feats: text_feats [Q,512] and class_weight [Q]")
        _lib.check(self._lib.tstar_yolo_set_text_feats(self._h, int(slot), t.ctypes.data, w.ctypes.data, t.shape[0], _lib.stream_ptr()),
                   "tstar_yolo_set_text_feats")
        self.Qs[int(slot)] = t.shape[0]

    def set_class_weights(self, class_weight: Sequence[float], slot: int = 0):
        w = np.ascontiguousarray(class_weight, dtype=np.float64)
        if w.shape != (self.Qs.get(int(slot), 0),):
            raise ValueError("set_class_weights: one weight per installed query")
        _lib.check(self._lib.tstar_yolo_set_class_weights(self._h, int(slot), w.ctypes.data, len(w), _lib.stream_ptr()),
                   "tstar_yolo_set_class_weights")

    def _outputs(self, B, dev, grid_rows, grid_cols, max_dets, image_sets, want_dense, want_cells, who):
        torch = self._torch
        r = YoloResult(scores=torch.empty((B, max_dets), dtype=torch.float32, device=dev),
                       labels=torch.empty((B, max_dets), dtype=torch.int32, device=dev),
                       boxes=torch.empty((B, max_dets, 4), dtype=torch.float32, device=dev),
                       n_kept=torch.empty((B,), dtype=torch.int32, device=dev))
        if want_cells:
            r.cell_conf = torch.empty((B, grid_rows * grid_cols), dtype=torch.float64, device=dev)
            r.cell_mask = torch.empty((B, grid_rows * grid_cols), dtype=torch.int32, device=dev)
        sets = None
        if image_sets is not None:
            sets = np.ascontiguousarray(image_sets, dtype=np.int32)
            if sets.shape != (B,):
                raise ValueError(who + ": image_sets needs one slot per image")
        if want_dense:
            qs = {self.Qs.get(int(v), 0) for v in (sets if sets is not None else [0])}
            if len(qs) != 1:
                raise ValueError(who + ": dense scores need the same query count for every image")
            r.dense_scores = torch.empty((B, self.n_anchor, qs.pop()), dtype=torch.float32, device=dev)
            r.dense_boxes = torch.empty((B, self.n_anchor, 4), dtype=torch.float32, device=dev)
        return r, sets

    def detect(self, images, grid_rows: int = 1, grid_cols: int = 1, score_threshold: float = 0.12, max_dets: int = 50,
               image_sets: Optional[Sequence[int]] = None, want_dense: bool = False, want_cells: bool = True) -> YoloResult:
        """images: torch u8 cuda tensor [B,H,W,3] (RGB, as the searcher hands them to the reference)."""
        torch = self._torch
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_cuda:
            raise ValueError("detect: images must be a cuda uint8 tensor [B,H,W,3]")
        images = images.contiguous()
        B, H, W, _ = images.shape
        dev = images.device
        r, sets = self._outputs(B, dev, grid_rows, grid_cols, max_dets, image_sets, want_dense, want_cells, "detect")
        rc = self._lib.tstar_yolo_detect(self._h, images.data_ptr(), B, H, W, int(grid_rows), int(grid_cols),
                                         None if sets is None else sets.ctypes.data, float(score_threshold), int(max_dets),
                                         r.scores.data_ptr(), r.labels.data_ptr(), r.boxes.data_ptr(), r.n_kept.data_ptr(),
                                         _lib.ptr(r.cell_conf), _lib.ptr(r.cell_mask), _lib.ptr(r.dense_scores), _lib.ptr(r.dense_boxes),
                                         _lib.stream_ptr())
        _lib.check(rc, "tstar_yolo_detect")
        return r

    def postprocess(self, embeds, dfl, B: int, H: int, W: int, grid_rows: int = 1, grid_cols: int = 1, score_threshold: float = 0.12,
                    max_dets: int = 50, image_sets: Optional[Sequence[int]] = None, want_dense: bool = False,
                    want_cells: bool = True) -> YoloResult:
        """Diagnostic: the tail of detect (tstar_yolo_postprocess) on caller-supplied head tensors.  embeds / dfl: one cuda
        float32 tensor per head level, [B * size^2, 512] and [B * size^2, 64] (side * 16 + bin)."""
        torch = self._torch
        if len(embeds) != len(dfl):
            raise ValueError("postprocess: one embedding and one DFL tensor per head level")
        keep = []
        if len(embeds) != len(Y.STRIDES) or B < 1:
            raise ValueError("postprocess: one tensor pair per head level and at least one image")
        for e, d, stride in zip(embeds, dfl, Y.STRIDES):
            rows = B * (Y.IMG_SIZE // stride) ** 2
            for t, c in ((e, Y.TEXT_DIM), (d, 4 * Y.REG_MAX)):
                if t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != (rows, c):
                    raise ValueError("postprocess: level tensors must be cuda float32 [B*size^2, 512] and [B*size^2, 64]")
            keep.append((e.contiguous(), d.contiguous()))
        dev = keep[0][0].device
        r, sets = self._outputs(B, dev, grid_rows, grid_cols, max_dets, image_sets, want_dense, want_cells, "postprocess")
        pe = (C.c_void_p * len(keep))(*[e.data_ptr() for e, _ in keep])
        pd = (C.c_void_p * len(keep))(*[d.data_ptr() for _, d in keep])
        rc = self._lib.tstar_yolo_postprocess(self._h, pe, pd, len(keep), int(B), int(H), int(W), int(grid_rows), int(grid_cols),
                                              None if sets is None else sets.ctypes.data, float(score_threshold), int(max_dets),
                                              r.scores.data_ptr(), r.labels.data_ptr(), r.boxes.data_ptr(), r.n_kept.data_ptr(),
                                              _lib.ptr(r.cell_conf), _lib.ptr(r.cell_mask), _lib.ptr(r.dense_scores), _lib.ptr(r.dense_boxes),
                                              _lib.stream_ptr())
        _lib.check(rc, "tstar_yolo_postprocess")
        return r
