"""Open-vocabulary detector plug-ins with the reference's duck-typed surface
(/root/reference/TStar/interface_heuristic.py): ``HeuristicInterface`` (:28-37) and
``OWLInterface`` (:200-280), backed by the HIP OWL-ViT-B/32 scorer instead of HF
transformers + torch.

Same names, argument meaning and behaviour as the reference where a caller can observe it:

* ``reparameterize_object_list(target_objects, cue_objects)`` builds
  ``texts = [[name.strip()], ..., [' ']]`` (:268-280, the trailing blank query included);
* ``inference_detector(images, **kw)`` scores ONLY ``images[0]`` (:234), keeps detections with
  score > 0.005 (:243) in patch order and returns ``[Detections]`` with ``.xyxy`` f32 [n,4]
  (pixels of the passed image), ``.confidence`` f32 [n], ``.class_id`` int64 [n]; it also
  refreshes ``self.detections_inbatch`` (:256);
* ``bbox_visualization(images, detections_inbatch)`` draws on the arrays it is given (:259-267).

Documented deviations: no ``./annotated_image.png`` is written per call (the reference's debug
block, :248-255, costs ~50 ms per call); the text tower runs once per
``reparameterize_object_list`` instead of once per detector call (it is constant per question).

``YoloWorldInterface`` (:39-190) is the second backend: the reference reaches YOLO-World through mmdet /
mmyolo and a repository that is NOT part of its tree, so the detector here is a from-scratch HIP
implementation of the published YOLO-World-v2 architecture (f32 VALU kernels, no MFMA -- BASELINE
configs[3]) whose parity against the real model is unpinned (oracle/yolo_ref.py states why); the
WRAPPER semantics the reference itself defines are kept: ``texts`` layout with the trailing blank
query, ``score > 0.12`` then top-50, only ``images[0]``, ``detections_inbatch``.

Extensions used by tstar_amd.TStarSearcher's batched fast path (a foreign heuristic without them
still works through ``inference_detector``): ``set_class_weights``, ``score_batch``.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from . import weights as W
from . import _lib
from .tokenizer import encode_queries


@dataclass
class Detections:
    """Minimal stand-in for ``supervision.Detections`` (the fields the searcher reads,
    /root/reference/TStar/interface_searcher.py:134)."""
    xyxy: np.ndarray
    confidence: np.ndarray
    class_id: np.ndarray

    def __len__(self) -> int:
        return int(self.xyxy.shape[0])


# what ``annotated_batch`` / ``_detections_from`` raise (ValueError) on a ``score_batch(..., boxes=False)`` result
NO_BOXES_ERROR = "this result was scored with boxes=False and holds no boxes; score the images with boxes=True to draw or list detections"


def _env_int(name: str, default):
    v = os.environ.get(name)
    if v is None or v.strip() == "":
        return default
    try:
        return int(v)
    except ValueError:
        raise ValueError(f"{name} must be an integer, not {v!r}") from None


class HeuristicInterface:
    def __init__(self, heuristic_type: str = "owl-vit", **kwargs):
        """Base of the detector plug-ins (empty in the reference too, interface_heuristic.py:28-37)."""


class OWLInterface(HeuristicInterface):
    def __init__(self, model_name_or_path: str = "google/owlvit-base-patch32", device: str = "cuda",
                 max_batch: Optional[int] = None, synthetic_seed: Optional[int] = None, state_dict: Optional[Dict] = None,
                 weights_dtype: Optional[str] = None, allow_standin_tokenizer: Optional[bool] = None,
                 patch_size: Optional[int] = None, input_size=None, family: Optional[str] = None,
                 feature_cache_frames: Optional[int] = None):
        """``device`` must be a HIP device (default "cuda" as in the reference, :201).

        ``feature_cache_frames=N`` (not given: ``TSTAR_FEATURE_CACHE``; default 0 = off): keep the query-independent detector
        tensors of up to N verification frames (a RECORD per frame, ``npatch * 518 * 4`` bytes: 1.19 MB at B/32 768 x 768) in a
        pool on the device, so that a later question about the same video skips the vision tower for the frames an earlier one
        verified -- ``score_frames`` / ``index_frames`` / ``feature_cache_stats``; ``TStarSearcher`` verifies through
        ``score_frames`` when the cache is on.  No result changes: every output equals the uncached call bit for bit.

        Supported checkpoints: OWL-ViT B/32 (``google/owlvit-base-patch32``, the default) and B/16
        (``google/owlvit-base-patch16``), and OWLv2 B/16 (``google/owlv2-base-patch16``, ``-ensemble``, ``-finetuned``: image
        960, patch 16).  The geometry, the model family included, comes from the checkpoint (its config.json, cross-checked
        against the tensor names and shapes; ``weights.geometry_of_checkpoint``) or from the keys and shapes of a given
        ``state_dict`` (``owlvit.*`` / ``owlv2.*``); any other geometry (L/14, OWLv2 at image 768, ...) raises ValueError before
        anything is allocated on the device.  An OWLv2 heuristic pre-processes as HF's ``Owlv2ImageProcessorPil`` does (pad to a
        square, Gaussian anti-aliasing, linear resize; bit for bit), scales boxes by max(H, W) as its post-processing does, and
        ``self.scorer.score(..., objectness=True)`` returns HF's ``objectness_logits``.

        Image-guided (one-shot) queries, both families: ``set_query_images({name: image})`` registers example images; from then
        on any object NAME found in the registry is represented by its example's embedding (HF's ``embed_image_query``:
        ``image_guided_detection`` up to the query vector) instead of its text, in every way queries are installed; an
        image-backed query is scored, thresholded and weighted exactly like a text query.  An example may be a REGION of an
        image: ``{name: (image, (x0, y0, x1, y1))}``, the box in pixels of the example.  ``detect_image_guided`` is HF's whole
        one-shot pipeline, ``image_guided_detection`` + ``post_process_image_guided_detection`` (NMS, per-image score
        rescaling), outside the search loop.
        ``family`` ("owlvit" / "owlv2") chooses the family of SYNTHETIC weights; not given, it is ``TSTAR_OWL_FAMILY``, else
        "owlv2" when ``model_name_or_path`` contains ``owlv2``, else "owlvit"; given together with real weights it must agree
        with them.  ``patch_size`` (32 or 16) chooses
        the geometry of SYNTHETIC weights (default 32); given together with real weights it must agree with them.  The
        geometry is kept as ``self.geometry`` (``weights.OwlGeometry``); ``inference_detector`` returns
        ``self.geometry.npatch`` detections (patch order) when every patch passes the threshold.

        ``input_size=(height, width)``: the size every image is resampled to (Pillow bicubic) before the vision tower, fixed
        for the heuristic's life; default the checkpoint's own 768 x 768.  Any other size is HF's
        ``forward(..., interpolate_pos_encoding=True)`` behind an image processor of that ``size``: the position table is
        resampled to the (height / patch) x (width / patch) grid and ``box_bias`` is built for it.  Each side must be a
        positive multiple of the patch size and the grid may hold at most 3600 patches (ValueError otherwise, before anything
        is allocated).  ``self.geometry`` then carries the size (``geometry.input_size``, ``geometry.npatch``) and compares
        unequal to ``weights.B32`` / ``B16``; ``geometry.checkpoint`` is the checkpoint's own.

        Under an UNCHANGED ``TStarFramework`` the heuristic is built by ``initialize_heuristic(heuristic_type)`` without keyword
        arguments (TStarFramework.py:171-187, 207), so the four arguments a deployment chooses can also come from the environment
        -- read only when the keyword is not given: ``TSTAR_WEIGHTS_DTYPE`` (``weights_dtype``; default "f32"),
        ``TSTAR_MAX_BATCH`` (``max_batch``; default 32), ``TSTAR_SYNTHETIC_SEED`` (``synthetic_seed``; unset = no synthetic
        weights: a missing checkpoint raises) and ``TSTAR_INPUT_SIZE`` (``input_size`` as ``HEIGHTxWIDTH``, e.g. ``448x768``;
        unset = the checkpoint's own size).

        Weights: ``state_dict`` (HF names) if given; else a local safetensors checkpoint of
        ``model_name_or_path`` if one exists on disk; else, only when ``synthetic_seed`` is not None,
        seeded synthetic weights (no checkpoint can be downloaded: there is no network).
        ``weights_dtype="bf16"`` rounds every weight matrix to bfloat16 (BASELINE config 5) and runs the
        GEMMs on the bf16 matrix pipe with the float32 activations carried as two round-to-nearest bf16
        terms (16 significand bits): products are exact and accumulate in float32; scores stay within
        ~1e-5 of a CPU float32 run on the same rounded weights (contract 1e-3).  ``"bf16_exact"`` splits
        the activations exactly into three terms instead (3 matrix products per algorithmic product):
        equal to that CPU run up to summation order.

        ``allow_standin_tokenizer``: the hash stand-in of tstar_amd.tokenizer is only meaningful with
        synthetic weights; default (None) = allowed exactly when the weights are the seeded synthetic
        ones.  With a real checkpoint and no CLIP vocab on disk, installing queries raises instead of
        feeding made-up ids to the real text tower."""
        import torch
        from .owl import OwlScorer
        if not str(device).startswith("cuda"):
            raise ValueError("tstar_amd.OWLInterface runs on the GPU only (device='cuda[:i]'); it has no CPU path")
        if weights_dtype is None:
            weights_dtype = os.environ.get("TSTAR_WEIGHTS_DTYPE") or "f32"
        if weights_dtype not in ("f32", "bf16", "bf16_exact", "f32x3"):
            raise ValueError(f"weights_dtype (or TSTAR_WEIGHTS_DTYPE) must be 'f32', 'bf16', 'bf16_exact' or 'f32x3', not {weights_dtype!r}")
        if max_batch is None:
            max_batch = _env_int("TSTAR_MAX_BATCH", 32)
        if synthetic_seed is None and state_dict is None:
            synthetic_seed = _env_int("TSTAR_SYNTHETIC_SEED", None)
        dev = torch.device(device)
        if dev.index is not None:
            torch.cuda.set_device(dev.index)
        if family is None:
            family = os.environ.get("TSTAR_OWL_FAMILY") or None
        family_given = family is not None
        if family is None:
            family = "owlv2" if "owlv2" in str(model_name_or_path).lower() else "owlvit"
        if family not in W.FAMILIES:
            raise ValueError(f"family (or TSTAR_OWL_FAMILY) must be one of {W.FAMILIES}, not {family!r}")
        if patch_size is not None and not (family == "owlv2" and family_given):
            W.geometry_for_patch(int(patch_size))                  # an unsupported value fails here, whatever the weights
        input_size = W.resolve_input_size(input_size)              # a malformed TSTAR_INPUT_SIZE fails here
        if state_dict is None:
            ckpt = W.find_pretrained(model_name_or_path)
            if ckpt is not None:
                geometry = W.geometry_of_checkpoint(ckpt)          # before the weights are read or anything is allocated
                W.with_input_size(geometry, input_size)            # likewise
                state_dict = W.load_safetensors_state_dict(ckpt)
                self.weights_source = ckpt
            elif synthetic_seed is not None:
                geometry = W.geometry_for_family(family, None if patch_size is None else int(patch_size))
                W.with_input_size(geometry, input_size)
                state_dict = W.synthetic_state_dict(int(synthetic_seed), geometry=geometry)
                self.weights_source = f"synthetic(seed={int(synthetic_seed)})"
            else:
                raise FileNotFoundError(
                    f"no local checkpoint for {model_name_or_path!r} (offline); pass synthetic_seed=<int> "
                    "for seeded synthetic OWL-ViT weights (B/32, or B/16 with patch_size=16; OWLv2 B/16 with family='owlv2' or a "
                    "model name containing 'owlv2') or state_dict=<HF state dict>")
        else:
            geometry = W.geometry_of_state_dict(state_dict)
            self.weights_source = "state_dict"
        if patch_size is not None and int(patch_size) != geometry.patch_size:
            raise ValueError(f"patch_size={int(patch_size)} disagrees with the weights of {self.weights_source!r}, which are "
                             f"{geometry.name} (patch {geometry.patch_size})")
        if family_given and family != geometry.family:
            raise ValueError(f"family={family!r} disagrees with the weights of {self.weights_source!r}, which are {geometry.name} "
                             f"({geometry.family})")
        geometry = W.with_input_size(geometry, input_size)
        self.geometry = geometry
        self.family = geometry.family
        if allow_standin_tokenizer is None:
            allow_standin_tokenizer = self.weights_source.startswith("synthetic(")
        self.allow_standin_tokenizer = bool(allow_standin_tokenizer)
        if weights_dtype in ("bf16", "bf16_exact"):
            state_dict = W.round_weights_to_bf16(state_dict)
        self.weights_dtype = weights_dtype
        self.model_name_or_path = model_name_or_path
        self.scorer = OwlScorer(W.pack_blob(state_dict, W.vision_spec(geometry), geometry), W.pack_blob(state_dict, W.text_spec(geometry)),
                                max_batch=max_batch, weights_mode=weights_dtype, patch_size=geometry.patch_size,
                                input_size=None if geometry == geometry.checkpoint else geometry.input_size, family=geometry.family)
        self.device = device
        from . import feature_cache as FC
        if feature_cache_frames is None:
            feature_cache_frames = FC.frames_from_env()
        if int(feature_cache_frames) < 0:
            raise ValueError("feature_cache_frames must not be negative")
        self.feature_cache = None                     # tstar_amd.feature_cache.FeatureCache when the cache is on
        if int(feature_cache_frames) > 0:
            # max_batch scratch slots past the pool proper: frames the full pool has no room for are scored from there
            self.feature_cache = FC.FeatureCache(int(feature_cache_frames), scratch=int(max_batch))
            self.scorer.records_reserve(int(feature_cache_frames) + int(max_batch))
        self.texts = ["couch", "table", "woman"]      # as the reference leaves it before reparameterisation (:203)
        self.detections_inbatch: List[Detections] = []
        self._class_weight: Optional[np.ndarray] = None
        self._ids = None
        self._query_images: Dict[str, np.ndarray] = {}       # name -> raw class embedding f32 [512] of its example image
        self.query_image_info: Dict[str, Dict] = {}

    # ---- image-guided queries ------------------------------------------------------------
    @staticmethod
    def _load_example(img, what: str) -> np.ndarray:
        from PIL import Image
        if isinstance(img, (str, os.PathLike)):
            with Image.open(img) as im:
                img = np.asarray(im.convert("RGB"), dtype=np.uint8)
        img = np.ascontiguousarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"{what} must be an HxWx3 uint8 RGB image or a path")
        return img

    @staticmethod
    def _relative_box(box, H: int, Wd: int, what: str) -> np.ndarray:
        """A query box in pixels of its H x W example -> float32 [4] relative (x0, y0, x1, y1), each ``float32(x) / float32(W)``;
        ValueError when the box is empty, inverted or reaches outside the image."""
        try:
            b = np.asarray(box, dtype=np.float32).reshape(-1)
        except (TypeError, ValueError):
            b = np.zeros(0, np.float32)
        if b.shape != (4,) or not np.isfinite(b).all():
            raise ValueError(f"{what}: the query box must be four finite numbers (x0, y0, x1, y1) in pixels")
        x0, y0, x1, y1 = (float(v) for v in b)
        if not (0 <= x0 < x1 <= Wd and 0 <= y0 < y1 <= H):
            raise ValueError(f"{what}: the query box ({x0:g}, {y0:g}, {x1:g}, {y1:g}) is empty, inverted or outside the "
                             f"{Wd} x {H} example image")
        return b / np.array([Wd, H, Wd, H], dtype=np.float32)

    def _embed_examples(self, arrays: Dict[object, np.ndarray], boxes: Dict[object, Optional[np.ndarray]]):
        """{key: example image} (+ {key: relative box or None}) -> {key: (ImageQueryResult, row)}: the examples of one size in one
        batched ``OwlScorer.embed_image_queries`` call."""
        import torch
        by_shape: Dict[tuple, list] = {}
        for key, img in arrays.items():
            by_shape.setdefault(img.shape, []).append(key)
        out = {}
        unit = np.array([0, 0, 1, 1], dtype=np.float32)
        for keys in by_shape.values():
            qb = None
            if any(boxes.get(k) is not None for k in keys):
                qb = np.stack([unit if boxes.get(k) is None else boxes[k] for k in keys])
            d_imgs = torch.from_numpy(np.stack([arrays[k] for k in keys])).cuda()
            r = self.scorer.embed_image_queries(d_imgs) if qb is None else self.scorer.embed_image_queries(d_imgs, query_boxes=qb)
            for i, key in enumerate(keys):
                out[key] = (r, i)
        return out

    def set_query_images(self, images: Dict[str, object]):
        """Register example images: ``{name: HxWx3 uint8 RGB array, or the path of an image file}``, or ``{name: (image_or_path,
        (x0, y0, x1, y1))}`` when only a region of the example is meant -- the box in pixels of the example; the whole example
        still goes through the vision tower, so the region keeps its surroundings, and the box takes the place of HF's whole-image
        query box in the selection (``OwlScorer.embed_image_queries(..., query_boxes=)``).  They are embedded at once
        (images of one size in one batched ``OwlScorer.embed_image_queries`` call) and the embeddings cached; from the next
        ``reparameterize_object_list`` / ``install_queries`` / ``install_queries_many`` on, a target or cue object whose name
        (after ``.strip()``) is registered is represented by its example's embedding instead of its text -- ``texts``, labels,
        class weights, the trailing blank query and the 32-query limit are as before, so a searcher needs no change.
        ``query_image_info[name]`` = ``{"best_index", "box_cxcywh", "n_selected", "giou_fallback", "query_box"}`` (``query_box``:
        the relative float32 box, None for a whole image).  An example for which HF
        would produce no query (no box within 80 % of the best overlap: every generalized IoU negative) raises ValueError naming
        the object, as does a box that is empty, inverted or outside its image; nothing is registered then.  Queries already
        installed are not touched."""
        arrays, boxes = {}, {}
        for name, img in images.items():
            key = str(name).strip()
            if not key:
                raise ValueError("set_query_images: an object name must not be blank")
            box = None
            if isinstance(img, tuple):
                if len(img) != 2:
                    raise ValueError(f"set_query_images: {key!r} must be an image, a path, or (image_or_path, (x0, y0, x1, y1))")
                img, box = img
            arrays[key] = self._load_example(img, f"set_query_images: {key!r}")
            boxes[key] = None if box is None else self._relative_box(box, arrays[key].shape[0], arrays[key].shape[1],
                                                                      f"set_query_images: {key!r}")
        embeds, info = {}, {}
        for key, (r, i) in self._embed_examples(arrays, boxes).items():
            if int(r.status[i]) == 2:
                raise ValueError(f"set_query_images: no query can be formed from the example image of {key!r}: none of its "
                                 "predicted boxes overlaps the " + ("whole image" if boxes[key] is None else "query box") +
                                 " (empty selection in HF's embed_image_query)")
            embeds[key] = r.embeds[i].copy()
            info[key] = dict(best_index=int(r.best[i]), box_cxcywh=r.boxes_cxcywh[i].copy(), n_selected=int(r.n_selected[i]),
                             giou_fallback=bool(r.status[i] == 1), query_box=None if boxes[key] is None else boxes[key].copy())
        self._query_images.update(embeds)
        self.query_image_info.update(info)

    def detect_image_guided(self, images, query_images, query_boxes=None, threshold: float = 0.0, nms_threshold: float = 0.3,
                            target_sizes=None):
        """HF's one-shot detection end to end: ``image_guided_detection`` + ``post_process_image_guided_detection``.
        ``images``: list of HxWx3 uint8 arrays.  ``query_images``: ONE example (array or path) for all images, or a list with one
        per image (HF's pairing: image b with query b).  ``query_boxes``: None, one box or one per example (None entries allowed):
        the region of the example that is meant, (x0, y0, x1, y1) in pixels of the example.  ``target_sizes``: (height, width)
        per image the boxes are scaled to, default each image's own; an OWLv2 heuristic scales by max(height, width) on both
        axes, as its HF processor does.
        Returns one dict per image: ``{"scores": alphas float32 [k], "labels": None, "boxes": xyxy float32 [k,4], "patches": int64
        [k], "detections": Detections}`` -- the kept patches in patch order.  An image for which nothing is left (HF drops it
        from its list) has an empty entry.  An example from which no query can be formed raises ValueError naming its index.
        The query sets of ``reparameterize_object_list`` / ``install_queries`` are not touched: the queries go to slots the
        scorer's registry does not hold, a group at a time when there are more distinct examples than free slots, and the
        registry is what it was when the call returns.  RuntimeError when no slot is free: slots stay held until they are
        released -- after a lock-step group that filled all of them, ``scorer.release_slot(slot)`` for the slots no searcher uses
        any more frees them."""
        import torch
        images = [np.ascontiguousarray(im) for im in images]
        n = len(images)
        if n < 1:
            raise ValueError("detect_image_guided: no image")
        for b, im in enumerate(images):
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError(f"detect_image_guided: image {b} must be an HxWx3 uint8 RGB array")
        shared = not isinstance(query_images, (list, tuple))
        queries = [query_images] * n if shared else list(query_images)
        if len(queries) != n:
            raise ValueError("detect_image_guided: query_images must be one example, or one per image")
        if query_boxes is None:
            qboxes = [None] * n
        elif len(query_boxes) == 4 and all(q is not None and np.ndim(q) == 0 for q in query_boxes):
            qboxes = [query_boxes] * n                           # one box (four numbers) for every example
        else:
            qboxes = list(query_boxes)
            if len(qboxes) != n:
                raise ValueError("detect_image_guided: query_boxes must be one box, or one per example")
        if target_sizes is None:
            target_sizes = [im.shape[:2] for im in images]
        target_sizes = np.asarray(target_sizes)
        if target_sizes.shape != (n, 2):
            raise ValueError("detect_image_guided: target_sizes needs one (height, width) per image")
        # 1. the distinct (example, box) pairs, embedded once each
        distinct, arrays, boxes, of_image = {}, {}, {}, []
        for b, (q, qb) in enumerate(zip(queries, qboxes)):
            ident = (q if isinstance(q, (str, os.PathLike)) else id(q), None if qb is None else tuple(float(v) for v in np.ravel(qb)))
            if ident not in distinct:
                k = distinct[ident] = len(distinct)
                arrays[k] = self._load_example(q, f"detect_image_guided: query image {b}")
                boxes[k] = None if qb is None else self._relative_box(qb, arrays[k].shape[0], arrays[k].shape[1],
                                                                      f"detect_image_guided: query image {b}")
            of_image.append(distinct[ident])
        embeds = {}
        for k, (r, i) in self._embed_examples(arrays, boxes).items():
            if int(r.status[i]) == 2:
                b = of_image.index(k)
                raise ValueError(f"detect_image_guided: no query can be formed from query image {b}: none of its predicted boxes "
                                 "overlaps the " + ("whole image" if boxes[k] is None else "query box") +
                                 " (empty selection in HF's embed_image_query)")
            embeds[k] = r.embeds[i]
        # 2. - 4. a group of distinct queries at a time, in slots the registry does not hold
        sc = self.scorer
        from .owl import MAX_SETS
        free = [sl for sl in range(MAX_SETS - 1, -1, -1) if sl not in sc.Qs and sl not in sc._pending]
        if not free:
            raise RuntimeError(f"detect_image_guided: all {MAX_SETS} query-set slots hold installed query sets; none is free for a "
                               "one-shot query (scorer.release_slot(slot) frees one that is no longer used)")
        results = [None] * n
        ks = sorted(embeds)
        try:
            for g0 in range(0, len(ks), len(free)):
                slot_of = {k: free[j] for j, k in enumerate(ks[g0:g0 + len(free)])}
                for k, sl in slot_of.items():
                    sc.set_query_embeds(embeds[k][None, :], [1], [1.0], slot=sl)
                by_shape: Dict[tuple, List[int]] = {}
                for b in range(n):
                    if of_image[b] in slot_of:
                        by_shape.setdefault(images[b].shape, []).append(b)
                for idx in by_shape.values():
                    for c0 in range(0, len(idx), sc.max_batch):
                        chunk = idx[c0:c0 + sc.max_batch]
                        d_img = torch.from_numpy(np.stack([images[b] for b in chunk])).cuda()
                        r = sc.score(d_img, 1, 1, want_logits=True, image_sets=[slot_of[of_image[b]] for b in chunk])
                        post = sc.image_guided_postprocess(r.scores, r.boxes_cxcywh, threshold, nms_threshold, target_sizes[chunk])
                        alphas, xyxy, keep = post.alphas.cpu().numpy(), post.boxes.cpu().numpy(), post.keep.cpu().numpy()
                        for j, b in enumerate(chunk):
                            m = keep[j]
                            dets = Detections(xyxy=xyxy[j][m], confidence=alphas[j][m], class_id=np.zeros(int(m.sum()), dtype=np.int64))
                            results[b] = {"scores": dets.confidence, "labels": None, "boxes": dets.xyxy, "patches": np.nonzero(m)[0],
                                          "detections": dets}
        finally:
            # the registry as it was: these slots held nothing.  The handle keeps Q = 1 and the one-shot row in them; with the registry
            # entry gone (Qs.get(slot, 0) == 0) they are reachable neither through score(want_logits) nor get_query_embeds, and the
            # next install of the slot overwrites them
            for sl in free:
                sc.release_slot(sl)
        return results

    def clear_query_images(self):
        """Forget every example image: names are text queries again from the next install on."""
        self._query_images = {}
        self.query_image_info = {}

    def _image_overrides(self, texts):
        """{query row: embedding} of the rows of ``texts`` whose name has an example image (never the trailing blank query)."""
        if not self._query_images:
            return None
        return {i: self._query_images[t[0]] for i, t in enumerate(texts[:-1]) if t[0] in self._query_images} or None

    # ---- reference surface -------------------------------------------------------------
    def reparameterize_object_list(self, target_objects: List[str], cue_objects: List[str]):
        combined = list(target_objects) + list(cue_objects)
        self.texts = [[obj.strip()] for obj in combined] + [[' ']]
        ids, am = encode_queries(self.texts, self.model_name_or_path, allow_standin=self.allow_standin_tokenizer)
        self._ids, self._am = ids, am
        # default weights = the searcher's own defaults (target 1.0, cue 0.5, unknown 0.5;
        # interface_searcher.py:88-91,136); a searcher overrides them via set_class_weights
        w = [1.0] * len(target_objects) + [0.5] * len(cue_objects) + [0.5]
        # recorded now, run through the text tower when slot 0 is first used (OwlScorer.set_queries): a searcher's constructor
        # calls this like the reference's, but a lock-step group never scores against slot 0
        self.scorer.set_queries(ids, am, w, lazy=True, overrides=self._image_overrides(self.texts))
        self._class_weight = np.asarray(w, dtype=np.float64)

    def inference_detector(self, images, **kwargs) -> List[Detections]:
        import torch
        img = np.array(images[0], dtype=np.uint8, order="C")                  # only image 0, as the reference (own copy)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("inference_detector expects HxWx3 uint8 RGB images")
        d_img = torch.from_numpy(img).cuda().unsqueeze(0)
        r = self.scorer.score(d_img, 1, 1)
        dets = [self._detections_from(r, 0)]
        self.detections_inbatch = dets
        return dets

    def inference(self, image_path, use_amp: bool = False) -> Detections:
        """(:217-230) detector on an image FILE (decoded with Pillow, RGB) against the current ``texts``."""
        from PIL import Image
        with Image.open(image_path) as im:
            image = np.asarray(im.convert("RGB"), dtype=np.uint8)
        return self.inference_detector([image], use_amp=use_amp)[0]

    def bbox_visualization(self, images, detections_inbatch):
        out = []
        for image, det in zip(images, detections_inbatch):
            out.append(draw_boxes(image, det))
        return out

    # ---- fast-path extensions ----------------------------------------------------------
    def set_class_weights(self, object2weight: Dict[str, float]):
        """Install ``object2weight.get(name, 0.5)`` per query (interface_searcher.py:136)."""
        w = [float(object2weight.get(t[0], 0.5)) for t in self.texts]
        self.scorer.set_class_weights(w)
        self._class_weight = np.asarray(w, dtype=np.float64)

    aux_lane = True      # score_batch(..., lane=1) runs in a second workspace: safe to enqueue on another stream beside lane 0

    def score_batch(self, d_images, grid_rows: int, grid_cols: int, image_sets=None, lane: int = 0, boxes: bool = True):
        """Batched scoring of device images u8 [B,H,W,3] -> tstar_amd.owl.ScoreResult (device tensors).
        ``image_sets``: query-set slot per image (see ``install_queries``); default slot 0.  ``lane``: see ``OwlScorer.score``.
        ``boxes=False`` (1 x 1 grid only): the box head is skipped and the result's ``boxes`` is None -- for callers that read only
        ``cell_conf`` / ``cell_mask`` (the searcher's verification frames without a visual history); same bits in every other field.
        ``annotated_batch`` / ``_detections_from`` raise ``NO_BOXES_ERROR`` on such a result."""
        return self.scorer.score(d_images, grid_rows, grid_cols, image_sets=image_sets, lane=lane, boxes=boxes)

    # ---- frame records (feature cache) -------------------------------------------------
    def _cache(self):
        if self.feature_cache is None:
            raise RuntimeError("the feature cache is off: build the heuristic with feature_cache_frames=N (or TSTAR_FEATURE_CACHE=N)")
        return self.feature_cache

    @staticmethod
    def _gather_resized(frames, size):
        """[(store, second)] -> cuda u8 [n, height, width, 3]: the frames gathered from their stores and resized to ``size`` =
        (width, height) by the searcher's own kernel (tstar_frames_resize, as ``TStarSearcher._device_verify_frames``); one launch
        per run of frames of one store (at most ``store.lease_frames`` of them: a run is one lease), one index upload."""
        import torch
        ow, oh = int(size[0]), int(size[1])
        dev = frames[0][0].device
        out = torch.empty((len(frames), oh, ow, 3), dtype=torch.uint8, device=dev)
        d_idx = torch.as_tensor([int(sec) for _, sec in frames], dtype=torch.int32, device=dev)
        lib = _lib.load()
        i0 = 0
        while i0 < len(frames):
            store = frames[i0][0]
            i1 = i0
            while i1 < len(frames) and frames[i1][0] is store and i1 - i0 < (store.lease_frames or len(frames)):
                i1 += 1
            _, H, Wd, _ = store.shape
            lease = store.lease([int(sec) for _, sec in frames[i0:i1]], d_idx[i0:i1])
            _lib.check(lib.tstar_frames_resize(lease.frames.data_ptr(), lease.N, H, Wd, lease.idx.data_ptr(), i1 - i0, ow, oh,
                                               out[i0:i1].data_ptr(), int(store.fmt == "nv12"), _lib.stream_ptr()), "tstar_frames_resize")
            lease.done()
            i0 = i1
        return out

    def score_frames(self, store, secs, size=None, image_sets=None, boxes: bool = False):
        """``score_batch(frames, 1, 1, ...)`` of the frames ``secs`` of ``store`` resized to ``size`` = (width, height) (default: the
        searcher's verification size, 600 x 285) -- same ``ScoreResult``, same bits -- through the frame records: only frames
        without a record are gathered, resized and run through the vision tower (they leave their records behind); every frame
        is then scored from its record.  ``boxes=True``: also ``r.boxes`` (and all frames in ``r.frames``, gathered for the caller
        to paint).  ``r.cache_hit``: numpy bool per frame.  Needs the cache on (RuntimeError otherwise)."""
        return self.score_frames_of([(store, int(s)) for s in secs], size=size, image_sets=image_sets, boxes=boxes)

    def score_frames_of(self, frames, size=None, image_sets=None, boxes: bool = False, want_logits: bool = False):
        """``score_frames`` for frames of several stores: ``frames`` = [(store, second)] (a lock-step group's verification batch)."""
        import torch
        cache = self._cache()
        if size is None:
            from .interface_searcher import VERIFY_H, VERIFY_W
            size = (VERIFY_W, VERIFY_H)
        frames = list(frames)
        if not frames:
            raise ValueError("score_frames: no frame")
        keys = [cache.key(st, sec, size) for st, sec in frames]
        parts, pos = [], 0
        while pos < len(frames):
            # (one pass unless the pool is full and more than max_batch frames of the call have no record)
            plan = cache.plan(keys[pos:])
            part = frames[pos:pos + plan.n]
            try:
                d_all = self._gather_resized(part, size) if boxes else None
                d_miss = None
                if plan.miss_pos:
                    if d_all is not None:
                        d_miss = d_all if len(plan.miss_pos) == plan.n else d_all.index_select(
                            0, torch.as_tensor(plan.miss_pos, dtype=torch.long, device=d_all.device))
                    else:
                        d_miss = self._gather_resized([part[i] for i in plan.miss_pos], size)
                r = self.scorer.score_records(d_miss, plan.miss_slots, plan.slots, size,
                                              image_sets=None if image_sets is None else list(image_sets[pos:pos + plan.n]),
                                              want_logits=want_logits, boxes=boxes)
            except BaseException:
                cache.rollback(plan)
                raise
            r.frames = d_all
            r.cache_hit = np.asarray(plan.hit, dtype=bool)
            parts.append(r)
            pos += plan.n
        if len(parts) == 1:
            return parts[0]
        from .owl import ScoreResult
        cat = lambda name: None if getattr(parts[0], name) is None else torch.cat([getattr(p_, name) for p_ in parts])   # noqa: E731
        r = ScoreResult(**{name: cat(name) for name in ("scores", "labels", "boxes", "cell_conf", "cell_mask", "n_kept", "logits",
                                                        "boxes_cxcywh", "frames")})
        r.cache_hit = np.concatenate([p_.cache_hit for p_ in parts])
        return r

    def index_frames(self, store, secs=None, batch: Optional[int] = None, size=None) -> int:
        """Fill the records of the frames ``secs`` of ``store`` (default: every second) without scoring anything, ``batch`` frames
        per forward (default ``max_batch``): a question asked afterwards pays the grid forwards only.  Frames the pool has no
        room for are left out.  Returns the number of records written."""
        cache = self._cache()
        if size is None:
            from .interface_searcher import VERIFY_H, VERIFY_W
            size = (VERIFY_W, VERIFY_H)
        secs = list(range(store.num_seconds)) if secs is None else [int(s) for s in secs]
        batch = int(batch) if batch else self.scorer.max_batch
        written = 0
        for i0 in range(0, len(secs), batch):
            part = [(store, s) for s in secs[i0:i0 + batch]]
            plan = cache.plan([cache.key(st, sec, size) for st, sec in part], use_scratch=False)
            if not plan.miss_pos:
                continue
            try:
                self.scorer.score_records(self._gather_resized([part[i] for i in plan.miss_pos], size), plan.miss_slots, [], size)
            except BaseException:
                cache.rollback(plan)
                raise
            written += len(plan.miss_pos)
        return written

    def feature_cache_stats(self) -> dict:
        """``{"hits", "misses", "uncached", "slots", "used", "frame_bytes", "pool_bytes"}``; ``{"slots": 0}`` with the cache off."""
        if self.feature_cache is None:
            return {"hits": 0, "misses": 0, "uncached": 0, "slots": 0, "used": 0, "frame_bytes": self.scorer.records_frame_bytes(), "pool_bytes": 0}
        st = self.feature_cache.stats()
        fb = self.scorer.records_frame_bytes()
        st.update(frame_bytes=fb, pool_bytes=(fb + 15) // 16 * 16 * self.scorer.records_slots())
        return st

    def install_queries(self, slot: int, target_objects: List[str], cue_objects: List[str],
                        object2weight: Optional[Dict[str, float]] = None) -> List[List[str]]:
        """Install a question's queries in slot 1..63 WITHOUT touching ``self.texts`` (slot 0 is what
        ``reparameterize_object_list`` manages).  Several (video, question) items can then be scored in
        one batch, each image against its own slot.  Returns the texts list of the slot."""
        texts, (slot, ids, am, weights, overrides) = self._query_entry(slot, target_objects, cue_objects, object2weight)
        self.scorer.set_queries(ids, am, weights, slot=slot, overrides=overrides)
        return texts

    def _query_entry(self, slot, target_objects, cue_objects, object2weight):
        """(texts of the slot, (slot, token ids, attention mask, class weights, image rows)) of one question: blank query appended,
        targets weigh 1.0 and cues 0.5 unless ``object2weight`` says otherwise (interface_searcher.py:88-91, 135-137); image rows:
        ``_image_overrides``."""
        if not 1 <= int(slot) <= 63:
            raise ValueError("install_queries: slot must be in 1..63")
        texts = [[obj.strip()] for obj in list(target_objects) + list(cue_objects)] + [[' ']]
        ids, am = encode_queries(texts, self.model_name_or_path, allow_standin=self.allow_standin_tokenizer)
        o2w = dict(object2weight or {})
        for o in target_objects:
            o2w.setdefault(o, 1.0)
        for o in cue_objects:
            o2w.setdefault(o, 0.5)
        return texts, (int(slot), ids, am, [float(o2w.get(t[0], 0.5)) for t in texts], self._image_overrides(texts))

    def install_queries_many(self, items) -> List[List[List[str]]]:
        """``install_queries`` for several slots at once -- ``items``: [(slot, target_objects, cue_objects, object2weight)] -- with
        the text tower run ONCE over all their queries (a lock-step group installs the questions of its items together).
        Returns the texts list of every slot; identical to one ``install_queries`` call per item."""
        built = [self._query_entry(*it) for it in items]
        self.scorer.set_queries_many([e for _, e in built])
        return [t for t, _ in built]

    def annotated_batch(self, d_images, r, start: int = 0, count: Optional[int] = None):
        """Device form of ``bbox_visualization`` + ``Detections`` for images that are already on the device (the
        searcher's visual history): paints the kept boxes of ``r`` (images ``start .. start+count`` of a
        ``score_batch`` result) onto ``d_images`` u8 [count,H,W,3] IN PLACE, then brings images and detections to the
        host with one copy each.  Returns (images uint8 [count,H,W,3], [Detections] * count)."""
        count = int(d_images.shape[0]) if count is None else int(count)
        if not d_images.is_contiguous() or d_images.shape[0] != count:
            raise ValueError("annotated_batch: d_images must be a contiguous [count,H,W,3] uint8 device tensor")
        if r.boxes is None:
            raise ValueError("annotated_batch: " + NO_BOXES_ERROR)
        boxes = r.boxes[start:start + count].contiguous()
        scores = r.scores[start:start + count].contiguous()
        lib = _lib.load()
        _lib.check(lib.tstar_draw_boxes_np(d_images.data_ptr(), count, int(d_images.shape[1]), int(d_images.shape[2]),
                                           boxes.data_ptr(), scores.data_ptr(), int(boxes.shape[1]), _lib.stream_ptr()),
                   "tstar_draw_boxes_np")
        imgs = d_images.cpu().numpy()
        s, bx, lab = scores.cpu().numpy(), boxes.cpu().numpy(), r.labels[start:start + count].cpu().numpy()
        dets = []
        for k in range(count):
            keep = s[k] > np.float32(0.005)
            dets.append(Detections(xyxy=bx[k][keep], confidence=s[k][keep], class_id=lab[k][keep].astype(np.int64)))
        return imgs, dets

    def _detections_from(self, r, b: int) -> Detections:
        if r.boxes is None:
            raise ValueError("_detections_from: " + NO_BOXES_ERROR)
        s = r.scores[b].cpu().numpy()
        keep = s > np.float32(0.005)
        return Detections(xyxy=r.boxes[b].cpu().numpy()[keep], confidence=s[keep],
                          class_id=r.labels[b].cpu().numpy()[keep].astype(np.int64))


def _yolo_scale_from_config(config_path: Optional[str]) -> str:
    """'yolo_world_v2_xl_vlpan_...' -> 'xl' (the config the reference wires, TStarFramework.py:181: the yolov8_x base scaled
    "from X to XL", widen 1.5); BASELINE configs[3] names the L model, which is the default when the name says nothing."""
    import re
    m = re.search(r"yolo_world(?:_v2)?_(s|m|l|xl|x)_", os.path.basename(str(config_path or "")))
    return m.group(1) if m else "l"


class YoloWorldInterface(HeuristicInterface):
    def __init__(self, config_path: Optional[str] = None, checkpoint_path: Optional[str] = None, device: str = "cuda:0", *,
                 scale: Optional[str] = None, synthetic_seed: Optional[int] = None, state_dict: Optional[Dict] = None,
                 text_state_dict: Optional[Dict] = None, max_batch: int = 16):
        """Arguments as the reference (:40-47: ``config_path``, ``checkpoint_path``, ``device``).  The mmengine config is
        only consulted for the model scale (its file name); weights come from ``state_dict`` (mmyolo / YOLO-World names),
        else ``checkpoint_path`` if that file exists (a torch checkpoint with a ``state_dict`` entry), else -- only when
        ``synthetic_seed`` is not None -- seeded synthetic parameters (there is no network to fetch a checkpoint).
        The CLIP text tower (HuggingCLIPLanguageBackbone in the real model) is the HIP text tower shared with the
        OWL-ViT backend, fed from ``text_state_dict`` (HF OWL-ViT / CLIP text names) or the checkpoint's
        ``backbone.text_model`` entries or synthetic weights."""
        import torch
        from .owl import OwlScorer
        from .yolo import YoloDetector
        from . import yolo_world as YW
        if not str(device).startswith("cuda"):
            raise ValueError("tstar_amd.YoloWorldInterface runs on the GPU only (device='cuda[:i]'); it has no CPU path")
        self.config_path, self.checkpoint_path, self.device = config_path, checkpoint_path, device
        self.scale = scale or _yolo_scale_from_config(config_path)
        if state_dict is None and synthetic_seed is None and not (checkpoint_path and os.path.isfile(checkpoint_path)):
            raise FileNotFoundError(
                f"no YOLO-World checkpoint at {checkpoint_path!r} (offline); pass synthetic_seed=<int> for seeded synthetic "
                f"YOLO-World-v2-{self.scale.upper()} weights or state_dict=<mmyolo state dict>")
        dev = torch.device(device)
        if dev.index is not None:
            torch.cuda.set_device(dev.index)
        if state_dict is None and checkpoint_path and os.path.isfile(checkpoint_path):
            # tensors only: the mmengine checkpoint's meta / optimizer objects are never needed, so nothing is unpickled
            # beyond what torch's safe loader admits
            ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
            ck = ck.get("state_dict", ck)
            state_dict = {k: v.float().numpy() for k, v in ck.items() if hasattr(v, "numpy")}
            self.weights_source = checkpoint_path
        elif state_dict is not None:
            self.weights_source = "state_dict"
        else:
            state_dict = YW.synthetic_state_dict(int(synthetic_seed), self.scale)
            self.weights_source = f"synthetic(seed={int(synthetic_seed)})"
        if text_state_dict is None:
            pre = "backbone.text_model.model."
            clip = {k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}
            if clip:          # HF CLIPTextModelWithProjection names -> the OWL-ViT text tower's names
                text_state_dict = {("owlvit." + k) if not k.startswith("text_projection") else "owlvit." + k: np.asarray(v, np.float32)
                                   for k, v in clip.items()}
                pos = "owlvit.text_model.embeddings.position_embedding.weight"
                if pos in text_state_dict:
                    text_state_dict[pos] = text_state_dict[pos][:W.T_LEN]          # 77 CLIP positions, queries use <= 16
            elif self.weights_source.startswith("synthetic("):
                text_state_dict = W.synthetic_state_dict(int(synthetic_seed), "text")
            else:
                raise FileNotFoundError("the YOLO-World state dict carries no CLIP text tower; pass text_state_dict=")
        self.allow_standin_tokenizer = self.weights_source.startswith("synthetic(")
        self.detector = YoloDetector(state_dict, self.scale, max_batch=max_batch)
        self.text_tower = OwlScorer(None, W.pack_blob(text_state_dict, W.text_spec()), max_batch=1)
        self.model_name_or_path = "openai/clip-vit-base-patch32"
        self.texts = []
        self.detections_inbatch: List[Detections] = []
        self._text_feats = None
        self._pending0 = None
        self.set_BBoxAnnotator()

    def set_BBoxAnnotator(self):
        """(:68-76) the reference builds supervision annotators; boxes are painted by ``draw_boxes`` here."""
        self.BOUNDING_BOX_ANNOTATOR = draw_boxes
        self.LABEL_ANNOTATOR = None

    # ---- reference surface -------------------------------------------------------------
    def _encode(self, texts, weights, slot):
        ids, am = encode_queries(texts, self.model_name_or_path, allow_standin=self.allow_standin_tokenizer)
        self.text_tower.set_queries(ids, am, weights, slot=0)
        feats = self.text_tower.get_query_embeds(0)              # text_embeds / ||text_embeds|| (the backbone's forward_text)
        self.detector.set_text_feats(feats, weights, slot=slot)
        return feats

    def reparameterize_object_list(self, target_objects: List[str], cue_objects: List[str]):
        """(:78-93) texts = [[name.strip()], ..., [' ']]; ``model.reparameterize(texts)`` caches the text features."""
        combined = list(target_objects) + list(cue_objects)
        self.texts = [[obj.strip()] for obj in combined] + [[' ']]
        w = [1.0] * len(target_objects) + [0.5] * len(cue_objects) + [0.5]
        # tokenised now (a missing vocabulary must be reported here), run through the CLIP text tower when slot 0 is first used
        ids, am = encode_queries(self.texts, self.model_name_or_path, allow_standin=self.allow_standin_tokenizer)
        self._pending0 = (ids, am, list(w))
        self._text_feats = None
        self._class_weight = np.asarray(w, dtype=np.float64)

    def set_query_images(self, images):
        """Image-guided queries are OWL-ViT / OWLv2's (``OWLInterface.set_query_images``): YOLO-World has no counterpart."""
        raise NotImplementedError("YoloWorldInterface has no image-guided queries: YOLO-World matches text features only; use the "
                                  "OWL-ViT / OWLv2 heuristic (heuristic_type='owl-vit') for example images")

    def _flush0(self):
        """Install the recorded queries of slot 0 (see ``reparameterize_object_list``)."""
        p = getattr(self, "_pending0", None)
        if p is not None:
            self._pending0 = None
            self.text_tower.set_queries(p[0], p[1], p[2], slot=0)
            self._text_feats = self.text_tower.get_query_embeds(0)
            self.detector.set_text_feats(self._text_feats, p[2], slot=0)

    def inference_detector(self, images, max_dets: int = 50, score_threshold: float = 0.12, use_amp: bool = False) -> List[Detections]:
        """(:136-168) only ``images[0]``; detections with score > ``score_threshold``, the ``max_dets`` best, descending."""
        import torch
        img = np.array(images[0], dtype=np.uint8, order="C")
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("inference_detector expects HxWx3 uint8 RGB images")
        self._flush0()
        r = self.detector.detect(torch.from_numpy(img).cuda().unsqueeze(0), 1, 1, score_threshold=score_threshold, max_dets=max_dets,
                                 want_cells=False)
        dets = [self._detections_from(r, 0)]
        self.detect_outputs_raw = r
        self.detections_inbatch = dets
        return dets

    def inference(self, image, max_dets: int = 100, score_threshold: float = 0.3, use_amp: bool = False) -> Detections:
        """(:96-134) detector on an image FILE.  mmdet's LoadImageFromFile hands BGR to the pipeline, whose preprocessor
        swaps to RGB; ``inference_detector`` receives RGB and (as in the reference) lets the same swap happen, so the file
        is decoded to BGR order here to end up with the channel order the model was trained on."""
        from PIL import Image
        with Image.open(image) as im:
            rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
        return self.inference_detector([np.ascontiguousarray(rgb[:, :, ::-1])], max_dets=max_dets, score_threshold=score_threshold)[0]

    def bbox_visualization(self, images, detections_inbatch):
        """(:170-190) annotated COPIES; like the reference, every entry annotates ``images[len(detections_inbatch) - 1]``."""
        out = []
        for detections in detections_inbatch:
            image = images[len(detections_inbatch) - 1]
            out.append(draw_boxes(image.copy(), detections))
        return out

    # ---- fast-path extensions (same contract as OWLInterface) -----------------------------
    def set_class_weights(self, object2weight: Dict[str, float]):
        w = [float(object2weight.get(t[0], 0.5)) for t in self.texts]
        if getattr(self, "_pending0", None) is not None:      # slot 0 not installed yet: the weights ride along
            self._pending0 = (self._pending0[0], self._pending0[1], w)
        else:
            self.detector.set_class_weights(w)
        self._class_weight = np.asarray(w, dtype=np.float64)

    def score_batch(self, d_images, grid_rows: int, grid_cols: int, image_sets=None):
        if getattr(self, "_pending0", None) is not None and (image_sets is None or 0 in [int(v) for v in image_sets]):
            self._flush0()
        return self.detector.detect(d_images, grid_rows, grid_cols, score_threshold=0.12, max_dets=50, image_sets=image_sets)

    def install_queries(self, slot: int, target_objects: List[str], cue_objects: List[str],
                        object2weight: Optional[Dict[str, float]] = None) -> List[List[str]]:
        if not 1 <= int(slot) <= 63:
            raise ValueError("install_queries: slot must be in 1..63")
        texts = [[obj.strip()] for obj in list(target_objects) + list(cue_objects)] + [[' ']]
        o2w = dict(object2weight or {})
        for o in target_objects:
            o2w.setdefault(o, 1.0)
        for o in cue_objects:
            o2w.setdefault(o, 0.5)
        self._encode(texts, [float(o2w.get(t[0], 0.5)) for t in texts], int(slot))
        return texts

    def install_queries_many(self, items) -> List[List[List[str]]]:
        """``install_queries`` for several slots with ONE run of the CLIP text tower over all their queries (the text tower keeps
        the same slot numbers; each slot's normalised text features then go to the detector's guide layers)."""
        out, entries, weights = [], [], []
        for slot, target_objects, cue_objects, object2weight in items:
            if not 1 <= int(slot) <= 63:
                raise ValueError("install_queries: slot must be in 1..63")
            texts = [[obj.strip()] for obj in list(target_objects) + list(cue_objects)] + [[' ']]
            o2w = dict(object2weight or {})
            for o in target_objects:
                o2w.setdefault(o, 1.0)
            for o in cue_objects:
                o2w.setdefault(o, 0.5)
            w = [float(o2w.get(t[0], 0.5)) for t in texts]
            ids, am = encode_queries(texts, self.model_name_or_path, allow_standin=self.allow_standin_tokenizer)
            entries.append((int(slot), ids, am, w))
            weights.append(w)
            out.append(texts)
        self.text_tower.set_queries_many(entries)
        for (slot, _, _, _), w in zip(entries, weights):
            self.detector.set_text_feats(self.text_tower.get_query_embeds(slot), w, slot=slot)
        return out

    def annotated_batch(self, d_images, r, start: int = 0, count: Optional[int] = None):
        """Images + detections of a ``score_batch`` result on the host, boxes painted (<= 50 per image: host painter)."""
        count = int(d_images.shape[0]) if count is None else int(count)
        imgs = d_images.cpu().numpy()
        dets = [self._detections_from(r, start + k) for k in range(count)]
        for k in range(count):
            draw_boxes(imgs[k], dets[k])
        return imgs, dets

    def _detections_from(self, r, b: int) -> Detections:
        n = int(r.n_kept[b].item())
        return Detections(xyxy=r.boxes[b, :n].cpu().numpy(), confidence=r.scores[b, :n].cpu().numpy(),
                          class_id=r.labels[b, :n].cpu().numpy().astype(np.int64))


def draw_boxes(image: np.ndarray, det: Detections, color=(255, 64, 64)) -> np.ndarray:
    """1-px rectangles painted IN PLACE on ``image`` (the reference's supervision BoxAnnotator also
    paints on the array it is given, Appendix B.14) and returned."""
    H, Wd = image.shape[:2]
    b = np.asarray(det.xyxy, dtype=np.float64).reshape(-1, 4)
    # round half to even (Python round / np.rint / the device painter's rint), clamp to the image
    xs = np.clip(np.rint(b[:, [0, 2]]), 0, Wd - 1).astype(np.int64)
    ys = np.clip(np.rint(b[:, [1, 3]]), 0, H - 1).astype(np.int64)
    for (xa, xb), (ya, yb) in zip(xs.tolist(), ys.tolist()):
        if xb < xa or yb < ya:
            continue
        image[ya, xa:xb + 1] = color
        image[yb, xa:xb + 1] = color
        image[ya:yb + 1, xa] = color
        image[ya:yb + 1, xb] = color
    return image


def initialize_heuristic(heuristic_type: str = "owl-vit", **kwargs) -> HeuristicInterface:
    """Factory with the reference's signature (TStarFramework.py:171-187).  ``model_name_or_path=`` overrides the OWL-ViT
    checkpoint (default ``google/owlvit-base-patch32``; B/16 and OWLv2 B/16 checkpoints are supported too); ``input_size=(height, width)``
    overrides the detector's input size (default the checkpoint's 768 x 768; ``TSTAR_INPUT_SIZE=HxW`` when not given)."""
    if heuristic_type == "owl-vit":
        kwargs.setdefault("model_name_or_path", "google/owlvit-base-patch32")
        return OWLInterface(**kwargs)
    if heuristic_type == "yolo-World":
        # the paths the reference hard-codes (TStarFramework.py:181-182); the checkpoint is used when it exists
        config_path = "./YOLO-World/configs/pretrain/yolo_world_v2_xl_vlpan_bn_2e-3_100e_4x8gpus_obj365v1_goldg_train_lvis_minival.py"
        checkpoint_path = "./pretrained/YOLO-World/yolo_world_v2_xl_obj365v1_goldg_cc3mlite_pretrain-5daf1395.pth"
        kwargs.setdefault("config_path", config_path)
        kwargs.setdefault("checkpoint_path", checkpoint_path)
        return YoloWorldInterface(**kwargs)
    raise NotImplementedError(f"Heuristic type '{heuristic_type}' is not implemented.")
