"""OWL-ViT-B/32 and B/16, and OWLv2-B/16, parameter sets for the HIP scorer.

The reference loads ``google/owlvit-base-patch32`` (or whatever checkpoint it is
given) through HF transformers (/root/reference/TStar/interface_heuristic.py:207-210,
TStarFramework.py:176).  The HIP library takes ONE flat little-endian float32 blob
whose layout is fixed by ``vision_spec()`` / ``text_spec()`` below (mirrored entry
by entry in ``tstar_amd/csrc/owl_weights.h``).  This module

* builds that blob from a HF-style ``state_dict`` (names as in
  ``transformers/models/owlvit/modeling_owlvit.py``), either real weights found
  on disk (safetensors) or
* seeded synthetic weights: ``numpy.random.RandomState`` (frozen legacy stream,
  so CPU oracle, tests and the GPU box regenerate identical parameters) with
  the HF initialiser std's (modeling_owlvit.py ``_init_weights``; drawn from a
  unit-variance uniform instead of a normal, which keeps the std), small
  non-zero biases / LayerNorm perturbations so every parameter is exercised,
  and class-head shift/scale scaled by 0.01 so scores do not saturate
  (SURVEY.md 8c caveat (c)).

Two OWL-ViT vision geometries are supported (``OwlGeometry``): B/32 (the default
everywhere; the module-level constants below are its numbers) and B/16.  They
share every width; only the patch grid, and with it the token count, the
patch-embedding matrix, the position table and ``box_bias``, differ.  OWLv2 B/16
(``OWLV2_B16``: image 960, patch 16) is a third geometry of the other FAMILY: the
same widths, keys prefixed ``owlv2.`` and an ``objectness_head`` after the box head.

No torch import at module import time; numpy only.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

# ---- architecture constants (configuration_owlvit.py defaults = base-patch32) ----
V_D = 768          # vision hidden
V_FF = 3072
V_LAYERS = 12
V_HEADS = 12
IMG = 768
PATCH = 32
GRID = IMG // PATCH            # 24
NPATCH = GRID * GRID           # 576
NTOK = NPATCH + 1              # 577
T_D = 512          # text hidden
T_FF = 2048
T_LAYERS = 12
T_HEADS = 8
T_LEN = 16
VOCAB = 49408
PROJ = 512
LN_EPS = 1e-5

Spec = List[Tuple[str, Tuple[int, ...], Tuple[str, ...]]]


@dataclass(frozen=True)
class OwlGeometry:
    """Patch geometry of an OWL-ViT vision tower.  Every supported checkpoint shares the widths above (vision 768 / 3072,
    12 layers, 12 heads; the same text tower; projection 512): only the patch grid differs."""
    image_size: int
    patch_size: int
    # the input size of the RUN in pixels (height, width): a property of the detector handle, not of the checkpoint.  0 = the
    # checkpoint's own image_size, so OwlGeometry(768, 32) == OwlGeometry(768, 32, 768, 768) == B32.  See with_input_size().
    input_h: int = 0
    input_w: int = 0
    # the model family: "owlvit" (keys ``owlvit.*``, Pillow bicubic pre-processing, boxes scaled by (W, H)) or "owlv2" (keys
    # ``owlv2.*``, an objectness head, pad-to-square + float resize, boxes scaled by max(H, W))
    family: str = "owlvit"

    def __post_init__(self):
        if not self.input_h:
            object.__setattr__(self, "input_h", self.image_size)
        if not self.input_w:
            object.__setattr__(self, "input_w", self.image_size)

    @property
    def grid(self) -> int:
        """Side of the CHECKPOINT's square patch grid (what its position table was trained on)."""
        return self.image_size // self.patch_size

    @property
    def gh(self) -> int:
        return self.input_h // self.patch_size

    @property
    def gw(self) -> int:
        return self.input_w // self.patch_size

    @property
    def input_size(self) -> Tuple[int, int]:
        return (self.input_h, self.input_w)

    @property
    def checkpoint(self) -> "OwlGeometry":
        """The same checkpoint at its own input size."""
        return OwlGeometry(self.image_size, self.patch_size, family=self.family)

    @property
    def prefix(self) -> str:
        """Prefix of the towers' HF state-dict keys."""
        return self.family + "."

    @property
    def npatch(self) -> int:
        return self.gh * self.gw

    @property
    def ntok(self) -> int:
        return self.npatch + 1

    @property
    def patch_k(self) -> int:
        return 3 * self.patch_size * self.patch_size

    @property
    def name(self) -> str:
        return f"B/{self.patch_size}" if self.family == "owlvit" else f"OWLv2 B/{self.patch_size}"


B32 = OwlGeometry(768, 32)     # google/owlvit-base-patch32: grid 24, 576 patches, T = 577 (the default everywhere)
B16 = OwlGeometry(768, 16)     # google/owlvit-base-patch16: grid 48, 2304 patches, T = 2305
OWLV2_B16 = OwlGeometry(960, 16, family="owlv2")   # google/owlv2-base-patch16(-ensemble, -finetuned): grid 60, 3600 patches, T = 3601
SUPPORTED = (B32, B16)                             # the OWL-ViT geometries (what ``patch_size=`` chooses between)
FAMILIES = ("owlvit", "owlv2")
SUPPORTED_TEXT = ("OWL-ViT B/32 and B/16 (image 768, patch 32 or 16; vision 768 wide, MLP 3072, 12 layers, 12 heads; "
                  "text 512 wide, MLP 2048, 12 layers, 8 heads; projection 512), and OWLv2 B/16 (image 960, patch 16, the same "
                  "widths, plus the objectness head)")


MAX_NPATCH = 3600              # patches per image a run may ask for (T = 3601)
INPUT_SIZE_RULE = (f"each side of the input size must be a positive multiple of the patch size, and the patch grid may hold at most "
                   f"{MAX_NPATCH} patches")


def with_input_size(geometry: OwlGeometry, input_size=None) -> OwlGeometry:
    """``geometry`` run at ``input_size`` = (height, width) pixels; None keeps the checkpoint's own size.  ValueError, naming
    the rule, for a size the detector does not run at -- before anything touches the device."""
    g = geometry.checkpoint
    if input_size is None:
        return g
    try:
        h, w = input_size
        ok = int(h) == h and int(w) == w
        h, w = int(h), int(w)
    except (TypeError, ValueError):
        raise ValueError(f"input_size must be (height, width), not {input_size!r}") from None
    P = g.patch_size
    if not ok or h <= 0 or w <= 0 or h % P or w % P or (h // P) * (w // P) > MAX_NPATCH:
        raise ValueError(f"input_size {input_size!r} is not supported at patch {P}: {INPUT_SIZE_RULE}")
    return OwlGeometry(g.image_size, P, h, w, g.family)


def input_size_from_env(name: str = "TSTAR_INPUT_SIZE"):
    """(height, width) from ``TSTAR_INPUT_SIZE=HxW`` (e.g. ``448x768``), or None when it is unset / empty."""
    v = os.environ.get(name)
    if v is None or v.strip() == "":
        return None
    parts = v.strip().lower().split("x")
    if len(parts) != 2 or not all(p.strip().isdigit() for p in parts):
        raise ValueError(f"{name} must look like HEIGHTxWIDTH (e.g. 448x768), not {v!r}")
    return int(parts[0]), int(parts[1])


def resolve_input_size(input_size=None):
    """The ``input_size`` keyword if it was given, else ``TSTAR_INPUT_SIZE``, else None: the environment is read only when the
    keyword is absent, like the other deployment settings of ``OWLInterface``."""
    return input_size if input_size is not None else input_size_from_env()


def geometry_for_patch(patch_size: int) -> OwlGeometry:
    """The supported geometry with this patch size (image 768); ValueError otherwise."""
    for g in SUPPORTED:
        if g.patch_size == patch_size:
            return g
    raise ValueError(f"patch_size {patch_size!r} is not supported; supported: {SUPPORTED_TEXT}")


def geometry_for_family(family: str = "owlvit", patch_size: Optional[int] = None) -> OwlGeometry:
    """The checkpoint geometry of ``family`` ("owlvit": B/32, or B/16 with ``patch_size=16``; "owlv2": B/16 at image 960);
    ValueError for an unknown family or a patch size the family does not have."""
    if family == "owlvit":
        return geometry_for_patch(32 if patch_size is None else patch_size)
    if family == "owlv2":
        if patch_size is not None and int(patch_size) != OWLV2_B16.patch_size:
            raise ValueError(f"patch_size {patch_size!r} is not supported for owlv2; supported: {SUPPORTED_TEXT}")
        return OWLV2_B16
    raise ValueError(f"family {family!r} is not supported (one of {FAMILIES}); supported: {SUPPORTED_TEXT}")


def _layer_spec(prefix: str, d: int, ff: int) -> Spec:
    p = prefix
    return [
        (p + "ln1_w", (d,), (p + "layer_norm1.weight",)),
        (p + "ln1_b", (d,), (p + "layer_norm1.bias",)),
        (p + "qkv_w", (3 * d, d), (p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight")),
        (p + "qkv_b", (3 * d,), (p + "self_attn.q_proj.bias", p + "self_attn.k_proj.bias", p + "self_attn.v_proj.bias")),
        (p + "out_w", (d, d), (p + "self_attn.out_proj.weight",)),
        (p + "out_b", (d,), (p + "self_attn.out_proj.bias",)),
        (p + "ln2_w", (d,), (p + "layer_norm2.weight",)),
        (p + "ln2_b", (d,), (p + "layer_norm2.bias",)),
        (p + "fc1_w", (ff, d), (p + "mlp.fc1.weight",)),
        (p + "fc1_b", (ff,), (p + "mlp.fc1.bias",)),
        (p + "fc2_w", (d, ff), (p + "mlp.fc2.weight",)),
        (p + "fc2_b", (d,), (p + "mlp.fc2.bias",)),
    ]


def vision_spec(geometry: OwlGeometry = B32) -> Spec:
    """(blob entry name, shape, HF state_dict names concatenated along dim 0)."""
    g = geometry
    vm = g.prefix + "vision_model."
    s: Spec = [
        ("patch_w", (V_D, g.patch_k), (vm + "embeddings.patch_embedding.weight",)),
        ("class_emb", (V_D,), (vm + "embeddings.class_embedding",)),
        ("pos_emb", (g.ntok, V_D), (vm + "embeddings.position_embedding.weight",)),
        ("pre_ln_w", (V_D,), (vm + "pre_layernorm.weight",)),
        ("pre_ln_b", (V_D,), (vm + "pre_layernorm.bias",)),
    ]
    for i in range(V_LAYERS):
        s += _layer_spec(f"{vm}encoder.layers.{i}.", V_D, V_FF)
    s += [
        ("post_ln_w", (V_D,), (vm + "post_layernorm.weight",)),
        ("post_ln_b", (V_D,), (vm + "post_layernorm.bias",)),
        ("det_ln_w", (V_D,), ("layer_norm.weight",)),
        ("det_ln_b", (V_D,), ("layer_norm.bias",)),
        ("cls_w", (PROJ, V_D), ("class_head.dense0.weight",)),
        ("cls_b", (PROJ,), ("class_head.dense0.bias",)),
        ("shift_w", (V_D,), ("class_head.logit_shift.weight",)),
        ("shift_b", (1,), ("class_head.logit_shift.bias",)),
        ("scale_w", (V_D,), ("class_head.logit_scale.weight",)),
        ("scale_b", (1,), ("class_head.logit_scale.bias",)),
        ("box0_w", (V_D, V_D), ("box_head.dense0.weight",)),
        ("box0_b", (V_D,), ("box_head.dense0.bias",)),
        ("box1_w", (V_D, V_D), ("box_head.dense1.weight",)),
        ("box1_b", (V_D,), ("box_head.dense1.bias",)),
        ("box2_w", (4, V_D), ("box_head.dense2.weight",)),
        ("box2_b", (4,), ("box_head.dense2.bias",)),
        ("box_bias", (g.npatch, 4), ("box_bias",)),
    ]
    if g.family == "owlv2":                 # Owlv2ForObjectDetection.objectness_head: a box-head-shaped MLP with one output
        s += [
            ("obj0_w", (V_D, V_D), ("objectness_head.dense0.weight",)),
            ("obj0_b", (V_D,), ("objectness_head.dense0.bias",)),
            ("obj1_w", (V_D, V_D), ("objectness_head.dense1.weight",)),
            ("obj1_b", (V_D,), ("objectness_head.dense1.bias",)),
            ("obj2_w", (1, V_D), ("objectness_head.dense2.weight",)),
            ("obj2_b", (1,), ("objectness_head.dense2.bias",)),
        ]
    return s


def text_spec(geometry: OwlGeometry = B32) -> Spec:
    """The text tower's entries; only the key prefix depends on the geometry (its family)."""
    tm = geometry.prefix + "text_model."
    s: Spec = [
        ("tok_emb", (VOCAB, T_D), (tm + "embeddings.token_embedding.weight",)),
        ("tpos_emb", (T_LEN, T_D), (tm + "embeddings.position_embedding.weight",)),
    ]
    for i in range(T_LAYERS):
        s += _layer_spec(f"{tm}encoder.layers.{i}.", T_D, T_FF)
    s += [
        ("final_ln_w", (T_D,), (tm + "final_layer_norm.weight",)),
        ("final_ln_b", (T_D,), (tm + "final_layer_norm.bias",)),
        ("text_proj", (PROJ, T_D), (geometry.prefix + "text_projection.weight",)),
    ]
    return s


def spec_size(spec: Spec) -> int:
    return int(sum(int(np.prod(shape)) for _, shape, _ in spec))


def compute_box_bias(geometry: OwlGeometry = B32) -> np.ndarray:
    """box_bias buffer, restated from modeling_owlvit.py:1072-1104 (``compute_box_bias(gh, gw)``).

    xy = ((col+1)/gw, (row+1)/gh); bias = log(v+1e-4) - log1p(-v+1e-4); size
    entries use v = (1/gw, 1/gh); gh x gw = the run's patch grid (24 x 24 at B/32,
    48 x 48 at B/16, 14 x 24 at B/32 run on 448 x 768).  Row-major over the patch
    grid.  Uses torch float32 ops (as HF does) so the buffer is bit-identical to
    the one HF builds; torch is imported lazily.
    """
    import torch
    gh, gw = geometry.gh, geometry.gw
    xs = torch.arange(1, gw + 1, dtype=torch.float32)
    ys = torch.arange(1, gh + 1, dtype=torch.float32)
    xx, yy = torch.meshgrid(xs, ys, indexing="xy")
    coords = torch.stack((xx, yy), dim=-1)
    coords[..., 0] /= gw
    coords[..., 1] /= gh
    coords = torch.clip(coords.view(-1, 2), 0.0, 1.0)
    cb = torch.log(coords + 1e-4) - torch.log1p(-coords + 1e-4)
    size = torch.full_like(cb, 1.0)
    size[..., 0] /= gw
    size[..., 1] /= gh
    sb = torch.log(size + 1e-4) - torch.log1p(-size + 1e-4)
    return torch.cat([cb, sb], dim=-1).numpy().astype(np.float32)


def interpolate_pos_emb(pos_emb: np.ndarray, geometry: OwlGeometry) -> np.ndarray:
    """The checkpoint's position table [G*G + 1, 768] as the run's [gh*gw + 1, 768], with the statements of HF's
    ``OwlViTVisionEmbeddings.interpolate_pos_encoding``: row 0 (CLS) kept, the G x G patch rows resampled to gh x gw with
    ``torch.nn.functional.interpolate(mode="bicubic", align_corners=False)`` on the CPU.  At gh = gw = G the table is
    returned unchanged, as HF does.  torch is imported lazily."""
    g = geometry
    G = g.grid
    pos = np.ascontiguousarray(pos_emb, dtype=np.float32).reshape(G * G + 1, V_D)
    if g.gh == G and g.gw == G:
        return pos
    import torch
    t = torch.from_numpy(pos).unsqueeze(0)
    cls, patch = t[:, :1], t[:, 1:]
    patch = patch.reshape(1, G, G, V_D).permute(0, 3, 1, 2)
    patch = torch.nn.functional.interpolate(patch, size=(g.gh, g.gw), mode="bicubic", align_corners=False)
    patch = patch.permute(0, 2, 3, 1).reshape(1, -1, V_D)
    return np.ascontiguousarray(torch.cat((cls, patch), dim=1)[0].numpy(), dtype=np.float32)


def _std_for(name: str, shape: Tuple[int, ...]) -> float:
    """HF ``_init_weights`` std per parameter (modeling_owlvit.py:532-565)."""
    vision = "vision_model" in name
    d = V_D if vision else T_D
    layers = V_LAYERS if vision else T_LAYERS
    if name.endswith("class_embedding"):
        return d ** -0.5
    if "embedding" in name:
        return 0.02
    if any(k in name for k in ("q_proj.weight", "k_proj.weight", "v_proj.weight")):
        return (d ** -0.5) * ((2 * layers) ** -0.5)
    if "out_proj.weight" in name:
        return d ** -0.5
    if "fc1.weight" in name:
        return (2 * d) ** -0.5
    if "fc2.weight" in name:
        return (d ** -0.5) * ((2 * layers) ** -0.5)
    if "text_projection" in name:
        return T_D ** -0.5
    if name.startswith("class_head") or name.startswith("box_head") or name.startswith("objectness_head"):
        return 0.02
    return 0.02


def synthetic_state_dict(seed: int = 0, towers: str = "both", geometry: OwlGeometry = B32) -> Dict[str, np.ndarray]:
    """Seeded synthetic OWL-ViT parameters (B/32 unless ``geometry`` says otherwise) keyed by HF state_dict names.

    Drawn from ONE ``RandomState(seed)`` stream in spec order (vision first),
    so the text tower does not depend on whether the vision tower was built:
    each tower uses its own stream (seed, seed + 1).
    """
    out: Dict[str, np.ndarray] = {}

    def fill(spec: Spec, rs: np.random.RandomState) -> None:
        for _, _, hf_names in spec:
            for hf in hf_names:
                shape = _hf_shape(hf, geometry)
                n = int(np.prod(shape))
                if hf == "box_bias":
                    out[hf] = compute_box_bias(geometry)
                    continue
                # unit-variance uniform: (u - 0.5) * sqrt(12); the legacy
                # random_sample stream is frozen and ~30x faster than gauss
                x = ((rs.random_sample(n) - 0.5) * 3.4641016151377544).astype(np.float32).reshape(shape)
                if hf.endswith(".weight") and "norm" in hf.split(".")[-2]:
                    x = (1.0 + 0.1 * x).astype(np.float32)
                elif hf.endswith(".bias"):
                    x = (0.02 * x).astype(np.float32)
                else:
                    x = (np.float32(_std_for(hf, shape)) * x).astype(np.float32)
                if hf.startswith("class_head.logit_shift") or hf.startswith("class_head.logit_scale"):
                    x = (x * np.float32(0.01)).astype(np.float32)
                out[hf] = x

    geometry = geometry.checkpoint
    if towers in ("both", "vision"):
        fill(vision_spec(geometry), np.random.RandomState(seed))
    if towers in ("both", "text"):
        fill(text_spec(geometry), np.random.RandomState(seed + 1))
    return out


_HF_SHAPES: Dict[OwlGeometry, Dict[str, Tuple[int, ...]]] = {}


def _hf_shape(hf: str, geometry: OwlGeometry = B32) -> Tuple[int, ...]:
    geometry = geometry.checkpoint                  # a state dict holds the checkpoint's tables, whatever size it is run at
    shapes = _HF_SHAPES.get(geometry)
    if shapes is None:
        shapes = _HF_SHAPES[geometry] = {}
        for spec in (vision_spec(geometry), text_spec(geometry)):
            for _, shape, hf_names in spec:
                k = len(hf_names)
                for h in hf_names:
                    if h.endswith("patch_embedding.weight"):
                        shapes[h] = (V_D, 3, geometry.patch_size, geometry.patch_size)
                    elif h.startswith("class_head.logit_s") and h.endswith("weight"):
                        shapes[h] = (1, V_D)
                    elif k > 1:
                        shapes[h] = (shape[0] // k,) + tuple(shape[1:])
                    else:
                        shapes[h] = tuple(shape)
    return shapes[hf]


def to_bf16_values(a: np.ndarray) -> np.ndarray:
    """Round float32 values to the nearest bfloat16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(a.shape)


def round_weights_to_bf16(sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """BASELINE config 5 ("bf16 ViT weights"): every matrix / embedding table is rounded to bf16;
    biases, LayerNorm parameters and the box_bias buffer stay float32."""
    out = {}
    for k, v in sd.items():
        v = np.asarray(v, dtype=np.float32)
        out[k] = to_bf16_values(v) if (v.ndim >= 2 and k != "box_bias") else v
    return out


def pack_blob(sd: Dict[str, np.ndarray], spec: Spec, geometry: Optional[OwlGeometry] = None) -> np.ndarray:
    """Concatenate ``sd`` entries into the flat f32 blob the C ABI expects.  ``box_bias`` is a non-persistent buffer in
    transformers 5.x (not in the state dict): when it is missing it is computed for the spec's patch grid.

    ``geometry`` (with ``spec = vision_spec(geometry)``): a run at another input size than the checkpoint's.  ``pos_emb`` is
    then the checkpoint's table resampled to the run's grid (``interpolate_pos_emb``) and ``box_bias`` is computed for that
    grid (``compute_box_bias``), whatever the state dict holds: both are HF's own values under
    ``interpolate_pos_encoding=True``, bit for bit."""
    parts = []
    resized = geometry is not None and geometry != geometry.checkpoint
    for name, shape, hf_names in spec:
        if resized and name == "pos_emb":
            arr = interpolate_pos_emb(np.asarray(sd[hf_names[0]], dtype=np.float32), geometry)
        elif resized and name == "box_bias":
            arr = compute_box_bias(geometry)
        elif name == "box_bias" and "box_bias" not in sd:
            g = geometry.checkpoint if geometry is not None else next((g for g in SUPPORTED + (OWLV2_B16,) if g.npatch == shape[0]), None)
            if g is None:
                raise ValueError(f"weight box_bias: no supported geometry has {shape[0]} patches")
            arr = compute_box_bias(g)
        else:
            arr = np.concatenate([np.asarray(sd[h], dtype=np.float32).reshape(-1) for h in hf_names])
        if arr.size != int(np.prod(shape)):
            raise ValueError(f"weight {name}: expected {shape}, got {arr.size} elements")
        parts.append(arr.reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def unpack_blob(blob: np.ndarray, spec: Spec) -> Dict[str, np.ndarray]:
    """Blob-entry-name -> array view (for the oracle)."""
    out = {}
    off = 0
    for name, shape, _ in spec:
        n = int(np.prod(shape))
        out[name] = blob[off:off + n].reshape(shape)
        off += n
    if off != blob.size:
        raise ValueError(f"blob has {blob.size} floats, spec wants {off}")
    return out


def find_pretrained(model_name_or_path: str = "google/owlvit-base-patch32"):
    """Return a path to a local safetensors checkpoint, or None.

    No network: only a local directory / HF cache hit counts.
    """
    cands = []
    if os.path.isdir(model_name_or_path):
        cands.append(os.path.join(model_name_or_path, "model.safetensors"))
    hub = os.path.expanduser(os.environ.get("HF_HOME", "~/.cache/huggingface"))
    snap = os.path.join(hub, "hub", "models--" + model_name_or_path.replace("/", "--"), "snapshots")
    if os.path.isdir(snap):
        for d in sorted(os.listdir(snap)):
            cands.append(os.path.join(snap, d, "model.safetensors"))
    for c in cands:
        if os.path.isfile(c):
            return c
    return None


def load_safetensors_state_dict(path: str) -> Dict[str, np.ndarray]:
    from safetensors.numpy import load_file
    sd = load_file(path)
    return {k: np.asarray(v, dtype=np.float32) for k, v in sd.items()}


# ---- checkpoint geometry ----------------------------------------------------------------------------------------------
# configuration_owlvit.py / configuration_owlv2.py defaults: a key that a config.json leaves out holds these values
_VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=768,
                        patch_size=32)
_VISION_DEFAULTS_V2 = dict(_VISION_DEFAULTS, patch_size=16)
_TEXT_DEFAULTS = dict(hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8)
_VISION_FIXED = dict(hidden_size=V_D, intermediate_size=V_FF, num_hidden_layers=V_LAYERS, num_attention_heads=V_HEADS)
_TEXT_FIXED = dict(hidden_size=T_D, intermediate_size=T_FF, num_hidden_layers=T_LAYERS, num_attention_heads=T_HEADS)
_PATCH_SUFFIX = "vision_model.embeddings.patch_embedding.weight"
_POS_SUFFIX = "vision_model.embeddings.position_embedding.weight"
_PATCH_KEY = "owlvit." + _PATCH_SUFFIX
_POS_KEY = "owlvit." + _POS_SUFFIX
_GEOMETRY_KEYS = tuple(f + "." + k for f in FAMILIES for k in (_PATCH_SUFFIX, _POS_SUFFIX))


def geometry_of_config(cfg: dict) -> OwlGeometry:
    """The geometry an OWL-ViT / OWLv2 ``config.json`` (as a dict) describes; ValueError (naming what was found and what is
    supported) for anything but OWL-ViT B/32 and B/16 and OWLv2 B/16 at image 960."""
    mt = cfg.get("model_type", "owlvit")
    if mt not in FAMILIES:
        raise ValueError(f"config model_type {mt!r} is not supported (only owlvit and owlv2 are); supported: {SUPPORTED_TEXT}")
    vdef = _VISION_DEFAULTS if mt == "owlvit" else _VISION_DEFAULTS_V2
    vc = dict(vdef, **{k: v for k, v in (cfg.get("vision_config") or {}).items() if k in vdef})
    tc = dict(_TEXT_DEFAULTS, **{k: v for k, v in (cfg.get("text_config") or {}).items() if k in _TEXT_DEFAULTS})
    proj = cfg.get("projection_dim", PROJ)
    found = (f"vision hidden {vc['hidden_size']}, MLP {vc['intermediate_size']}, {vc['num_hidden_layers']} layers, "
             f"{vc['num_attention_heads']} heads, image {vc['image_size']}, patch {vc['patch_size']}; text hidden {tc['hidden_size']}, "
             f"MLP {tc['intermediate_size']}, {tc['num_hidden_layers']} layers, {tc['num_attention_heads']} heads; projection {proj}")
    ok = all(vc[k] == v for k, v in _VISION_FIXED.items()) and all(tc[k] == v for k, v in _TEXT_FIXED.items()) and proj == PROJ
    try:
        g = OwlGeometry(int(vc["image_size"]), int(vc["patch_size"]), family=mt)
    except (TypeError, ValueError):
        ok, g = False, None
    if not ok or g not in (SUPPORTED if mt == "owlvit" else (OWLV2_B16,)):
        raise ValueError(f"unsupported {'OWL-ViT' if mt == 'owlvit' else 'owlv2'} geometry ({found}); supported: {SUPPORTED_TEXT}")
    return g


def family_of_state_dict(keys) -> str:
    """"owlvit" or "owlv2" by the key prefix of the vision tower's patch embedding; ValueError when neither is there."""
    keys = set(keys)
    for f in FAMILIES:
        if f + "." + _PATCH_SUFFIX in keys or f + "." + _POS_SUFFIX in keys:
            return f
    raise ValueError(f"no {_PATCH_KEY} / {_POS_KEY} (nor their owlv2.* forms): not an OWL-ViT / OWLv2 detector state dict")


def geometry_of_state_dict(shapes) -> OwlGeometry:
    """The geometry the vision tensors' shapes imply: ``patch_embedding`` [768, 3, P, P] and ``position_embedding``
    [(image / P)^2 + 1, 768]; the family comes from the key prefix (``owlvit.`` / ``owlv2.``).  ``shapes``: HF name -> shape or
    array (a state dict works)."""
    shapes = {k: tuple(getattr(v, "shape", v)) for k, v in shapes.items() if k in _GEOMETRY_KEYS}
    fam = family_of_state_dict(shapes)
    pe, pos = shapes.get(fam + "." + _PATCH_SUFFIX), shapes.get(fam + "." + _POS_SUFFIX)
    if pe is None or pos is None:
        raise ValueError(f"no {fam}.{_PATCH_SUFFIX} / {fam}.{_POS_SUFFIX}: not an OWL-ViT / OWLv2 detector state dict")
    if len(pe) != 4 or pe[0] != V_D or pe[1] != 3 or pe[2] != pe[3]:
        raise ValueError(f"{fam} patch_embedding has shape {list(pe)}; supported: {SUPPORTED_TEXT}")
    for g in (SUPPORTED if fam == "owlvit" else (OWLV2_B16,)):
        if g.patch_size == pe[2]:
            if pos != (g.ntok, V_D):
                raise ValueError(f"{fam} position_embedding has shape {list(pos)}; patch {pe[2]} wants [{g.ntok}, {V_D}]")
            return g
    raise ValueError(f"{fam} patch_embedding has shape {list(pe)} (patch {pe[2]}); supported: {SUPPORTED_TEXT}")


def geometry_of_checkpoint(path: str) -> OwlGeometry:
    """Geometry of a local checkpoint (a directory or its ``model.safetensors``): ``config.json`` next to the weights
    (``model_type`` / ``vision_config`` / ``text_config`` / ``projection_dim``) cross-checked against the tensor names and
    shapes, which are read from the safetensors header alone.  A disagreement or an unsupported geometry raises ValueError;
    without a config.json the tensors decide."""
    st = os.path.join(path, "model.safetensors") if os.path.isdir(path) else path
    cfg_path = os.path.join(os.path.dirname(st), "config.json")
    g_cfg = None
    if os.path.isfile(cfg_path):
        with open(cfg_path) as f:
            g_cfg = geometry_of_config(json.load(f))
    if not os.path.isfile(st):
        if g_cfg is None:
            raise ValueError(f"{path!r} holds neither model.safetensors nor config.json")
        return g_cfg
    from safetensors import safe_open
    with safe_open(st, framework="numpy") as f:
        keys = set(f.keys())
        shapes = {k: tuple(f.get_slice(k).get_shape()) for k in _GEOMETRY_KEYS if k in keys}
    g_w = geometry_of_state_dict(shapes)
    if g_cfg is not None and g_cfg != g_w:
        raise ValueError(f"config.json says {g_cfg.name} (image {g_cfg.image_size}, patch {g_cfg.patch_size}) but the weights are "
                         f"{g_w.name}: " + ", ".join(f"{k} {list(v)}" for k, v in sorted(shapes.items())))
    return g_w
