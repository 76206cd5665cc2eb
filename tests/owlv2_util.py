"""Helpers of tests/test_owlv2_host.py and tests/test_gpu_owlv2.py: a float64 numpy restatement of HF's
``Owlv2ImageProcessorPil`` (pad to a square, scipy's Gaussian anti-aliasing filter, ``scipy.ndimage.zoom(order=1,
mode="mirror", grid_mode=True)``, clip, normalise), HF's own processor / forward as the witnesses, an HF-initialised OWLv2
checkpoint directory, and the CRC of the OWL-ViT B/16 run at (960, 960) whose bits this feature must not move."""
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B16_960_GOLDEN = os.path.join(HERE, "golden", "owlvit_b16_960_crc.txt")
B16_960_MODES = ("f32", "f32x3")


# ------------------------------------------------------------------------------------------- OWL-ViT B/16 at (960, 960)
def b16_960_crcs():
    """{mode: crc32} of scores | labels | boxes | logits | cell_conf of ONE seeded 285 x 600 image through a synthetic OWL-ViT
    B/16 scorer with ``input_size=(960, 960)`` (T = 3601, the token count OWLv2 runs at), on the current device."""
    import torch
    from tstar_amd import weights as W
    from tstar_amd.owl import OwlScorer
    from tstar_amd.tokenizer import encode_queries
    g = W.with_input_size(W.B16, (960, 960))
    sd = W.synthetic_state_dict(0, geometry=g)
    vb, tb = W.pack_blob(sd, W.vision_spec(g), g), W.pack_blob(sd, W.text_spec())
    ids, am = encode_queries([["couch"], ["tv"], ["chair"], [" "]], "google/owlvit-base-patch32", allow_standin=True)
    img = torch.from_numpy(np.random.RandomState(960).randint(0, 256, (1, 285, 600, 3)).astype(np.uint8)).cuda()
    out = {}
    for mode in B16_960_MODES:
        s = OwlScorer(vb, tb, max_batch=1, weights_mode=mode, patch_size=16, input_size=(960, 960))
        s.set_queries(ids, am, [1.0, 0.5, 0.5, 0.5])
        r = s.score(img, 4, 4, want_logits=True)
        torch.cuda.synchronize()
        c = 0
        for f in ("scores", "labels", "boxes", "logits", "cell_conf"):
            c = zlib.crc32(getattr(r, f).cpu().numpy().tobytes(), c)
        out[mode] = c & 0xFFFFFFFF
        s.close()
    return out


def format_b16_960(crcs):
    return "".join(f"{m} {crcs[m]:08x}\n" for m in B16_960_MODES)


def read_b16_960_golden():
    out = {}
    with open(B16_960_GOLDEN) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                m, c = line.split()
                out[m] = int(c, 16)
    return out


# -------------------------------------------------------------------------------------- the processor, restated in numpy
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
# (source (H, W), target (h, w)): the six of the issue, one square source (no padding: the lower clip bound is not 0) and one
# where a single axis shrinks
PROCESSOR_CASES = [((285, 600), (960, 960)), ((1520, 3200), (960, 960)), ((380, 800), (64, 96)), ((95, 200), (96, 64)),
                   ((37, 23), (64, 64)), ((700, 500), (480, 640)), ((131, 131), (64, 96)), ((600, 600), (480, 960))]


def rescale_table():
    """float32 [256]: HF's rescale, float32(float64(u8) * (1 / 255))."""
    return (np.arange(256, dtype=np.float64) * (1 / 255)).astype(np.float32)


def mirror(i, S):
    """scipy's "mirror" extension about the edge SAMPLES (-1 -> 1, S -> S - 2), for indices at most S - 1 outside."""
    i = np.abs(np.asarray(i))
    return np.where(i > S - 1, 2 * (S - 1) - i, i)


def axis_sigma(S, out):
    """(sigma, radius) of the anti-aliasing filter on an axis of S samples resized to ``out``; radius -1: the axis is skipped."""
    sigma = max(0.0, (S / out - 1) / 2)
    if sigma <= 1e-15:
        return sigma, -1
    return sigma, int(4.0 * sigma + 0.5)


def gaussian_weights(sigma, lw):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, lw), float64 [2 lw + 1]."""
    x = np.arange(-lw, lw + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def zoom_taps(S, out):
    """(i0, i1, t) per output index of ``scipy.ndimage.zoom(order=1, mode="mirror", grid_mode=True)`` from S to ``out``."""
    cc = (np.arange(out) + 0.5) * (S / out) - 0.5
    c = np.abs(cc)
    c = np.where(c > S - 1, 2 * (S - 1) - c, c)
    i0 = np.floor(c).astype(np.int64)
    return i0, mirror(i0 + 1, S), c - i0


def filter_axis(x, axis, S, out):
    """The Gaussian pass of one axis on float32 ``x`` [S, S, 3] (float64 accumulation in scipy's correlate1d order for a
    symmetric kernel, one rounding to float32); the axis unchanged when its sigma is skipped."""
    sigma, lw = axis_sigma(S, out)
    if lw < 0:
        return x
    w = gaussian_weights(sigma, lw)
    xm = np.moveaxis(x, axis, 0).astype(np.float64)
    idx = np.arange(S)
    acc = xm * w[lw]
    for k in range(lw, 0, -1):                           # correlate1d's symmetric loop starts at the outermost pair
        acc = acc + (xm[mirror(idx - k, S)] + xm[mirror(idx + k, S)]) * w[lw - k]
    return np.moveaxis(acc.astype(np.float32), 0, axis)


def preprocess_restated(image, size, normalize=True):
    """float32 [3, h, w]: ``Owlv2ImageProcessorPil(size=...)`` on one HxWx3 uint8 image, restated."""
    H, W = image.shape[:2]
    h, w = size
    S = max(H, W)
    sq = np.zeros((S, S, 3), np.float32)
    sq[:H, :W] = rescale_table()[image]
    lo, hi = sq.min(), sq.max()
    x = filter_axis(sq, 0, S, h)
    x = filter_axis(x, 1, S, w)
    y0, y1, ty = zoom_taps(S, h)
    x0, x1, tx = zoom_taps(S, w)
    x = x.astype(np.float64)
    wy0, wy1 = (1 - ty)[:, None, None], ty[:, None, None]
    wx0, wx1 = (1 - tx)[None, :, None], tx[None, :, None]
    z = (x[y0][:, x0] * wy0) * wx0
    z = z + (x[y0][:, x1] * wy0) * wx1
    z = z + (x[y1][:, x0] * wy1) * wx0
    z = z + (x[y1][:, x1] * wy1) * wx1
    z = np.clip(z.astype(np.float32), lo, hi)
    if normalize:
        z = (z - np.array(CLIP_MEAN, np.float32)) / np.array(CLIP_STD, np.float32)
    return np.ascontiguousarray(z.transpose(2, 0, 1), dtype=np.float32)


def hf_pixels(image, size, normalize=True):
    """float32 [3, h, w]: HF's own ``Owlv2ImageProcessorPil`` at ``size`` = (h, w) on one HxWx3 uint8 image."""
    from transformers.models.owlv2.image_processing_pil_owlv2 import Owlv2ImageProcessorPil
    proc = Owlv2ImageProcessorPil(size={"height": int(size[0]), "width": int(size[1])}, do_normalize=bool(normalize))
    px = proc(images=[image], return_tensors="np")["pixel_values"][0]
    return np.ascontiguousarray(px, dtype=np.float32)


def im2col(px, P=16):
    """float32 [3, h, w] -> the patch-embed A operand [gh * gw, 3 P P] (row = patch, column = c P P + y P + x)."""
    _, h, w = px.shape
    gh, gw = h // P, w // P
    return np.ascontiguousarray(px.reshape(3, gh, P, gw, P).transpose(1, 3, 0, 2, 4).reshape(gh * gw, 3 * P * P))


def axis_reads(S, out, j0, j1):
    """(lowest, highest) source index of an axis that the restatement reads for the outputs [j0, j1): their zoom taps and, around
    each tap, the Gaussian's radius, mirrored at the square's edges."""
    _, lw = axis_sigma(S, out)
    lw = max(lw, 0)
    i0, i1, _ = zoom_taps(S, out)
    taps = np.concatenate([i0[j0:j1], i1[j0:j1]])
    reach = np.concatenate([mirror(taps + k, S) for k in range(-lw, lw + 1)])
    return int(reach.min()), int(reach.max())


# ------------------------------------------------------------------------------------------------------------- HF's model
def make_hf_model(seed=0):
    """HF's ``Owlv2ForObjectDetection`` (base widths, image 960, patch 16) at its own init."""
    import torch
    import transformers
    torch.manual_seed(seed)
    cfg = transformers.Owlv2Config(vision_config={"image_size": 960, "patch_size": 16})
    return transformers.Owlv2ForObjectDetection(cfg).eval()


def make_checkpoint_dir(dirpath, seed=0):
    """tests/owl_input_size_util.make_checkpoint_dir for OWLv2: HF's model at its own init with the class head's scale / shift
    x 0.01 and the box head shrunk by 1 / sqrt(fan_in) (unsaturated scores and boxes), ``save_pretrained`` + a CLIP vocabulary.
    The objectness head is a second box-head-shaped MLP with the same unit-variance init (logits in the tens of thousands, where
    one float32 ulp is already 4e-3): it is shrunk the same way, so its logits are O(1) and an absolute bound means something."""
    import torch
    from clip_vocab_util import write_clip_vocab
    m = make_hf_model(seed)
    with torch.no_grad():
        for lin in (m.class_head.logit_scale, m.class_head.logit_shift):
            lin.weight.mul_(0.01)
            lin.bias.mul_(0.01)
        for head in (m.box_head, m.objectness_head):
            for lin in (head.dense0, head.dense1, head.dense2):
                lin.weight.mul_(lin.weight.shape[1] ** -0.5)
    os.makedirs(dirpath, exist_ok=True)
    m.save_pretrained(dirpath, safe_serialization=True)
    write_clip_vocab(dirpath)
    return m


def hf_detect_at(model, tokenizer, image, names, size, threshold=0.005):
    """HF's OWLv2 detector on the CPU at input ``size`` = (h, w): pixels from ``Owlv2ImageProcessorPil`` at that size, forward
    with ``interpolate_pos_encoding=True``, HF's own ``post_process_object_detection`` with ``target_sizes=[(H, W)]``."""
    import torch
    from transformers.models.owlv2.image_processing_pil_owlv2 import Owlv2ImageProcessorPil
    enc = tokenizer(names, padding="max_length", max_length=16, truncation=True, return_tensors="pt")
    px = torch.from_numpy(hf_pixels(image, size)[None])
    with torch.no_grad():
        o = model(input_ids=enc["input_ids"], attention_mask=enc["attention_mask"], pixel_values=px, interpolate_pos_encoding=True)
    H, W = image.shape[:2]
    post = Owlv2ImageProcessorPil().post_process_object_detection(o, threshold=threshold, target_sizes=[(H, W)])[0]
    dense = torch.sigmoid(o.logits[0].max(dim=-1).values)
    return dict(dense_scores=dense.numpy(), scores=post["scores"].numpy(), labels=post["labels"].numpy(), xyxy=post["boxes"].numpy(),
                text_embeds=o.text_embeds[0].numpy(), objectness=o.objectness_logits[0].numpy())
