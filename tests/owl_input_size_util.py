"""Helpers of tests/test_owl_input_size.py and tests/test_gpu_owl_input_size.py (and of the script that records
tests/golden/attention_t32n1_crc.txt): seeded attention inputs and their CRCs, a float64 attention reference, and HF's own
forward / image processor at an input size other than the checkpoint's (``interpolate_pos_encoding=True``)."""
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CRC_GOLDEN = os.path.join(HERE, "golden", "attention_t32n1_crc.txt")
CRC_CASES = (577, 2305)                     # T % 32 == 1: the code path whose bits must not move (B = 2, 12 heads)
ATTN_KERNELS = ("f32", "split", "x3")


def attention_input(T, B=2, heads=12, seed=None):
    """float32 qkv [B*T, 3*64*heads] from numpy's frozen legacy stream (the same bytes on every machine)."""
    rs = np.random.RandomState(T if seed is None else seed)
    return rs.standard_normal((B * T, 3 * 64 * heads)).astype(np.float32)


def run_attention(lib, name, dqkv, out, B, T, heads):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    if name == "f32":
        return lib.tstar_attention_f32(dqkv.data_ptr(), out.data_ptr(), B, T, heads, 0, None, st)
    if name == "split":
        return lib.tstar_attention_split(dqkv.data_ptr(), out.data_ptr(), B, T, heads, st)
    return lib.tstar_attention_x3(dqkv.data_ptr(), out.data_ptr(), B, T, heads, st)


def attention_crcs():
    """{(kernel, T): crc32 of the output bytes} for the seeded inputs of CRC_CASES, on the current device."""
    import torch
    from tstar_amd import _lib
    lib = _lib.load()
    out = {}
    for T in CRC_CASES:
        B, heads = 2, 12
        dqkv = torch.from_numpy(attention_input(T, B, heads)).cuda()
        for name in ATTN_KERNELS:
            o = torch.full((B * T, heads * 64), float("nan"), device="cuda")
            _lib.check(run_attention(lib, name, dqkv, o, B, T, heads))
            torch.cuda.synchronize()
            out[(name, T)] = zlib.crc32(o.cpu().numpy().tobytes()) & 0xFFFFFFFF
    return out


def format_crcs(crcs):
    return "".join(f"{k} {T} {crcs[(k, T)]:08x}\n" for T in CRC_CASES for k in ATTN_KERNELS)


def read_crc_golden():
    out = {}
    with open(CRC_GOLDEN) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                k, T, c = line.split()
                out[(k, int(T))] = int(c, 16)
    return out


def attn_ref64(qkv, B, T, heads):
    """softmax(Q K^T / 8) V in float64, one image at a time (qkv: CPU float32 tensor [B*T, 3*64*heads])."""
    import torch
    D = heads * 64
    out = []
    for b in range(B):
        q, k, v = qkv[b * T:(b + 1) * T].double().view(T, 3 * D).split(D, dim=-1)
        q = q.view(T, heads, 64).transpose(0, 1)
        k = k.view(T, heads, 64).transpose(0, 1)
        v = v.view(T, heads, 64).transpose(0, 1)
        att = torch.softmax(torch.matmul(q, k.transpose(1, 2)) * 0.125, dim=-1)
        out.append(torch.matmul(att, v).transpose(0, 1).reshape(T, D))
    return torch.cat(out)


def make_hf_model(patch_size=32, seed=0):
    """HF's ``OwlViTForObjectDetection`` at its own init (no files written)."""
    import torch
    import transformers
    torch.manual_seed(seed)
    cfg = transformers.OwlViTConfig() if patch_size == 32 else transformers.OwlViTConfig(vision_config={"patch_size": patch_size})
    return transformers.OwlViTForObjectDetection(cfg).eval()


def make_checkpoint_dir(dirpath, patch_size=32, seed=0):
    """tests/hf_checkpoint_util.make_checkpoint_dir for either patch size: HF's model at its own init with the class head's
    scale / shift and the box head shrunk the same way (unsaturated scores and boxes), ``save_pretrained`` + a CLIP vocabulary."""
    import torch
    from clip_vocab_util import write_clip_vocab
    m = make_hf_model(patch_size, seed)
    with torch.no_grad():
        for lin in (m.class_head.logit_scale, m.class_head.logit_shift):
            lin.weight.mul_(0.01)
            lin.bias.mul_(0.01)
        for lin in (m.box_head.dense0, m.box_head.dense1, m.box_head.dense2):
            lin.weight.mul_(lin.weight.shape[1] ** -0.5)
    os.makedirs(dirpath, exist_ok=True)
    m.save_pretrained(dirpath, safe_serialization=True)
    write_clip_vocab(dirpath)
    return m


def hf_pixels(image, size):
    """float32 [3, h, w]: HF's own Pillow image processor at ``size`` = (h, w) on one HxWx3 uint8 image."""
    from transformers.models.owlvit import image_processing_pil_owlvit as P
    proc = P.OwlViTImageProcessorPil(size={"height": int(size[0]), "width": int(size[1])})
    px = proc(images=[image], return_tensors="np")["pixel_values"][0]
    return np.ascontiguousarray(px, dtype=np.float32)


def hf_detect_at(model, tokenizer, image, names, size, threshold=0.005):
    """tests/hf_checkpoint_util.hf_detect at input ``size`` = (h, w): pixels from HF's own image processor at that size,
    forward with ``interpolate_pos_encoding=True``; same post-processing (boxes in pixels of the passed image)."""
    import torch
    enc = tokenizer(names, padding="max_length", max_length=16, truncation=True, return_tensors="pt")
    px = torch.from_numpy(hf_pixels(image, size)[None])
    with torch.no_grad():
        o = model(input_ids=enc["input_ids"], attention_mask=enc["attention_mask"], pixel_values=px, interpolate_pos_encoding=True)
    logits, boxes = o.logits[0], o.pred_boxes[0]
    mx = logits.max(dim=-1)
    scores, labels = torch.sigmoid(mx.values), mx.indices
    cx, cy, w, h = boxes.unbind(-1)
    H, W = image.shape[:2]
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1) * torch.tensor([W, H, W, H], dtype=torch.float32)
    keep = scores > threshold
    return dict(dense_scores=scores.numpy(), scores=scores[keep].numpy(), labels=labels[keep].numpy(), xyxy=xyxy[keep].numpy(),
                text_embeds=o.text_embeds[0].numpy())
