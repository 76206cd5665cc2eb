"""What the CPU and the GPU tests of the scaled JPEG decode (1/2, 1/4, 1/8 size) share: the pictures, Pillow's draft as the
yardstick, the coefficients of a file and the calls of the scaled entries."""
import ctypes as C
import functools
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402

SCALES = (2, 4, 8)
# (W, H).  10 x 8 and 40 x 8 give 4:2:2 its shortest covered chroma row, 3 samples, at scale 2 and at scale 8
SIZES = [(8, 8), (16, 16), (17, 9), (33, 31), (77, 45), (40, 24), (200, 120), (10, 8), (40, 8)]
SAMPLINGS = JU.SAMPLINGS
QUALITIES = (5, 75, 100)
KINDS = ("noise", "gradient", "checkerboard")


def ceil_div(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def picture(kind, W, H, seed=0):
    """uint8 [H,W,3]: uniform noise, a two-way colour gradient, or a 3-pixel checkerboard of two saturated colours."""
    if kind == "noise":
        out = JU.noise_picture(H, W, seed=seed + 31 * W + H)
    elif kind == "gradient":
        y, x = np.mgrid[0:H, 0:W]
        out = np.stack([x * 255 // max(1, W - 1), y * 255 // max(1, H - 1), (x + y + seed) * 255 // max(1, W + H - 2 + seed)], axis=-1)
        out = out.astype(np.uint8)
    else:
        y, x = np.mgrid[0:H, 0:W]
        on = (((x + seed) // 3 + y // 3) & 1).astype(bool)
        out = np.where(on[..., None], np.array([255, 16, 240], np.uint8), np.array([0, 230, 20], np.uint8)).astype(np.uint8)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def pillow_draft(data, s):
    """The yardstick: Pillow (libjpeg-turbo) decoding ``data`` at 1/s size.  The draft must have taken exactly this scale."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        W, H = im.size
        im.draft(im.mode, (W // s, H // s))
        assert im.size == (ceil_div(W, s), ceil_div(H, s)), f"Pillow's draft of {W}x{H} at 1/{s} gave {im.size}"
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def coefficients(datas):
    """Files of one covered geometry -> (geom, coef int16 [n, blocks * 64], quant uint16 [n, 192]) by the host entropy stage."""
    from tstar_amd import jpeg
    rc, geom, msg = jpeg.probe(datas[0])
    assert rc == jpeg.OK, msg
    blocks, _ = jpeg._sizes(geom)
    coef = np.zeros((len(datas), blocks * 64), dtype=np.int16)
    quant = np.zeros((len(datas), 192), dtype=np.uint16)
    status, msg = jpeg.entropy_batch(list(datas), geom, coef, quant, 1)
    assert not status.any(), msg
    return geom, coef, quant


def sizes(geom, s):
    """tstar_jpeg_sizes_scaled -> (rc, ow, oh, plane bytes, covered)."""
    from tstar_amd import _lib
    out = (C.c_size_t * 4)(7, 7, 7, 7)
    rc = _lib.load().tstar_jpeg_sizes_scaled(*geom, s, out)
    return (rc, *(int(v) for v in out))


def reconstruct_host(geom, coef, quant, s, threads=1):
    """tstar_jpeg_reconstruct_scaled_host into a buffer filled with 0xA5 -> (rc, uint8 [n, oh, ow, 3])."""
    from tstar_amd import _lib
    n, W, H = len(coef), geom[0], geom[1]
    out = np.full((n, ceil_div(H, s), ceil_div(W, s), 3), 0xA5, dtype=np.uint8)
    rc = _lib.load().tstar_jpeg_reconstruct_scaled_host(coef.ctypes.data, quant.ctypes.data, n, *geom, s, out.ctypes.data, threads)
    return rc, out


def chroma_row(W, sampling, s):
    """Samples of a scaled chroma row that goes through the triangle filter, else None (the rule of DESIGN.md 8j)."""
    k = 8 // s
    return ceil_div(W * k, 16) if sampling == "422" and k >= 2 else None


def covered(W, sampling, s):
    cw = chroma_row(W, sampling, s)
    return cw is None or cw > 2
