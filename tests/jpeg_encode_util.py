"""Helpers of the JPEG encoder tests: the matrix both the CPU and the GPU tests walk, the test pictures and Pillow's side.

Every reference JPEG is made at test time by Pillow's encoder (libjpeg-turbo); nothing binary is committed.
"""
import functools
import io
import struct

import numpy as np

SMALL_SIZES = [(1, 1), (2, 3), (8, 8), (16, 16), (17, 23), (24, 40), (33, 7), (45, 80), (90, 161)]       # H x W
QUALITIES = [5, 30, 75, 95, 100]
SUBSAMPLINGS = ["4:2:0", "4:2:2", "4:4:4"]
CONTENTS = ["noise", "smooth", "black", "white", "red", "green", "blue"]


def pillow_bytes(a, quality=75, subsampling="4:2:0"):
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 8 * a.size)        # Pillow's encoder cannot grow its buffer mid-scan (noise at quality 100)
    try:
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def picture(content, H, W):
    from PIL import Image
    rs = np.random.RandomState(1000 * H + W)
    if content == "noise":
        a = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    elif content == "smooth":                         # a small random image resized up with bicubic
        small = rs.randint(0, 256, size=(max(2, H // 8), max(2, W // 8), 3)).astype(np.uint8)
        a = np.asarray(Image.fromarray(small).resize((W, H), Image.BICUBIC))
    else:
        rgb = {"black": (0, 0, 0), "white": (255, 255, 255), "red": (255, 0, 0), "green": (0, 255, 0), "blue": (0, 0, 255)}[content]
        a = np.empty((H, W, 3), dtype=np.uint8)
        a[:] = rgb
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def sos_end(data):
    """Offset one past the SOS segment: where the entropy-coded bytes start."""
    p = 2
    while True:
        assert data[p] == 0xFF
        m, L = data[p + 1], struct.unpack(">H", data[p + 2:p + 4])[0]
        p += 2 + L
        if m == 0xDA:
            return p


def new_counters():
    return np.zeros(5, dtype=np.uint64)
