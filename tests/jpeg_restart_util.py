"""Helpers of the restart-interval tests of the JPEG encoder: the matrix both the CPU and the GPU tests walk and Pillow's side.

Every reference JPEG is made at test time by Pillow's encoder (libjpeg-turbo); nothing binary is committed.
"""
import functools
import io

import numpy as np

from jpeg_encode_util import picture

# (H, W, subsampling): 5 x 3 MCUs; 3 x 4 MCUs of 16 x 8; 5 x 3 MCUs of one block; one MCU; 3 x 2 MCUs whose last column and last
# row hold dummy luma blocks (24 x 40 is 3 x 5 real blocks inside 4 x 6)
GEOMETRIES = [(45, 77, "4:2:0"), (31, 33, "4:2:2"), (24, 40, "4:4:4"), (8, 8, "4:2:0"), (24, 40, "4:2:0")]
QUALITIES = [30, 75, 100]
KINDS = ["smooth", "noise"]
# on 15 MCUs: 1 -> 14 markers (the D0..D7 numbering wraps), 4 -> a short last interval, 15 and 16 -> DRI and no marker
INTERVALS = [dict(restart_blocks=b) for b in (1, 3, 4, 7, 15, 16)] + [dict(restart_rows=1), dict(restart_rows=2),
                                                                      dict(restart_rows=2, restart_blocks=3)]       # rows win
# seed of the noise picture of each geometry, chosen with the host twin's counters so that over the corpus an interval ends
# byte-aligned, a padded byte comes out as 0xFF and data bytes are stuffed (test_the_corpus_reaches_every_path holds them to it)
NOISE_SEEDS = {(45, 77, "4:2:0"): 11, (31, 33, "4:2:2"): 12, (24, 40, "4:4:4"): 13, (8, 8, "4:2:0"): 14, (24, 40, "4:2:0"): 15}


def mcus(H, W, subsampling):
    hs, vs = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:4": (1, 1)}[subsampling]
    return -(-W // (8 * hs)), -(-H // (8 * vs))


def interval_of(H, W, subsampling, restart_rows=0, restart_blocks=0):
    return restart_rows * mcus(H, W, subsampling)[0] if restart_rows else restart_blocks


@functools.lru_cache(maxsize=None)
def rst_picture(kind, H, W, subsampling):
    if kind == "noise":
        a = np.random.RandomState(NOISE_SEEDS[(H, W, subsampling)]).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        a.setflags(write=False)
        return a
    return picture(kind, H, W)


def pillow_restart_bytes(a, quality=75, subsampling="4:2:0", restart_rows=0, restart_blocks=0):
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 8 * a.size + 65536)        # Pillow's encoder cannot grow its buffer mid-scan
    try:
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=restart_rows,
                                restart_marker_blocks=restart_blocks)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


def markers_of(scan):
    """The RSTn codes of a stuffed scan, in order (FF D0..D7 can only be a marker there)."""
    return [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]


def new_restart_counters():
    return np.zeros(3, dtype=np.uint64)
