"""What the CPU and the GPU tests of the lossless JPEG re-coding share: the geometry / interval cases, the sources, a crafted frame
the standard tables cannot code, and the comparison of a piece's records with the planner's.

Every JPEG is made at test time by Pillow's encoder (libjpeg-turbo) or assembled by hand here; nothing binary is committed.
"""
import functools
import io
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402

# (W, H, sampling, interval in MCUs): one MCU; dummy blocks on both edges; nine intervals (RST7 -> RST0 wraps); two small intervals
# at 4:2:2 and 4:4:4; an interval larger than the frame (DRI present, no marker)
CASES = [(16, 16, "420", 2), (17, 9, "420", 1), (48, 48, "420", 1), (40, 24, "422", 1), (40, 24, "422", 2), (24, 40, "444", 1),
         (24, 40, "444", 2), (48, 48, "420", 1000), (24, 40, "444", 65535)]
CASE_IDS = [f"{w}x{h}-{s}-n{n}" for w, h, s, n in CASES]
# sources every case is re-coded from; all of them must be RE-CODED (kept == 0)
SOURCES = ["q75", "noise100", "restart", "optimize", "qtables"]
PILLOW_SOURCES = {"q75": 75, "noise100": 100, "optimize": 75}        # source -> the quality Pillow is asked again with an interval
KEPT_SOURCES = ["gray", "progressive", "category11"]

# custom tables: a flat luma table and a chroma table with values above 255 (16-bit DQT entries, SOF1)
QTABLES = [[3 + (k % 7) for k in range(64)], [40 + 9 * k for k in range(64)]]


def _save(im, **kw):
    from PIL import ImageFile
    buf = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 1 << 20)
    try:
        im.save(buf, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def picture(W, H, source, seed=0):
    if source == "noise100":
        return JU.noise_picture(H, W, seed=7 + seed)
    pic = JU.synthetic_picture(H, W, frame=(3 + seed) % 16).copy()
    pic[::3, ::2] ^= np.uint8(0x55 + seed)                           # texture: every block carries AC coefficients
    return pic


@functools.lru_cache(maxsize=None)
def source(W, H, sampling, name, seed=0):
    """(rgb uint8 [H,W,3], JPEG bytes) of one source."""
    from PIL import Image
    rgb = picture(W, H, name, seed)
    im = Image.fromarray(rgb)
    sub = JU.SUBSAMPLING[sampling]
    if name == "q75":
        data = _save(im, quality=75, subsampling=sub)
    elif name == "noise100":
        data = _save(im, quality=100, subsampling=sub)
    elif name == "restart":
        data = _save(im, quality=90, subsampling=sub, restart_marker_blocks=3)
    elif name == "optimize":
        data = _save(im, quality=75, subsampling=sub, optimize=True)
    elif name == "qtables":
        data = _save(im, qtables=QTABLES, subsampling=sub)
    elif name == "gray":
        data = _save(im.convert("L"), quality=75)
    elif name == "progressive":
        data = _save(im, quality=75, subsampling=sub, progressive=True)
    elif name == "category11":
        data = category11_frame(W, H, sampling)
    else:
        raise KeyError(name)
    return rgb, data


def pillow_with_interval(rgb, sampling, quality, interval):
    from PIL import Image
    return _save(Image.fromarray(rgb), quality=quality, subsampling=JU.SUBSAMPLING[sampling], restart_marker_blocks=interval)


def category11_frame(W, H, sampling):
    """A three-component baseline frame of the case's geometry, assembled by hand, whose first luma block holds an AC coefficient of
    1024: size category 11, which the standard AC tables have no code for.  One DC table {0} (code 0) and one AC table {EOB: 0,
    run 0 / size 11: 10} serve every component; every other block is DC 0 + EOB."""
    hs, vs = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}[sampling]
    mcus = (-(-W // (8 * hs))) * (-(-H // (8 * vs)))
    blocks = mcus * (hs * vs + 2)
    bits = "0" + "10" + format(1024, "011b") + "0" + "00" * (blocks - 1)
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    assert b"\xff" not in scan

    def seg(marker, payload):
        return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xDB, b"\x00" + bytes([1] * 64))
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, (hs << 4) | vs, 0, 2, 0x11, 0, 3, 0x11, 0]))
    out += seg(0xC4, b"\x00" + bytes([1] + [0] * 15) + b"\x00")                     # DC 0: one code of length 1 -> category 0
    out += seg(0xC4, b"\x10" + bytes([1, 1] + [0] * 14) + b"\x00\x0b")              # AC 0: EOB, then run 0 / size 11
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x00, 3, 0x00, 0, 63, 0]))
    return out + scan + b"\xff\xd9"


def dqt_payloads(data):
    """The payloads of the DQT segments in file order, joined."""
    segs, _ = JU.segments(data)
    return b"".join(data[a + 4:b] for m, a, b in segs if m == 0xDB)


def host_coefficients(data):
    """(geometry, coef int16, quant uint16 [192]) of one file through the project's host decoder."""
    from tstar_amd import jpeg
    rc, geom, msg = jpeg.probe(data)
    assert rc == jpeg.OK, msg
    blocks = jpeg._sizes(geom)[0]
    coef = np.zeros((1, blocks * 64), dtype=np.int16)
    quant = np.zeros((1, 192), dtype=np.uint16)
    status, msg = jpeg.entropy_batch([data], geom, coef, quant, 1)
    assert status[0] == jpeg.OK, msg
    return tuple(geom), coef[0], quant[0]


def batch(W, H, sampling, with_kept=True):
    """Files of one geometry and different lengths: every source twice (other pictures), kept ones in between."""
    files = []
    for seed in (0, 1):
        for name in SOURCES:
            files.append(source(W, H, sampling, name, seed)[1])
        if with_kept:
            files.insert(len(files) - 2, source(W, H, sampling, KEPT_SOURCES[seed], seed)[1])
    if with_kept:
        files.append(source(W, H, sampling, "category11")[1])
    return files


def n_kept(files):
    from tstar_amd import jpeg
    kept = 0
    for f in files:
        rc, geom, _ = jpeg.probe(f)
        if rc != jpeg.OK or geom[2] != 3:
            kept += 1
        else:
            blocks = jpeg._sizes(geom)[0]
            st, _ = jpeg.entropy_batch([f], geom, np.zeros((1, blocks * 64), np.int16), np.zeros((1, 192), np.uint16), 1)
            kept += int(st[0] != jpeg.OK)
    return kept


def arena_of_plans(plans_lens):
    """[(SegmentPlan, lens)] -> the Arena an open builds of them (jpeg_resident.ArenaBuilder)."""
    from tstar_amd import jpeg_resident
    b = jpeg_resident.ArenaBuilder()
    for plan, lens in plans_lens:
        b.add(plan, lens)
    return b.finish()


def assert_arenas_equal(got, want):
    """Field for field: off, len, quant, frame records, segments, table sets."""
    for name in ("off", "len", "quant", "frames", "segments", "table_sets"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"arena.{name} differs"
