"""What the CPU and the GPU tests of the re-coding with optimised Huffman tables share: Pillow's files as the yardstick of the
per-frame mode, a small DHT parser, and the groups' tables worked out from per-frame counts.

Every JPEG is made at test time (``jpeg_recode_util``); nothing binary is committed.
"""
import functools
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_recode_util as U  # noqa: E402
import jpeg_util as JU  # noqa: E402

# geometries the interval-free re-code is held against Pillow's optimize=True file on
PLAIN_GEOMETRIES = [(48, 48, "420"), (17, 9, "420"), (40, 24, "422"), (24, 40, "444")]


def pillow_optimized(rgb, sampling, quality, interval=0):
    """Pillow's ``save(quality=, subsampling=, optimize=True[, restart_marker_blocks=interval])``."""
    from PIL import Image
    kw = dict(quality=quality, subsampling=JU.SUBSAMPLING[sampling], optimize=True)
    if interval:
        kw["restart_marker_blocks"] = interval
    return U._save(Image.fromarray(rgb), **kw)


@functools.lru_cache(maxsize=None)
def groups_of_one_cases():
    """The smallest inputs on which tables per frame and tables shared by groups of ONE frame take every branch -> ((files, interval,
    the per-frame files of the host twin, its stats), ...), worked out once: three different 48x48 4:2:0 frames at an interval of 2
    (9 MCUs: 5 intervals, the last one short) with a grayscale file, which is kept and belongs to no group, among them; and one
    24x16 4:4:4 frame without an interval (no DRI)."""
    from tstar_amd import jpeg_recode as JR
    cases = []
    for files, n in (([U.source(48, 48, "420", "q75")[1], U.source(48, 48, "420", "gray")[1], U.source(48, 48, "420", "noise100")[1],
                       U.source(48, 48, "420", "qtables", 1)[1]], 2), ([U.source(24, 16, "444", "q75")[1]], 0)):
        stats = {}
        cases.append((files, n, JR.recode_host(files, n, stats, optimize=True), stats))
    return tuple(cases)


def without(stats, key):
    return {k: v for k, v in stats.items() if k != key}


def pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def dht_tables(data):
    """The DHT segments of a file in order -> [(id byte, bits uint8 [16], huffval bytes)]; one table per segment is expected."""
    segs, _ = JU.segments(data)
    out = []
    for m, a, b in segs:
        if m == 0xC4:
            body = data[a + 4:b]
            n = sum(body[1:17])
            assert len(body) == 17 + n, "a DHT segment with more than one table"
            out.append((body[0], np.frombuffer(body[1:17], dtype=np.uint8), bytes(body[17:17 + n])))
    return out


def markers(data):
    """(DRI value or 0, the RSTn markers of the scan in order as numbers 0..7)."""
    segs, scan_at = JU.segments(data)
    dri = 0
    for m, a, b in segs:
        if m == 0xDD:
            dri = int.from_bytes(data[a + 4:a + 6], "big")
    scan = data[scan_at:]
    found = [scan[i + 1] - 0xD0 for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    return dri, found


def frame_counts(data, interval):
    """The symbol counts uint32 [4, 257] the encoder's walk gives one covered file's coefficients at this interval."""
    from tstar_amd import jpeg_encode as JE
    geom, coef, _ = U.host_coefficients(data)
    tables = {}
    JE.scan_host(coef[None], geom[0], geom[1], {(2, 2): "4:2:0", (2, 1): "4:2:2", (1, 1): "4:4:4"}[(geom[3], geom[4])], threads=1,
                 restart_blocks=interval, optimize=True, tables=tables)
    return tables["hist"][0]


def tables_of_counts(counts):
    """uint32 [4, 257] -> [(bits list, huffval bytes)] x 4 through the pure table procedure."""
    from tstar_amd import jpeg_encode as JE
    out = []
    for t in range(4):
        got = JE.huff_optimal(counts[t, :256])
        assert got["status"] == JE.HUFF_OK
        out.append((got["bits"].tolist(), got["vals"]))
    return out


def fibonacci_hist(n_groups, group=0, table=0, symbols=33):
    """Counts [n_groups, 4, 257] of ordinary shape (every DC category and every AC symbol once, so that any frame can be coded
    and any decoder takes the tables) but for one table of one group: 1, 2, 3, 5, 8, ... on ``symbols`` symbols, whose optimal code
    is ``symbols`` bits deep beside the reserved symbol (33: the overflow)."""
    h = np.zeros((n_groups, 4, 257), dtype=np.uint32)
    h[:, [0, 2], :12] = 1
    h[:, [1, 3], :256] = 1
    f = [1, 2]
    while len(f) < symbols:
        f.append(f[-1] + f[-2])
    h[group, table] = 0
    h[group, table, :symbols] = f[:symbols]
    return h
