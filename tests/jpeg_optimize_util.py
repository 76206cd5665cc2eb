"""Helpers of the optimised-Huffman-table tests of the JPEG encoder: Pillow's side, a Python restatement of libjpeg's table
procedure (jchuff.c: jpeg_gen_optimal_table), a reader of the tables and symbol counts of a finished file, and the pictures.

Every reference JPEG is made at test time by Pillow's encoder (libjpeg-turbo); nothing binary is committed.
"""
import functools
import io
import struct

import numpy as np

from jpeg_encode_util import sos_end
from jpeg_restart_util import GEOMETRIES, rst_picture        # noqa: F401 -- the matrix of the tests

QUALITIES = [1, 30, 75, 100]
KINDS = ["smooth", "noise"]
INTERVALS = [dict(), dict(restart_blocks=1), dict(restart_blocks=4), dict(restart_blocks=16), dict(restart_rows=1)]
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def pillow_optimize_bytes(a, quality=75, subsampling="4:2:0", restart_rows=0, restart_blocks=0):
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 8 * a.size + 65536)        # Pillow's encoder cannot grow its buffer mid-scan
    try:
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=subsampling, optimize=True, restart_marker_rows=restart_rows,
                                restart_marker_blocks=restart_blocks)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


# ------------------------------------------------------------------------------------------------ the procedure, restated
OK, CLEN_OVERFLOW = 0, 1


def optimal_table(freq):
    """256 counts (at least one not zero) -> (bits [16], huffval bytes, status, limiting steps): the five points of the procedure.
    Sizes by libjpeg's own bookkeeping (codesize / others chains), not by a tree, so that it checks the project's parent links."""
    f = [int(v) for v in freq] + [1]                   # the reserved symbol
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1 = -1
        for i in range(257):                           # smallest non-zero count, ties to the largest index
            if f[i] and (c1 < 0 or f[i] <= f[c1]):
                c1 = i
        c2 = -1
        for i in range(257):
            if f[i] and i != c1 and (c2 < 0 or f[i] <= f[c2]):
                c2 = i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    if max(codesize) > 32:
        return [0] * 16, b"", CLEN_OVERFLOW, 0
    bits = [0] * 33
    for s in codesize:
        if s:
            bits[s] += 1
    steps = 0
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
            steps += 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                       # the reserved symbol's code
    huffval = bytes(j for s in range(1, 33) for j in range(256) if codesize[j] == s)
    return bits[1:17], huffval, OK, steps


def canonical_codes(bits, huffval):
    """-> (code [256], len [256]) of Annex C; len 0: no code"""
    code, ln = [0] * 256, [0] * 256
    c, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code[huffval[k]], ln[huffval[k]] = c, l
            c += 1
            k += 1
        c <<= 1
    return code, ln


def fibonacci_counts(n):
    """1, 2, 3, 5, 8, ... on symbols 0 .. n-1: beside the reserved symbol's 1 every merge takes the running tree and the next
    symbol, so the depths reach n."""
    f = [1, 2]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    out = np.zeros(256, dtype=np.int64)
    out[:n] = f[:n]
    return out


# ------------------------------------------------------------------------------------------------ reading a finished file
def file_tables(data):
    """The DHT segments of a file, in order -> list of (id byte, bits [16], huffval bytes, segment bytes with marker)."""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m, L = data[p + 1], struct.unpack(">H", data[p + 2:p + 4])[0]
        if m == 0xC4:
            seg = data[p + 4:p + 2 + L]
            assert sum(seg[1:17]) == len(seg) - 17, "one table per DHT segment"
            out.append((seg[0], list(seg[1:17]), bytes(seg[17:]), bytes(data[p:p + 2 + L])))
        p += 2 + L
        if m == 0xDA:
            return out


def file_histograms(data, hs, vs, W, H):
    """Decodes the scan of a baseline 3-component file with its own tables and counts the symbols -> int64 [4, 256] in DHT order
    (DC luma, AC luma, DC chroma, AC chroma).  Restart markers are followed; nothing but the symbols is kept."""
    tabs = {t[0]: t for t in file_tables(data)}
    dec = {}
    for tid, (_, bits, vals, _) in tabs.items():
        code, ln = canonical_codes(bits, vals)
        dec[tid] = {(ln[s], code[s]): s for s in range(256) if ln[s]}
    scan = data[sos_end(data):]
    raw, marks, i = bytearray(), [], 0                 # unstuffed bytes; bit positions where a marker was
    while i < len(scan):
        b = scan[i]
        if b == 0xFF:
            nxt = scan[i + 1]
            if nxt == 0:
                raw.append(0xFF)
            elif 0xD0 <= nxt <= 0xD7:
                marks.append(8 * len(raw))
            elif nxt == 0xD9:
                break
            i += 2
            continue
        raw.append(b)
        i += 1
    bitstr = "".join(f"{b:08b}" for b in raw)
    hist = np.zeros((4, 256), dtype=np.int64)
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    pos, mark_i = 0, 0
    dri = data.find(b"\xff\xdd\x00\x04", 0, sos_end(data))
    interval = struct.unpack(">H", data[dri + 4:dri + 6])[0] if dri >= 0 else 0

    def symbol(tid):
        nonlocal pos
        c, n = 0, 0
        while True:
            c = (c << 1) | int(bitstr[pos])
            pos += 1
            n += 1
            if (n, c) in dec[tid]:
                return dec[tid][(n, c)]
            assert n < 16

    for m in range(mcus):
        if interval and m and m % interval == 0:
            assert marks[mark_i] - 8 < pos <= marks[mark_i]
            pos = marks[mark_i]                        # the padding in front of a marker
            mark_i += 1
        for comp in [0] * (hs * vs) + [1, 2]:
            t = 0 if comp == 0 else 1
            s = symbol(t)
            hist[2 * t, s] += 1
            pos += s
            k = 1
            while k < 64:
                rs = symbol(0x10 | t)
                hist[2 * t + 1, rs] += 1
                if rs == 0:
                    break
                if rs == 0xF0:
                    k += 16
                    continue
                k += (rs >> 4) + 1
                pos += rs & 15
    return hist


# ------------------------------------------------------------------------------------------------ pictures
@functools.lru_cache(maxsize=None)
def flat_picture(H, W):
    """mid-gray: every DC difference and every AC coefficient is 0, so each of the four tables holds one symbol"""
    a = np.full((H, W, 3), 128, dtype=np.uint8)
    a.setflags(write=False)
    return a


def batch_of(H, W, s, n=3):
    """n different pictures of one geometry: noise, smooth, noise mirrored, ..."""
    base = [rst_picture("noise", H, W, s), rst_picture("smooth", H, W, s)]
    return np.stack([np.ascontiguousarray(base[i % 2] if i < 2 else np.roll(base[i % 2][::-1], i, axis=1)) for i in range(n)])


def _basis_block(zz, amp):
    """8 x 8 samples around 128 that hold the AC basis function at zigzag position zz with this amplitude"""
    u, v = divmod(ZIGZAG[zz], 8)                       # natural index = row (vertical frequency) * 8 + column
    y, x = np.mgrid[0:8, 0:8]
    b = np.cos((2 * y + 1) * u * np.pi / 16) * np.cos((2 * x + 1) * v * np.pi / 16)
    return np.clip(np.round(128 + amp * b / np.abs(b).max() / 2), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def deep_table_picture(types):
    """A gray picture of 8 x 8 blocks, each one AC basis function: block type i sits at zigzag position (i mod 15) + 1 with amplitude
    40 for the first 15 types and 220 for the rest, and appears F(i) times, F = 1, 2, 3, 5, ...; 64 blocks to a row.  At quality 80,
    4:4:4, its AC-luma symbol counts force code sizes above 16."""
    counts = [int(v) for v in fibonacci_counts(types)[:types]]
    blocks = [_basis_block(i % 15 + 1, 40 if i < 15 else 220) for i in range(types) for _ in range(counts[i])]
    rows = -(-len(blocks) // 64)
    img = np.full((rows * 8, 64 * 8), 128, dtype=np.uint8)
    for k, b in enumerate(blocks):
        r, c = divmod(k, 64)
        img[r * 8:r * 8 + 8, c * 8:c * 8 + 8] = b
    a = np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2))
    a.setflags(write=False)
    return a
