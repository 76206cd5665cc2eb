"""What the CPU and the GPU tests of the compressed-resident JPEG store share: the frame mixes and an arena built from them."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as JU  # noqa: E402

# name -> (H, W, sampling, quality, tables, kind); kind: "mixed" alternates crops of the synthetic video with noise, "noise" is noise
# alone, "progressive" is "mixed" with frame PROGRESSIVE_AT coded progressively (a frame the device decoder does not cover)
MIXES = {f"{h}x{w}-{s}": (h, w, s, 75, "default", "mixed") for (h, w) in ((17, 33), (72, 128)) for s in ("420", "422", "444", "gray")}
MIXES["restart3"] = (72, 128, "420", 75, "restart", "mixed")             # a restart marker every 3 MCUs: many short segments
MIXES["long-noise"] = (96, 128, "444", 95, "default", "noise")           # one segment per frame, longer than TSTAR_JPEG_SPLIT_BYTES
MIXES["optimize"] = (72, 128, "420", 75, "optimize", "mixed")            # a table set per frame
MIXES["progressive"] = (72, 128, "420", 75, "default", "progressive")
PROGRESSIVE_AT = 2


@functools.lru_cache(maxsize=None)
def mix_frames(name, n):
    """n JPEG files of the mix (a tuple of bytes), all of one geometry."""
    H, W, sampling, quality, tables, kind = MIXES[name]
    out = []
    for i in range(n):
        noise = kind == "noise" or i % 2 == 1
        pic = JU.noise_picture(H, W, seed=1000 + i) if noise else JU.synthetic_picture(H, W, frame=i % 16)
        out.append(JU.encode(pic, sampling, quality, tables, progressive=(kind == "progressive" and i == PROGRESSIVE_AT)))
    return tuple(out)


def geometry(datas):
    """The geometry of the first frame the decoder covers."""
    from tstar_amd import jpeg
    for d in datas:
        rc, geom, _ = jpeg.probe(d)
        if rc == jpeg.OK:
            return geom
    raise AssertionError("no covered frame")


def build_arena(datas, geom, chunk=4, gap=0):
    """The arena of ``datas`` planned ``chunk`` frames at a time, as an open does (``gap`` bytes of filler in front of every chunk)
    -> (jpeg_resident.Arena with host bytes, route int32 [n])."""
    from tstar_amd import jpeg, jpeg_resident as JR
    b = JR.ArenaBuilder()
    parts, routes, at = [], [], 0
    for c0 in range(0, len(datas), chunk):
        part = list(datas[c0:c0 + chunk])
        plan = jpeg.plan_segments(part, geom)
        parts.append(b"\xEE" * gap + b"".join(part))
        b.add(plan, [len(d) for d in part], base=at + gap)
        at += len(parts[-1])
        routes.append(plan.route.copy())
    return b.finish(np.frombuffer(b"".join(parts), dtype=np.uint8)), np.concatenate(routes)


def crafted_arena(seed=0):
    """An arena of random bytes with made-up records: frames of 0 .. 20 000 bytes, one starting at every offset mod 16, so that a
    copy meets every head, tail and shift.  Nothing here decodes; the gather only moves and rebases."""
    from tstar_amd import jpeg, jpeg_resident as JR
    rs = np.random.RandomState(seed)
    lens = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 100, 1000, 4097, 16384, 20000, 5, 0]
    lens += [int(v) for v in rs.randint(1, 300, size=16)]
    chunks, off, at = [], [], 0
    for k, n in enumerate(lens):
        pad = (k - at) % 16                                           # frame k starts at k mod 16
        chunks.append(rs.randint(0, 256, size=pad + n).astype(np.uint8))
        off.append(at + pad)
        at += pad + n
    frames = np.zeros(len(lens), dtype=jpeg.FRAME_DTYPE)
    segs = []
    for e, n in enumerate(lens):
        ns = 0 if n == 0 else 1 + e % 3
        frames[e] = (e % 2, len(segs), ns, 0)
        segs += [(e, n * s // ns, n * (s + 1) // ns, 5 * s, 5, int(s == ns - 1)) for s in range(ns)]
    quant = rs.randint(1, 256, size=(len(lens), 192)).astype(np.uint16)
    return JR.Arena(np.asarray(off, dtype=np.uint64), np.asarray(lens, dtype=np.uint32), quant, frames,
                    np.array(segs, dtype=jpeg.SEGMENT_DTYPE), np.zeros((2, jpeg.TABLE_SET_BYTES), dtype=np.uint8), np.concatenate(chunks))


def host_coefficients(datas, geom):
    """The yardstick (tstar_jpeg_entropy_batch) -> (coef int16 [n, blocks * 64], quant uint16 [n, 192], status int32 [n])."""
    from tstar_amd import jpeg
    blocks = jpeg._sizes(geom)[0]
    coef = np.zeros((len(datas), blocks * 64), dtype=np.int16)
    quant = np.zeros((len(datas), 192), dtype=np.uint16)
    status, _ = jpeg.entropy_batch(list(datas), geom, coef, quant)
    return coef, quant, status


def shuffled_ids(ok_ids, seed, n=None):
    """A shuffled list over ``ok_ids`` in which every id occurs and some occur twice."""
    rs = np.random.RandomState(seed)
    ids = list(ok_ids) + [int(v) for v in rs.choice(ok_ids, size=max(2, len(ok_ids) // 2))]
    rs.shuffle(ids)
    return ids[:n] if n else ids
