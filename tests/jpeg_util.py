"""Helpers of the JPEG front-end tests: test pictures, Pillow-side encode / decode, and small writers for the containers.

Every JPEG is made at test time by Pillow's encoder (libjpeg-turbo); nothing binary is committed.
"""
import functools
import io
import struct

import numpy as np

SUBSAMPLING = {"420": 2, "422": 1, "444": 0, "gray": None}      # Pillow's subsampling= values
# the matrix both the CPU and the GPU tests walk
SIZES = [(360, 640), (97, 301), (8, 8), (17, 33), (1080, 1920)]
SAMPLINGS = ["420", "422", "444", "gray"]
QUALITIES = [30, 75, 95, 100]
TABLES = ["default", "optimize", "restart"]


def turbo():
    """True when Pillow decodes through libjpeg-turbo, the decoder the byte-equality is defined against."""
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


@functools.lru_cache(maxsize=4)
def _synthetic_full(frame):
    from tstar_amd.video import synthetic_frames_numpy
    return synthetic_frames_numpy([frame], 16, 1080, 1920, seed=5)[0]


def synthetic_picture(H, W, frame=3):
    """A crop of a 1080x1920 frame of the project's synthetic video (smooth gradients + planted rectangles)."""
    return np.ascontiguousarray(_synthetic_full(frame)[:H, :W])


def noise_picture(H, W, seed=0):
    """Uniform noise: the worst case for the range limit after the inverse DCT."""
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


def encode(rgb, sampling="420", quality=75, tables="default", progressive=False):
    """uint8 [H,W,3] -> JPEG bytes.  tables: "default" (Annex K Huffman tables), "optimize" (per-image tables) or "restart"
    (default tables + a restart marker every 3 MCUs)."""
    from PIL import Image, ImageFile
    im = Image.fromarray(rgb)
    kw = dict(quality=quality)
    if sampling == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = SUBSAMPLING[sampling]
    if tables == "optimize":
        kw["optimize"] = True
    elif tables == "restart":
        kw["restart_marker_blocks"] = 3
    if progressive:
        kw["progressive"] = True
    buf = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 4 * rgb.size)      # Pillow's encoder cannot grow its buffer mid-scan (noise at quality 100)
    try:
        im.save(buf, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


def matrix_files(H, W, sampling, quality):
    """[(label, jpeg bytes)] of one matrix cell: {synthetic, noise} x {default tables, optimised tables, restart interval}."""
    out = []
    for kind, pic in (("synthetic", synthetic_picture(H, W)), ("noise", noise_picture(H, W, seed=H + W + quality))):
        for tables in TABLES:
            out.append((f"{kind}/{tables}", encode(pic, sampling, quality, tables)))
    return out


def pillow_rgb(data):
    """The yardstick: what Pillow (libjpeg-turbo) decodes."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def segments(data):
    """[(marker, start, end)] of the marker segments before the entropy data, and the offset where that data starts."""
    out, p = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[p] == 0xFF, p
        m = data[p + 1]
        L = struct.unpack(">H", data[p + 2:p + 4])[0]
        out.append((m, p, p + 2 + L))
        p += 2 + L
        if m == 0xDA:
            return out, p


def strip_dht(data):
    """The same JPEG without its DHT segments (what AVI MJPG frames commonly look like)."""
    segs, _ = segments(data)
    out = bytearray(data)
    for m, a, b in reversed(segs):
        if m == 0xC4:
            del out[a:b]
    assert len(out) < len(data)
    return bytes(out)


def write_mjpeg(path, frames, pad=0):
    """Concatenated JPEGs; ``pad`` zero bytes between frames."""
    with open(path, "wb") as f:
        for fr in frames:
            f.write(fr)
            f.write(b"\x00" * pad)


def write_avi(path, frames, width, height, rate=30, scale=1, index=True, fourcc=b"MJPG", audio=False, absolute_index=False,
              avix=False):
    """A minimal AVI 1.0 file: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh, strf } ... }, LIST movi { NNdc ... }, idx1 }.

    Written from the RIFF / AVI layout as Microsoft's "AVI RIFF File Reference" describes it, independently of the reader
    in tstar_amd.jpeg (nothing is shared: no offset tables, no helper).  No third-party muxer is available where these
    tests run, so the AVI reader is pinned only against OUR OWN reading of that layout, not against files from ffmpeg or a
    camera.  ``audio`` puts an audio stream FIRST (the video chunks are then '01dc') with one '00wb' chunk per frame;
    ``absolute_index`` writes idx1 offsets from the start of the file instead of from the 'movi' fourcc; ``avix`` appends
    an (empty) OpenDML extension segment."""
    def chunk(cid, payload):
        return cid + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")

    def lst(kind, *parts):
        body = kind + b"".join(parts)
        return b"LIST" + struct.pack("<I", len(body)) + body

    n = len(frames)
    vid = b"01dc" if audio else b"00dc"
    avih = struct.pack("<10I16x", int(round(1e6 * scale / rate)), 0, 0, 0x10 if index else 0, n, 0, 2 if audio else 1,
                       max(len(f) for f in frames), width, height)
    v_strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", fourcc, 0, 0, 0, 0, scale, rate, 0, n, 0, 0xFFFFFFFF, 0, 0, 0, width, height)
    v_strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, fourcc, width * height * 3, 0, 0, 0, 0)
    strls = [lst(b"strl", chunk(b"strh", v_strh), chunk(b"strf", v_strf))]
    if audio:
        a_strh = struct.pack("<4s4sIHHIIIIIIII4h", b"auds", b"\x00\x00\x00\x00", 0, 0, 0, 0, 1, 8000, 0, n * 16, 0, 0xFFFFFFFF, 1, 0, 0, 0, 0)
        a_strf = struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)
        strls.insert(0, lst(b"strl", chunk(b"strh", a_strh), chunk(b"strf", a_strf)))
    hdrl = lst(b"hdrl", chunk(b"avih", avih), *strls)
    movi_parts, entries, pos = [], [], 4            # pos: offset from the 'movi' fourcc
    for fr in frames:
        if audio:
            c = chunk(b"00wb", b"\x80" * 16)
            entries.append((b"00wb", pos, 16))
            movi_parts.append(c)
            pos += len(c)
        c = chunk(vid, fr)
        entries.append((vid, pos, len(fr)))
        movi_parts.append(c)
        pos += len(c)
    movi = lst(b"movi", *movi_parts)
    movi_fourcc_at = 12 + len(hdrl) + 8             # RIFF header (12) + hdrl + 'LIST' + size
    body = b"AVI " + hdrl + movi
    if index:
        base = movi_fourcc_at if absolute_index else 0
        body += chunk(b"idx1", b"".join(struct.pack("<4sIII", cid, 0x10, base + off, size) for cid, off, size in entries))
    out = b"RIFF" + struct.pack("<I", len(body)) + body
    if avix:
        ext = b"AVIX" + lst(b"movi")
        out += b"RIFF" + struct.pack("<I", len(ext)) + ext
    with open(path, "wb") as f:
        f.write(out)
