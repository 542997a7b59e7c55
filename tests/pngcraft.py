"""PNG files built by hand for the PNG-reader tests: any per-row filter
schedule, any IDAT split, ancillary chunks in front, and the knobs to build
the malformed files the reader must refuse.

Forward filtering (PNG spec section 9) uses only ORIGINAL pixels -- filtered =
x - predictor(a, b, c) mod 256 with a, b, c the left, upper and upper-left
original bytes of the same channel, 0 outside the image -- so it vectorises in
numpy; zlib and struct are stdlib.  tests/test_png_cpu.py pins the
construction to Pillow.

Plain helper module, imported like rrpath and parity: no fixtures, no pytest
settings.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}          # channels -> PNG colour type
# all 25 (previous, current) filter pairs in 26 rows
CYCLE = (0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 0, 2, 4, 1, 3, 0, 3, 1, 4, 2, 0, 4, 3, 2, 1, 0)


def chunk(ctype, data=b"", crc=None):
    """one chunk; ``crc`` overrides the computed CRC"""
    body = ctype + data
    c = zlib.crc32(body) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(data)) + body + struct.pack(">I", c)


def ihdr(w, h, depth=8, colour=2, compression=0, filt=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, compression, filt, interlace))


def cycle_filters(h, start=0):
    return [CYCLE[(start + y) % len(CYCLE)] for y in range(h)]


def filter_stream(img, filters):
    """[h, w, c] uint8 + one filter type per row -> the filtered scanlines
    (h rows of 1 + w c bytes) as bytes"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w, c = img.shape
    assert len(filters) == h
    x = img.astype(np.int32)
    a = np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, 1:] = x[:-1, :-1]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, paeth])          # [5, h, w, c]
    f = np.asarray(filters, dtype=np.int64)
    assert ((f >= 0) & (f <= 4)).all()
    res = ((x - pred[f, np.arange(h)]) & 255).astype(np.uint8).reshape(h, w * c)
    rows = np.empty((h, 1 + w * c), dtype=np.uint8)
    rows[:, 0] = f
    rows[:, 1:] = res
    return rows.tobytes()


def assemble(w, h, colour, zdata, splits=(), ancillary=(), depth=8, interlace=0, iend=True):
    """signature + IHDR + ancillary chunks + IDAT chunk(s) + IEND.  ``splits``:
    byte positions at which the zlib stream is cut into separate IDAT chunks;
    ``ancillary``: (type, data) pairs placed in front of the first IDAT."""
    out = [SIGNATURE, ihdr(w, h, depth, colour, interlace=interlace)]
    out += [chunk(t, d) for t, d in ancillary]
    cuts = [0] + sorted(s for s in set(splits) if 0 < s < len(zdata)) + [len(zdata)]
    out += [chunk(b"IDAT", zdata[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    if iend:
        out.append(chunk(b"IEND"))
    return b"".join(out)


def make(img, filters=None, splits=(), ancillary=(), level=6):
    """[h, w, c] uint8 (c = 1, 2, 3, 4) -> (PNG bytes, filtered stream)"""
    img = np.asarray(img, dtype=np.uint8)
    h, w, c = img.shape
    stream = filter_stream(img, cycle_filters(h) if filters is None else filters)
    return assemble(w, h, COLOUR_TYPE[c], zlib.compress(stream, level), splits, ancillary), stream


def to_rgb(img):
    """what Image.open(p).convert('RGB') gives for the file of ``img``: grey
    replicated, alpha dropped"""
    img = np.asarray(img, dtype=np.uint8)
    c = img.shape[2]
    if c <= 2:
        return np.repeat(img[:, :, :1], 3, axis=2)
    return np.ascontiguousarray(img[:, :, :3])


EDGE_VALUES = np.array([0, 1, 2, 127, 128, 254, 255], dtype=np.uint8)


def pixels(h, w, c, seed, edge=False):
    """uniform random bytes, or (``edge``) draws from EDGE_VALUES: Paeth ties
    and 9-bit Average sums"""
    rng = np.random.default_rng(seed)
    if edge:
        return EDGE_VALUES[rng.integers(0, len(EDGE_VALUES), (h, w, c))]
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def smooth(h, w, c, seed, k=5):
    """box-blurred noise: neighbouring pixels correlate, so an adaptive writer
    picks Sub / Up / Average / Paeth rows"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (h + k - 1, w + k - 1, c)).astype(np.float64)
    s = np.cumsum(np.cumsum(np.pad(x, ((1, 0), (1, 0), (0, 0))), 0), 1)
    box = s[k:, k:] - s[:-k, k:] - s[k:, :-k] + s[:-k, :-k]
    return np.clip(np.rint(box / (k * k)), 0, 255).astype(np.uint8)


def filter_bytes(png):
    """the per-row filter types of a (well-formed, 8-bit, non-interlaced) PNG"""
    pos, idat, w = 8, b"", None
    while pos < len(png):
        n, t = struct.unpack(">I4s", png[pos:pos + 8])
        data = png[pos + 8:pos + 8 + n]
        if t == b"IHDR":
            w, h, _, colour = struct.unpack(">IIBB", data[:10])
            c = {0: 1, 4: 2, 2: 3, 6: 4}[colour]
        elif t == b"IDAT":
            idat += data
        pos += 12 + n
    raw = zlib.decompress(idat)
    return [raw[y * (1 + w * c)] for y in range(h)]
