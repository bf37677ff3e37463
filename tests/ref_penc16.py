"""Plain restatement of the PNG re-encoder's format for 16-bit samples (context
option "penc16"), for tests: written from the PNG specification and the
format notes in DESIGN.md "PNG re-encode", not from the kernel or its header.

What differs from the 8-bit format (tests/ref_penc.py, tests/ref_penc_dyn.py):

  * IHDR: bit depth 16; colour type 0 / 4 / 2 / 6 for 1 / 2 / 3 / 4 samples
    per pixel (an LA image stays colour type 4: no gray-over-LA quirk)
  * every sample goes into its row high byte first (PNG spec 7.2)
  * the five filters run over those bytes with bpp = 2 x samples per pixel

From the filtered stream on nothing differs, so the pieces come from the
8-bit restatements: ref_penc.filter_rows treats its last axis as bytes per
pixel, ref_penc.deflate_fixed and ref_penc_dyn.deflate take any stream.

read() is a small reader that shares nothing with them: chunk walk with CRC
check, zlib, a per-row unfilter, big-endian to uint16.  (PIL reads gray16 as
I;16 exactly but converts the other 16-bit colour types to 8 bits.)

A helper module (no fixtures).
"""
import binascii
import struct
import zlib
from collections import namedtuple

import numpy as np

import ref_penc
import ref_penc_dyn

COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
SPP = {v: k for k, v in COLOUR_TYPE.items()}

Ref16 = namedtuple("Ref16", "file filters stream dyn")
Ref16.__doc__ = """encode()'s result: the PNG file, the filter type of every row, the filtered stream
(flat, H x (1 + 2 * W * spp) bytes) and whether the DEFLATE block is a dynamic one."""


def be_rows(px):
    """H x W x (2 * spp) uint8: the row bytes of a uint16 array H x W x spp, high byte first."""
    px = np.ascontiguousarray(px, np.uint16)
    if px.ndim == 2:
        px = px[:, :, None]
    h, w, spp = px.shape
    out = np.empty((h, w, spp, 2), np.uint8)
    out[..., 0] = px >> 8
    out[..., 1] = px & 0xFF
    return out.reshape(h, w, 2 * spp)


def encode(px, dynamic=False):
    """The bit-depth-16 PNG file of an H x W x spp uint16 array (spp = 1..4): a Ref16.
    dynamic: the format under option "penc_dynamic" (the shorter of the fixed and the per-image block)."""
    rows = be_rows(px)
    h, w, bpp = rows.shape
    types, filtered = ref_penc.filter_rows(rows)
    stream = filtered.reshape(-1)
    if dynamic:
        out = ref_penc_dyn.deflate(stream)
        body, dyn = out[0], out[1]
    else:
        body, dyn = ref_penc.deflate_fixed(stream)[0], False
    z = b"\x78\x01" + body + struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", w, h, 16, COLOUR_TYPE[bpp // 2], 0, 0, 0)
    ch = ref_penc._chunk
    data = b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", ihdr) + ch(b"IDAT", z) + ch(b"IEND", b"")
    return Ref16(data, types, stream, dyn)


# ------------------------------------------------------------------ an independent reader

Png16 = namedtuple("Png16", "px colour_type filters stream")
Png16.__doc__ = """read()'s result: the samples (H x W x spp uint16), the IHDR colour type, the filter type of
every row and the filtered stream as inflated."""


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def read(png):
    """A non-interlaced bit-depth-16 PNG -> Png16.  Every chunk's CRC is checked; IHDR first, IEND last."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    pos, chunks = 8, []
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        t, body = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        assert len(body) == n and binascii.crc32(t + body) & 0xFFFFFFFF == crc, f"chunk {t!r}: CRC"
        chunks.append((t, body))
        pos += 12 + n
    assert pos == len(png), "bytes after the last chunk"
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b""), [t for t, _ in chunks]
    w, h, depth, ct, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, flt, lace) == (16, 0, 0, 0), (depth, comp, flt, lace)
    spp = SPP[ct]
    bpp, rb = 2 * spp, 2 * spp * w
    raw = zlib.decompress(b"".join(body for t, body in chunks if t == b"IDAT"))
    assert len(raw) == h * (rb + 1), (len(raw), h, rb)
    types, rows = [], []
    prev = [0] * rb
    for y in range(h):
        line = raw[y * (rb + 1):(y + 1) * (rb + 1)]
        f, cur = line[0], list(line[1:])
        assert f <= 4, f"row {y}: filter type {f}"
        for x in range(rb):
            a = cur[x - bpp] if x >= bpp else 0
            b = prev[x]
            c = prev[x - bpp] if x >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f]
            cur[x] = (cur[x] + pred) & 0xFF
        types.append(f)
        rows.append(cur)
        prev = cur
    by = np.asarray(rows, np.uint16).reshape(h, w, spp, 2)
    px = (by[..., 0] << 8) | by[..., 1]
    return Png16(px.astype(np.uint16), ct, np.asarray(types, np.uint8), np.frombuffer(raw, np.uint8))


def first_difference(got, exp):
    """Where a file parts from the reference's, for failure messages: the first differing row's filter
    type and stream position when both inflate, then the raw byte offset."""
    if got == exp:
        return "equal"
    off = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
    where = f"first differing file byte {off} (lengths {len(got)} against {len(exp)})"
    try:
        g, e = read(got), read(exp)
    except Exception as err:  # the file does not even read: say so and give the offset
        return f"unreadable ({type(err).__name__}: {err}); {where}"
    if g.px.shape != e.px.shape or g.colour_type != e.colour_type:
        return f"IHDR: {g.px.shape} type {g.colour_type} against {e.px.shape} type {e.colour_type}; {where}"
    if not np.array_equal(g.stream, e.stream):
        p = int(np.flatnonzero(g.stream != e.stream)[0])
        row_len = len(e.stream) // e.px.shape[0]
        y = p // row_len
        return (f"filtered stream differs from position {p}: row {y} byte {p % row_len - 1} (-1 = the filter byte), "
                f"filter type {int(g.filters[y])} against the reference's {int(e.filters[y])}; {where}")
    return f"same filtered stream; {ref_penc_dyn.explain_difference(got, exp)}; {where}"
