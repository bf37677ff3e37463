"""alph_craft.py: ALPH chunks and the files around them from explicit choices, for the
webp_alpha tests: the forward filter, the raw form, header-less VP8L streams written by
webp_craft (whose green channel is the filtered plane) and the container with any number
of ALPH chunks and any VP8X flags.  Builds on vp8_craft.extended / chunk.

  filtered(alpha, filt)              the plane g that unfilters to alpha
  header(comp, filt, pre=0)          the header byte
  raw(alpha, filt, pre=0, extra=0)   ALPH payload, raw
  lossless(alpha, filt, kind, pre=0) ALPH payload, VP8L-coded ("index", "transforms", "cache")
  file(vp8, w, h, payloads, ...)     the WebP file
  chunks(data), with_alph(data, payload), vp8_chunk(w, h, seed)
"""
import io

import numpy as np
from PIL import Image

import ref_alph as R
import ref_webp as RW
import vp8_craft as VC
import webp_cases as WK
import webp_craft as WC


def filtered(alpha, filt):
    a = np.asarray(alpha, np.uint8).astype(int)
    h, w = a.shape
    p = np.zeros_like(a)
    if filt != R.NONE:
        p[0, 1:] = a[0, :-1]
        p[1:, 0] = a[:-1, 0]
        L, T, TL = a[1:, :-1], a[:-1, 1:], a[:-1, :-1]
        p[1:, 1:] = L if filt == R.HORIZONTAL else T if filt == R.VERTICAL else np.clip(L + T - TL, 0, 255)
    return ((a - p) & 255).astype(np.uint8)


def header(comp, filt, pre=0):
    return comp | (filt << 2) | (pre << 4)


def raw(alpha, filt, pre=0, extra=0):
    return bytes([header(R.RAW, filt, pre)]) + filtered(alpha, filt).tobytes() + b"\xee" * extra


def stream(g, kind):
    """A header-less VP8L stream whose green channel is the plane g (h x w).
    index:      colour indexing with packed pixels and backward references, what libwebp writes for few
                alpha levels (the plane may hold at most 16 values for pixels to be packed)
    transforms: predictor and subtract-green transforms; red and blue carry noise that the decoder drops
    cache:      a colour cache and backward references over the literal pixels"""
    g = np.asarray(g, np.uint8)
    h, w = g.shape
    px = [0xFF000000 | (int(v) << 8) for v in g.reshape(-1)]
    if kind == "index":
        table = sorted(set(px))
        res, xs, specs = WC.forward(px, w, h, [("index", table)])
        s = WK.Stream(xs)
        while len(s.px) < len(res):  # literals, and a backward reference where the packed pixels repeat
            i, run = len(s.px), 0
            while i and i + run < len(res) and res[i + run] == res[i + run - 1] and run < 70:
                run += 1
            if run >= 3:
                s.copy(run, dist=1)
            else:
                s.lit(res[i])
        assert s.px == res
        return WC.vp8l(w, h, transforms=specs, ops=s.ops)[5:]
    if kind == "transforms":
        rng = np.random.default_rng(w * 1000 + h)
        px = [p | (int(r) << 16) | int(b) for p, r, b in zip(px, rng.integers(0, 256, len(px)), rng.integers(0, 256, len(px)))]
        bw, bh = (w + 3) >> 2, (h + 3) >> 2
        res, xs, specs = WC.forward(px, w, h, [("green",), ("predictor", 2, [(3 * i + 1) % 14 for i in range(bw * bh)])])
        return WC.vp8l(w, h, transforms=specs, ops=WC.literals(res))[5:]
    assert kind == "cache"
    s = WK.Stream(w, 4)
    while len(s.px) < len(px):
        i = len(s.px)
        run = 0  # a copy from the pixel before, where the plane repeats
        while i and i + run < len(px) and px[i + run] == px[i + run - 1] and run < 40:
            run += 1
        if run >= 3:
            s.copy(run, dist=1)
        elif s.cache[RW.cache_slot(px[i], 4)] == px[i]:
            s.hit(px[i])
        else:
            s.lit(px[i])
    assert s.px == px
    return WC.vp8l(w, h, ops=s.ops, cache_bits=4)[5:]


def lossless(alpha, filt, kind, pre=0):
    return bytes([header(R.VP8L, filt, pre)]) + stream(filtered(alpha, filt), kind)


def file(vp8, w, h, payloads, flags=0x10, before=(), after=()):
    """VP8X with `flags`, one ALPH chunk per payload, then the VP8 chunk."""
    return VC.extended(vp8, w, h, flags=flags, before=list(before) + [VC.chunk(b"ALPH", p) for p in payloads], after=after)


def chunks(data):
    """[(fourcc, payload)] of a file."""
    out, pos = [], 12
    while pos + 8 <= len(data):
        n = int.from_bytes(data[pos + 4:pos + 8], "little")
        out.append((data[pos:pos + 4], data[pos + 8:pos + 8 + n]))
        pos += 8 + n + (n & 1)
    return out


def alph_of(data):
    return dict(chunks(data))[b"ALPH"]


def with_alph(data, payload):
    """The file with its ALPH chunk's payload replaced (a cut one, for instance)."""
    return VC.riff([VC.chunk(cc, payload if cc == b"ALPH" else body) for cc, body in chunks(data)])


def without_alph(data):
    """The same VP8 chunk as a file of its own: what webp_lossy alone decodes."""
    return VC.simple(dict(chunks(data))[b"VP8 "])


def photo(seed, h, w):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(x / 7.0 + y / 11.0), 128 + 90 * np.cos(x / 5.0 - y / 9.0), 100 + 80 * np.sin(y / 3.0)], -1)
    return np.clip(a + rng.normal(0, 10, a.shape), 0, 255).astype(np.uint8)


def save(rgba, **kw):
    b = io.BytesIO()
    Image.fromarray(rgba, "RGBA" if rgba.shape[2] == 4 else "RGB").save(b, "WEBP", **kw)
    return b.getvalue()


def vp8_chunk(w, h, seed=7):
    """The VP8 chunk Pillow writes for a seeded photo of this size."""
    return dict(chunks(save(photo(seed, h, w), quality=60, method=2)))[b"VP8 "]
