"""alph_cases.py — the lossy WebP files with alpha of the webp_alpha tests: Pillow-made ones,
crafted ones (alph_craft.py) for every pair of compression and filter at the sizes where the
kernels can go wrong, and the refusals with their status and text.  Everything is seeded.

pillow_cases() / crafted_cases() -> [(label, bytes)], all of which decode;
refusals() -> [(label, bytes, "UNSUPPORTED" | "CORRUPT", text, stream, pillow)]: stream True when
the file passes planning and the alpha stream's decode meets the fault; pillow is what Pillow
does with the file: "refuses" or "RGBA".
plain_cases() -> [(label, bytes)]: files that are not this option's and decode to Rgb8 as before.
"""
import functools

import numpy as np

import alph_craft as A
import ref_alph as R

# The smallest shapes at which the kernels can still go wrong: one pixel, one column, one row, the 64-row
# strip edge of the gradient walk (heights 63, 64, 65, 129), the wave edges of the row and column items
# (widths 63, 64, 65, 257), odd sizes for the fancy upsampling beside a fourth channel.
SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (17, 33), (63, 64), (64, 63), (65, 65), (257, 5), (5, 129), (257, 129)]
LOSSLESS_SIZES = [(1, 1), (17, 33), (65, 65), (257, 5), (5, 129)]


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def binary(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return (((x // 7 + y // 5) % 2) * 255).astype(np.uint8)


def hgrad(h, w):
    return np.tile((np.arange(w) * 4).astype(np.uint8), (h, 1))


def blob(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return (128 + 100 * np.sin(x / 5.0) * np.cos(y / 7.0)).astype(np.uint8)


def levels(seed, h, w, n=3):
    """A plane of n levels in runs, so that every filter's output keeps few values."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    pick = np.array([0, 255, 128, 64][:n], np.uint8)
    return pick[((x // 3 + y // 2 + rng.integers(0, 2, (h, w)) * (x % 5 == 0)) % n)]


@functools.lru_cache(None)
def pillow_cases():
    """Written by Pillow at 64x48, quality 75; the header byte each gives is part of the case."""
    h, w = 48, 64
    rgb = A.photo(3, h, w)
    out = []

    def add(label, alpha, hdr, **kw):
        data = A.save(np.dstack([rgb, alpha]), quality=75, **kw)
        assert A.alph_of(data)[0] == hdr, (label, A.alph_of(data)[0])
        out.append((label, data))

    add("noise", noise(1, h, w), 0)                                # raw, no filter
    add("noise_m0", noise(2, h, w), 0, method=0)
    add("binary_aq100", binary(h, w), 1, alpha_quality=100)        # VP8L, no filter
    add("hgrad_m0", hgrad(h, w), 5, method=0)                      # VP8L, horizontal filter
    add("hgrad_m6", hgrad(h, w), 5, method=6)
    add("blob_aq50", blob(h, w), 17, alpha_quality=50)             # VP8L with the pre-processing bit
    add("blob_aq0", blob(h, w), 17, alpha_quality=0)
    add("blob", blob(h, w), 9)                                     # VP8L, vertical filter, a predictor transform
    return out


@functools.lru_cache(None)
def crafted_cases():
    out = []
    for w, h in SIZES:
        vp8 = A.vp8_chunk(w, h)
        for filt in range(4):
            out.append(("raw_f%d_%dx%d" % (filt, w, h), A.file(vp8, w, h, [A.raw(noise(10 + filt, h, w), filt)])))
    vp8 = A.vp8_chunk(17, 33)
    for filt in range(4):
        out.append(("raw_f%d_pre1_17x33" % filt, A.file(vp8, 17, 33, [A.raw(noise(20 + filt, 33, 17), filt, pre=1)])))
    out.append(("raw_3_extra_bytes", A.file(vp8, 17, 33, [A.raw(noise(24, 33, 17), R.GRADIENT, extra=3)])))
    for w, h in LOSSLESS_SIZES:
        vp8 = A.vp8_chunk(w, h)
        for filt in range(4):
            for kind, alpha in (("index", levels(30 + filt, h, w, 2)), ("transforms", noise(40 + filt, h, w)),
                                ("cache", levels(50 + filt, h, w, 3))):
                out.append(("vp8l_%s_f%d_%dx%d" % (kind, filt, w, h), A.file(vp8, w, h, [A.lossless(alpha, filt, kind)])))
    vp8 = A.vp8_chunk(257, 129)
    out.append(("vp8l_index_f3_257x129", A.file(vp8, 257, 129, [A.lossless(levels(60, 129, 257, 2), R.GRADIENT, "index")])))
    out.append(("vp8l_cache_f1_pre1_257x129", A.file(vp8, 257, 129, [A.lossless(levels(61, 129, 257, 3), R.HORIZONTAL, "cache", pre=1)])))
    # chunks the walk skips on its way, and an ALPH chunk of odd length (its pad byte)
    vp8 = A.vp8_chunk(5, 1)
    out.append(("chunks_around", A.file(vp8, 5, 1, [A.raw(noise(70, 1, 5), R.VERTICAL)], flags=0x3c,
                                        before=[A.VC.chunk(b"ICCP", b"icc"), A.VC.chunk(b"ABCD", b"xyz")],
                                        after=[A.VC.chunk(b"EXIF", b"exif!")])))
    return out


@functools.lru_cache(None)
def plain_cases():
    """Not this option's: no ALPH chunk before the image chunk.  Rgb8 exactly as with webp_lossy alone."""
    vp8 = A.vp8_chunk(17, 33)
    return [("flag_without_chunk", A.file(vp8, 17, 33, [])),
            ("alph_after_the_image", A.VC.extended(vp8, 17, 33, flags=0x10, after=[A.VC.chunk(b"ALPH", A.raw(noise(80, 33, 17), 0))])),
            ("simple_file", A.VC.simple(vp8))]


def cut_stream(data, k):
    """The file with the last k bytes of its ALPH payload gone."""
    p = A.alph_of(data)
    return A.with_alph(data, p[:len(p) - k])


@functools.lru_cache(None)
def refusals():
    w, h = 17, 33
    vp8 = A.vp8_chunk(w, h)
    a = noise(90, h, w)
    good = A.raw(a, R.HORIZONTAL)
    U, X = "UNSUPPORTED", "CORRUPT"
    out = []
    for hdr in (2, 3, 64, 128, 0x42, 0xc1, 0x20, 0x35):  # compression 2, 3; reserved bits; pre-processing 2, 3
        out.append(("header byte %d" % hdr, A.file(vp8, w, h, [bytes([hdr]) + good[1:]]), X, R.E_HEADER, False, "refuses"))
    out.append(("raw plane one byte short", A.file(vp8, w, h, [good[:-1]]), X, R.E_RAW, False, "refuses"))
    out.append(("raw plane of one row", A.file(vp8, w, h, [good[:1 + w]]), X, R.E_RAW, False, "refuses"))
    out.append(("chunk of no bytes", A.file(vp8, w, h, [b""]), X, R.E_SHORT_CHUNK, False, "refuses"))
    out.append(("chunk of one byte", A.file(vp8, w, h, [b"\0"]), X, R.E_SHORT_CHUNK, False, "refuses"))
    out.append(("chunk of one byte, lossless", A.file(vp8, w, h, [b"\1"]), X, R.E_SHORT_CHUNK, False, "refuses"))
    out.append(("two chunks", A.file(vp8, w, h, [good, good]), U, R.E_TWO, False, "refuses"))
    out.append(("flag clear", A.file(vp8, w, h, [good], flags=0), U, R.E_FLAG, False, "RGBA"))
    pil = dict(pillow_cases())
    out.append(("pillow stream cut by 4", cut_stream(pil["blob_aq50"], 4), X, R.E_STREAM, True, "refuses"))
    out.append(("pillow stream cut to half", cut_stream(pil["blob"], len(A.alph_of(pil["blob"])) // 2), X, R.E_STREAM, True, "refuses"))
    craft = dict(crafted_cases())
    out.append(("crafted stream cut by 9", cut_stream(craft["vp8l_transforms_f2_17x33"], 9), X, R.E_STREAM, True, "refuses"))
    out.append(("stream of one byte", A.file(vp8, w, h, [b"\x05\xff"]), X, R.E_STREAM, True, "refuses"))
    # the subtract-green transform twice: bits 1, 01, 1, 01 from the least significant
    out.append(("stream with a transform twice", A.file(vp8, w, h, [b"\x01\x2d" + bytes(30)]), X, R.E_STREAM, True, "refuses"))
    return out
