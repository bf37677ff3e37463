"""vp8_cases.py — the lossy WebP files of the webp_lossy tests: Pillow-made ones, crafted
ones (vp8_craft.py) for what Pillow never writes, and the refusals with their status
and text.  Everything is seeded, so every process sees the same bytes.

pillow_cases() / crafted_cases() -> [(label, bytes)], all of which decode;
refusals() -> [(label, bytes, "UNSUPPORTED" | "CORRUPT", text, stream)]: stream True when
the file passes planning and k_vp8_parse meets the fault.
"""
import functools
import io

import numpy as np
from PIL import Image

import ref_vp8 as R
import vp8_craft as C


def _photo(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(x / 7.0 + y / 11.0), 128 + 90 * np.cos(x / 5.0 - y / 9.0), 100 + 80 * np.sin(y / 3.0)], -1)
    return np.clip(a + rng.normal(0, 10, a.shape), 0, 255).astype(np.uint8)


def _edges(rng, h, w):
    a = np.zeros((h, w, 3), np.uint8)
    a[:, :] = (250, 250, 250)
    a[h // 5:h // 2, w // 6:w // 2] = (10, 20, 200)
    a[h // 2:, w // 3:] = (220, 10, 30)
    a[::7, :] = (0, 0, 0)
    return a


def _images(rng, h, w):
    return [("photo", _photo(rng, h, w)), ("noise", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
            ("solid", np.full((h, w, 3), (40, 170, 90), np.uint8)),
            ("gray", np.repeat(_photo(rng, h, w)[..., :1], 3, -1)), ("edges", _edges(rng, h, w))]


def save(a, q, m):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "WEBP", quality=q, method=m)
    return b.getvalue()


@functools.lru_cache(None)
def pillow_cases():
    rng = np.random.default_rng(8)
    out = []
    for name, a in _images(rng, 40, 48):
        for q in (0, 30, 75, 95, 100):
            for m in (0, 6):
                out.append(("%s_48x40_q%d_m%d" % (name, q, m), save(a, q, m)))
    for w, h in ((1, 1), (16, 16), (17, 33), (33, 17), (40, 36), (130, 100)):
        out.append(("photo_%dx%d" % (w, h), save(_photo(rng, h, w), 75, 4)))
    out.append(("photo_24x280", save(_photo(rng, 280, 24), 60, 4)))  # MB rows and columns past the waves of a
    out.append(("photo_280x24", save(_photo(rng, 24, 280), 60, 4)))  # recon workgroup
    return out


# ------------------------------------------------------------ crafted

SMALL = [1] * 8 + [2, 2, 3, 4, 5, 6, 7, 8, 9, 10]
LARGE = [11, 18, 19, 34, 35, 66, 67, 300, 2114]


def block(rng, large=False, empty_p=0.25):
    lv = [0] * 16
    if rng.random() < empty_p:
        return lv
    last = int(rng.integers(0, 16))
    for i in range(last + 1):
        if i == last or rng.random() < 0.5:
            lv[i] = int(rng.choice(SMALL)) * (1 if rng.random() < 0.5 else -1)
    if large:  # one large value per block at most, so every intermediate of the transforms stays in 16 bits
        lv[int(rng.integers(0, last + 1))] = int(rng.choice(LARGE)) * (1 if rng.random() < 0.5 else -1)
    return lv


def rand_mbs(rng, mbw, mbh, ymode=None, bmode=None, uvmode=None, large=False, segs=1, skip_p=0.0):
    mbs = []
    for _ in range(mbw * mbh):
        ym = int(rng.integers(0, 5)) if ymode is None else ymode
        mb = dict(ymode=ym, uvmode=int(rng.integers(0, 4)) if uvmode is None else uvmode,
                  segment=int(rng.integers(0, segs)), skip=1 if rng.random() < skip_p else 0,
                  levels=[block(rng, large) for _ in range(25)])
        if ym == C.B_PRED:
            mb["bmodes"] = [int(rng.integers(0, 10)) if bmode is None else bmode for _ in range(16)]
        mbs.append(mb)
    return mbs


@functools.lru_cache(None)
def crafted_cases():
    rng = np.random.default_rng(80)
    out = []

    def add(label, w, h, wrap=C.simple, mbs=None, **hdr):
        mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
        mbs = rand_mbs(rng, mbw, mbh) if mbs is None else mbs
        out.append((label, wrap(C.frame(w, h, mbs, **hdr))))

    for n, rows in ((2, 3), (4, 5), (8, 9)):  # more MB rows than partitions
        add("parts%d_20x%d" % (n, 16 * rows - 3), 20, 16 * rows - 3, nparts=n, level=12)
    add("simple_filter", 48, 48, simple=1, level=20)
    add("simple_filter_sharp", 40, 33, simple=1, level=45, sharp=5)
    for s in (1, 4, 7):
        add("sharp%d" % s, 48, 48, level=30, sharp=s)
    add("lf_delta_plus_minus", 48, 48, level=20, lf=dict(update=True, ref=[5, None, 3, None], mode=[-7, 2, None, None]))
    add("lf_delta_minus_plus", 48, 48, level=20, lf=dict(update=True, ref=[-9, None, None, 1], mode=[12, None, None, None]))
    add("lf_delta_no_update", 32, 32, level=20, lf=dict(update=False))
    for lv in (1, 14, 15, 39, 40, 63):
        add("level%d" % lv, 48, 32, level=lv)
    add("level0", 48, 48, level=0)
    sq = dict(abs=0, q=[-10, 10, None, 5], f=[-5, 5, None, 20])
    add("seg_no_map", 48, 48, seg=dict(map=False, data=sq), level=20, base_q=50)
    add("seg_delta", 48, 48, mbs=rand_mbs(rng, 3, 3, segs=4), seg=dict(map=True, data=sq, probs=[120, None, 200]), level=20, base_q=50)
    add("seg_abs", 48, 48, mbs=rand_mbs(rng, 3, 3, segs=4),
        seg=dict(map=True, data=dict(abs=1, q=[10, 50, 90, 127], f=[0, 10, 40, 63]), probs=[128, 128, 128]), level=20)
    add("seg_abs_simple", 48, 48, mbs=rand_mbs(rng, 3, 3, segs=4), simple=1,
        seg=dict(map=True, data=dict(abs=1, q=[10, 50, 90, 127], f=[0, 10, 40, 63]), probs=[128, 128, 128]), level=20)
    add("seg_clip", 48, 48, mbs=rand_mbs(rng, 3, 3, segs=4), base_q=100, dq=(-15, 15, None, 15, -15),
        seg=dict(map=True, data=dict(abs=0, q=[60, -127, 20, -95], f=[60, -60, None, 0]), probs=[90, 100, 110]), level=30)
    add("seg_map_only", 48, 48, mbs=rand_mbs(rng, 3, 3, segs=4), seg=dict(map=True, data=None, probs=[None, 77, None]), level=9)
    add("no_skip_prob", 48, 48, skip_prob=None, level=10)
    add("skip_prob", 48, 48, mbs=rand_mbs(rng, 3, 3, skip_p=0.5), skip_prob=100, level=25)
    add("skip_all", 48, 48, mbs=rand_mbs(rng, 3, 3, skip_p=1.0), skip_prob=250, level=25)
    add("prob_updates", 48, 48, updates={int(i): int(v) for i, v in zip(rng.choice(1056, 60, replace=False), rng.integers(1, 256, 60))},
        level=10)
    for m in range(4):
        add("ymode%d_uvmode%d" % (m, m), 48, 48, mbs=rand_mbs(rng, 3, 3, ymode=m, uvmode=m), level=8, base_q=20)
    for b in range(10):
        add("bmode%d" % b, 48, 48, mbs=rand_mbs(rng, 3, 3, ymode=C.B_PRED, bmode=b), level=8, base_q=20)
    add("bpred_mixed", 64, 64, mbs=rand_mbs(rng, 4, 4, ymode=C.B_PRED), level=16, base_q=30)
    add("bpred_beside_16x16", 64, 48, mbs=[dict(m, ymode=(C.B_PRED if i % 2 else i % 4), bmodes=[int(v) for v in rng.integers(0, 10, 16)])
                                            for i, m in enumerate(rand_mbs(rng, 4, 3))], level=33)
    add("tokens_all_categories", 48, 48, mbs=rand_mbs(rng, 3, 3, large=True), base_q=0, level=5)
    add("dq_deltas", 33, 47, base_q=60, dq=(7, -8, 15, -15, 3), level=20)
    add("q127", 32, 32, base_q=127, level=63, sharp=3)
    add("colorspace_clamp", 32, 32, colorspace=1, clamp=1, level=10)
    for v in (1, 2, 3):
        add("version%d" % v, 32, 32, version=v, level=10)
    add("scale_bits", 32, 17, xscale=1, yscale=2, level=10)
    add("extended_iccp_exif_unknown", 35, 21, level=10,
        wrap=lambda p: C.extended(p, 35, 21, flags=0x2c, before=[C.chunk(b"ICCP", b"icc profile"), C.chunk(b"ABCD", b"xyz")],
                                  after=[C.chunk(b"EXIF", b"exif!"), C.chunk(b"XMP ", b"<x/>")]))
    add("extended_plain", 16, 16, level=0, wrap=lambda p: C.extended(p, 16, 16))
    add("tiny_1x1", 1, 1, level=20)
    add("wide_130x20", 130, 20, level=24, nparts=2)
    return out


def fitted_cut(data, n):
    """The first n bytes with the RIFF, chunk and (where it no longer fits) first-partition sizes made to fit."""
    h = R.parse(data)
    off = h["off"]
    assert h["status"] == R.OK and n >= off + 10
    cut = bytearray(data[:n])
    cut[4:8] = (n - 8).to_bytes(4, "little")
    cut[off - 4:off] = (n - off).to_bytes(4, "little")
    if h["part0"] > n - off - 10:
        tag = (int.from_bytes(cut[off:off + 3], "little") & 31) | ((n - off - 10) << 5)
        cut[off:off + 3] = tag.to_bytes(3, "little")
    return bytes(cut)


@functools.lru_cache(None)
def refusals():
    rng = np.random.default_rng(81)
    mbs = rand_mbs(rng, 2, 2)
    good = C.frame(32, 32, mbs, level=10)
    U, X = "UNSUPPORTED", "CORRUPT"
    out = [
        ("not a key frame", C.simple(C.frame(32, 32, mbs, key=0)), X, "WebP: VP8 frame is not a key frame", False),
        ("version 4", C.simple(C.frame(32, 32, mbs, version=4)), X, "WebP: VP8 version above 3", False),
        ("version 7", C.simple(C.frame(32, 32, mbs, version=7)), X, "WebP: VP8 version above 3", False),
        ("not shown", C.simple(C.frame(32, 32, mbs, show=0)), X, "WebP: VP8 frame is not shown", False),
        ("bad start code", C.simple(C.frame(32, 32, mbs, start=b"\x9d\x01\x2b")), X, "WebP: bad VP8 start code", False),
        ("first partition past the chunk", C.simple(C.frame(32, 32, mbs, part0_size=len(good))), X,
         "WebP: VP8 first partition reaches past the chunk", False),
        ("canvas differs", C.extended(good, 32, 33), X, "WebP: VP8X canvas size differs from the VP8 frame size", False),
        ("frame header cut", C.simple(good[:9]), X, "WebP: truncated VP8 frame header", False),
        ("alpha", C.extended(good, 32, 32, flags=0x10, before=[C.chunk(b"ALPH", b"\0" + bytes(32 * 32))]), U,
         "WebP: lossy WebP with alpha", False),
        ("animation flag", C.extended(good, 32, 32, flags=0x02), U, "WebP: animated WebP", False),
        ("animation chunks", C.extended(good, 32, 32, before=[C.chunk(b"ANIM", bytes(6)), C.chunk(b"ANMF", bytes(16))]), U,
         "WebP: animated WebP", False),
        ("chunk past the RIFF size", C.simple(good)[:-7], X, "WebP: truncated chunk", False),
        ("no image chunk", C.riff([C.chunk(b"VP8X", bytes([0] * 4) + (31).to_bytes(3, "little") * 2)]), X, "WebP: no image chunk", False),
    ]
    eight = C.simple(C.frame(32, 32, mbs, nparts=8, level=10))
    h = R.parse(eight)
    out.append(("partition table past the chunk", fitted_cut(eight, h["off"] + 10 + h["part0"] + 5), X, R.FAIL_PARTS, True))
    out.append(("tokens cut", fitted_cut(C.simple(good), len(C.simple(good)) - 40), X, R.FAIL_BITS, True))
    pil = dict(pillow_cases())["photo_40x36"]
    out.append(("pillow file cut", fitted_cut(pil, len(pil) * 2 // 3), X, R.FAIL_BITS, True))
    return out


@functools.lru_cache(None)
def lossless_file():
    b = io.BytesIO()
    Image.fromarray(_photo(np.random.default_rng(3), 20, 30)).save(b, "WEBP", lossless=True)
    return b.getvalue()
