"""webp_cases.py: the shared set of lossless WebP files of tests/test_webp_cpu.py and
tests/test_gpu_webp.py: Pillow-made files, files crafted bit by bit (webp_craft.py)
and refusals with the status and text the library answers."""
import functools
import io

import numpy as np
from PIL import Image

import ref_webp as R
import webp_craft as C

SETTINGS = [(m, q) for m in (0, 3, 6) for q in (0, 50, 100)]


def _save(a, method, quality):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "WEBP", lossless=True, exact=True, method=method, quality=quality)
    return b.getvalue()


def _photo(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x + y) * 255 // (w + h), x * 255 // w, y * 255 // h], -1)
    return (base + rng.integers(0, 6, (h, w, 3))).clip(0, 255).astype(np.uint8)


def _paletted(rng, n, h, w):
    pal = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    idx = rng.integers(0, n, (h, w))
    idx[h // 2:, :] = idx[:h - h // 2, :]  # repeats: backward references
    idx.flat[:n] = np.arange(n)
    return pal[idx]


def images():
    """name -> array; the kinds of the Pillow-made matrix (48 x 40 unless the kind needs more)."""
    rng = np.random.default_rng(2024)
    h, w = 40, 48
    out = {
        "noise_rgb": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
        "noise_rgba": rng.integers(0, 256, (h, w, 4), dtype=np.uint8),
        "photo": _photo(rng, h, w),
        "solid": np.full((h, w, 3), (12, 200, 77), np.uint8),
        "gray": np.repeat(_photo(rng, h, w)[..., :1], 3, axis=-1),
    }
    for n in (2, 3, 4, 16, 17, 200):
        out["pal%d" % n] = _paletted(rng, n, h, w)
    a = rng.integers(1, 256, (h, w, 4), dtype=np.uint8)
    a[5:20, 7:30, 3] = 0  # alpha 0 over non-zero RGB
    out["alpha0_rgb"] = a
    return out


SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 9), (33, 4), (129, 63), (130, 64), (127, 65), (200, 150)]


@functools.lru_cache(maxsize=None)
def pillow_cases():
    """[(name, bytes)]"""
    out = []
    for name, a in images().items():
        for m, q in SETTINGS:
            out.append(("%s_m%d_q%d" % (name, m, q), _save(a, m, q)))
    rng = np.random.default_rng(7)
    for i, (w, h) in enumerate(SIZES):
        m, q = SETTINGS[(2 * i + 3) % len(SETTINGS)]
        out.append(("photo_%dx%d_m%d_q%d" % (w, h, m, q), _save(_photo(rng, h, w), m, q)))
        if (w, h) in ((17, 9), (33, 4), (129, 63)):  # packed widths with a partial last packed pixel
            for n in (2, 4, 16):
                out.append(("pal%d_%dx%d" % (n, w, h), _save(_paletted(rng, n, h, w), 6, 100)))
    for (w, h), (m, q) in (((129, 63), (3, 0)), ((130, 64), (6, 100)), ((200, 150), (3, 0))):  # photo with a flat quarter: several groups
        a = _photo(rng, h, w)
        a[:h // 2, :w // 2] = _paletted(rng, 5, h // 2, w // 2)
        out.append(("mixed_%dx%d_m%d_q%d" % (w, h, m, q), _save(a, m, q)))
    out.append(("rgba_130x64", _save(np.concatenate([_photo(rng, 64, 130), rng.integers(0, 256, (64, 130, 1), dtype=np.uint8)], -1), 3, 50)))
    return out


# ------------------------------------------------------------ crafted

def _noise(n, seed, alpha=True):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return [int(p) | (0 if alpha else 0xFF000000) for p in v]


def _few(n, colours, seed):
    rng = np.random.default_rng(seed)
    pal = _noise(colours, seed + 1)
    return [pal[i] for i in rng.integers(0, colours, n)], pal


class Stream:
    """An op list with the colour cache modelled, so hits can be asked for by pixel."""

    def __init__(self, width, cache_bits=0):
        self.w, self.bits = width, cache_bits
        self.px, self.ops = [], []
        self.cache = [0] * (1 << cache_bits) if cache_bits else None

    def _ins(self, p):
        self.px.append(p)
        if self.cache is not None:
            self.cache[R.cache_slot(p, self.bits)] = p

    def lit(self, p):
        self.ops.append(("px", p))
        self._ins(p)

    def copy(self, length, dist=None, code=None):
        code = dist + 120 if code is None else code
        d = R.plane_distance(self.w, code)
        assert d <= len(self.px)
        self.ops.append(("copy", length, code))
        for _ in range(length):
            self._ins(self.px[-d])

    def hit(self, p):
        s = R.cache_slot(p, self.bits)
        assert self.cache[s] == p
        self.ops.append(("cache", s))
        self._ins(p)

    def fill(self, total, seed=1):
        for p in _noise(total - len(self.px), seed):
            self.lit(p)


def _file(w, h, alpha=1, **kw):
    return C.simple_file(C.vp8l(w, h, alpha, **kw))


def _transformed(px, w, h, transforms, alpha=1):
    res, xs, specs = C.forward(px, w, h, transforms)
    return _file(w, h, alpha, transforms=specs, ops=C.literals(res))


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """[(name, bytes)]: each decodes."""
    out = []
    px9 = _noise(81, 11)
    for mode in range(16):
        out.append(("predictor_mode%d" % mode, _transformed(px9, 9, 9, [("predictor", 2, [mode] * 9)])))
    out.append(("predictor_mixed_modes", _transformed(_noise(63 * 70, 12), 63, 70, [("predictor", 3, [i % 14 for i in range(8 * 9)])])))
    cm = [((3 * i + 1) & 255, (200 + 7 * i) & 255, (90 + 31 * i) & 255) for i in range(9)]
    # orders libwebp never writes
    out.append(("order_pred_color_green_index", _transformed(px9, 9, 9, [("predictor", 2, [5] * 9), ("color", 2, cm), ("green",), ("index", None)])))
    p4, pal4 = _few(17 * 9, 4, 13)
    out.append(("order_index_green_color_pred", _transformed(p4, 17, 9, [("index", pal4), ("green",), ("color", 2, cm[:6]), ("predictor", 2, [11, 12, 13, 10, 5, 7])])))
    p16, pal16 = _few(33 * 5, 16, 14)
    out.append(("order_green_index_pred_color", _transformed(p16, 33, 5, [("green",), ("index", None), ("predictor", 2, [12] * 10), ("color", 3, [cm[0], cm[1], cm[2]])])))
    out.append(("bits_pred2_color9", _transformed(px9, 9, 9, [("predictor", 2, [13] * 9), ("color", 9, cm[:1])])))
    out.append(("bits_pred9_color2", _transformed(px9, 9, 9, [("color", 2, cm), ("predictor", 9, [11])])))
    p2, pal2 = _few(33 * 4, 2, 15)
    out.append(("index_2colours_33x4", _transformed(p2, 33, 4, [("index", pal2)])))
    p3, pal3 = _few(17 * 9, 3, 16)
    out.append(("index_past_table", _transformed(p3, 17, 9, [("index", pal3)])))
    # an index past a 3-entry table (packed two bits per pixel: index 3 exists in the stream)
    res, xs, specs = C.forward(p3, 17, 9, [("index", pal3)])
    res[2] |= 0x0000FF00
    out.append(("index_past_table_used", _file(17, 9, 1, transforms=specs, ops=C.literals(res))))

    for bits in (1, 11):
        s = Stream(16, bits)
        ps = _noise(40, 20 + bits)
        for p in ps:
            s.lit(p)
        s.copy(24, dist=7)
        s.hit(s.px[-1])  # a hit right after a copy: the copy's last pixel
        if s.cache[R.cache_slot(s.px[-9], bits)] == s.px[-9]:
            s.hit(s.px[-9])
        s.fill(16 * 8, 3)
        out.append(("cache_bits%d" % bits, _file(16, 8, ops=s.ops, cache_bits=bits)))
    # a copy whose pixels collide in one slot: the last one stays
    s = Stream(16, 1)
    pool = _noise(400, 31)
    same = [p for p in pool if R.cache_slot(p, 1) == 0][:70]
    for p in same:
        s.lit(p)
    s.copy(70, dist=70)
    s.hit(same[-1])
    s.copy(3, dist=2)
    s.hit(s.px[-1])
    s.fill(16 * 10, 4)
    out.append(("cache_collide", _file(16, 10, ops=s.ops, cache_bits=1)))

    s = Stream(3)
    s.fill(32, 5)
    for code in range(1, 121):
        s.copy(1, code=code)
    s.fill(153, 6)
    out.append(("distance_codes_narrow", _file(3, 51, ops=s.ops)))
    s = Stream(40)
    s.fill(40 * 9, 7)
    for code in range(1, 121):
        s.copy(2, code=code)
    s.fill(40 * 16, 8)
    out.append(("distance_codes_wide", _file(40, 16, ops=s.ops)))

    w, h = 65, 317
    s = Stream(w)
    s.fill(65, 9)
    for d in (1, 2, 63, 64, 65):
        s.copy(4096, dist=d)
    s.fill(w * h, 10)
    mw = (w + 3) // 4
    meta = [(x + y) & 1 for y in range((h + 3) // 4) for x in range(mw)]
    out.append(("long_copies_two_groups", _file(w, h, ops=s.ops, meta=meta, meta_bits=2)))

    s = Stream(4)
    s.fill(4, 11)
    s.copy(12, dist=4)
    out.append(("copy_to_last_pixel", _file(4, 4, ops=s.ops)))

    # code length 15: lengths 1, 2, .., 14, 15, 15 on green
    g15 = [("px", 0xFF000000 | ((i % 16) << 8) | 0x330044) for i in range(64)]
    lens15 = list(range(1, 15)) + [15, 15]
    out.append(("code_length_15", _file(8, 8, ops=g15, groups=[[("lens", lens15), None, None, None, None]])))
    out.append(("max_symbol", _file(8, 8, ops=g15, groups=[[("lens", lens15, dict(max_symbol=16, cl_stream=[(l, 0) for l in lens15])), None, None, None, None]])))
    rnd = _noise(64, 17)
    cl16 = [0] * 19
    cl16[16] = 1
    rep16 = ("lens", [8] * 256, dict(cl_lens=cl16, cl_stream=[(16, 3)] * 42 + [(16, 1)]))
    out.append(("repeat16_first", _file(8, 8, ops=C.literals(rnd), groups=[[None, rep16, None, None, None]])))
    cl1718 = [0] * 19
    cl1718[1], cl1718[17], cl1718[18] = 1, 2, 2
    two = ("lens", [1, 1], dict(cl_lens=cl1718, cl_stream=[(1, 0), (1, 0), (18, 127), (18, 97), (17, 5)]))
    out.append(("repeat17_18_to_end", _file(8, 8, ops=[("px", (p & 0x00FFFFFF) | ((p >> 31) << 24)) for p in rnd], groups=[[None, None, None, two, None]])))
    out.append(("all_single_symbol", _file(7, 5, ops=[("px", 0x80112233)] * 35)))
    out.append(("rba_single_green_normal", _file(7, 5, ops=[("px", 0xFF400050 | ((p & 255) << 8)) for p in _noise(35, 18)])))

    def grouped(w, h):
        mw = (w + 3) // 4
        meta = list(range(mw * ((h + 3) // 4)))
        ops = [("px", 0xFF000000 | (meta[(y // 4) * mw + x // 4] * 0x010203 & 0xFFFFFF)) for y in range(h) for x in range(w)]
        return meta, ops
    meta, ops = grouped(64, 32)
    assert max(meta) + 1 == R.MAX_GROUPS
    out.append(("groups_at_limit", _file(64, 32, ops=ops, meta=meta, meta_bits=2)))
    out.append(("two_groups_alternating", _file(19, 13, ops=C.literals(_noise(19 * 13, 19)), meta=[(i % 5 + i // 5) & 1 for i in range(5 * 4)], meta_bits=2)))
    out.append(("alpha_bit_clear_alpha_data", _file(9, 9, 0, ops=C.literals(px9))))

    pay = C.vp8l(9, 9, 1, ops=C.literals(px9))
    icc, exif = C.chunk(b"ICCP", b"\x01\x02\x03"), C.chunk(b"EXIF", b"Exif\0\0II*\0\x08")
    out.append(("extended_alpha", C.extended_file(pay, 9, 9, 1, before=[icc], after=[exif, C.chunk(b"XMP ", b"<x/>"), C.chunk(b"ABCD", b"odd")], icc=1, exif=1)))
    out.append(("extended_no_alpha", C.extended_file(pay, 9, 9, 0, before=[icc], after=[exif], icc=1, exif=1)))
    out.append(("extended_alpha_flag_header_clear", C.extended_file(C.vp8l(9, 9, 0, ops=C.literals(px9)), 9, 9, 1)))
    return out


@functools.lru_cache(maxsize=None)
def refusals():
    """[(name, bytes, status, why)]"""
    px = _noise(16, 40)
    ok = C.vp8l(4, 4, 1, ops=C.literals(px))
    lossy = C.chunk(b"VP8 ", b"\x30\x01\x00\x9d\x01\x2a\x04\x00\x04\x00")
    U, X = "UNSUPPORTED", "CORRUPT"
    out = [
        ("animated_flag", C.extended_file(ok, 4, 4, 1, anim=1), U, "WebP: animated WebP"),
        ("animated_chunks", C.riff([C.vp8x(4, 4, 1), C.chunk(b"ANIM", b"\0" * 6), C.chunk(b"ANMF", b"\0" * 16 + C.chunk(b"VP8L", ok))]), U, "WebP: animated WebP"),
        ("extended_lossy", C.riff([C.vp8x(4, 4, 0), lossy]), U, "WebP: lossy WebP"),
        ("extended_lossy_alpha", C.riff([C.vp8x(4, 4, 1), C.chunk(b"ALPH", b"\0\1\2"), lossy]), U, "WebP: lossy WebP"),
        ("canvas_mismatch", C.extended_file(ok, 5, 4, 1), X, "WebP: VP8X canvas size differs from the VP8L size"),
        ("truncated_chunk", C.simple_file(ok)[:-3], X, "WebP: truncated chunk"),
        ("chunk_past_riff", C.riff([C.vp8x(4, 4, 1), b"VP8L\xff\xff\x00\x00" + ok]), X, "WebP: truncated chunk"),
        ("bad_signature", C.simple_file(b"\x2e" + ok[1:]), X, "WebP: bad VP8L signature"),
        ("version_1", C.simple_file(C.vp8l(4, 4, 1, ops=C.literals(px), version=1)), X, "WebP: bad VP8L version"),
        ("no_image_chunk", C.riff([C.vp8x(4, 4, 0), C.chunk(b"EXIF", b"abcd")]), X, "WebP: no image chunk"),
        ("short_vp8l", C.riff([C.chunk(b"VP8L", b"\x2f\0\0")]), X, "WebP: truncated chunk"),
    ]
    g = [("px", 0xFF000000 | ((i % 3) << 8)) for i in range(16)]
    out.append(("code_incomplete", _file(4, 4, ops=g, groups=[[("lens", [2, 2, 2]), None, None, None, None]]), X, R.E_CODE))
    out.append(("code_oversubscribed", _file(4, 4, ops=g, groups=[[("lens", [1, 1, 1]), None, None, None, None]]), X, R.E_CODE))
    out.append(("code_empty", _file(4, 4, ops=g[:0] + [("px", 0xFF000000)] * 16, groups=[[None, ("lens", [0, 0]), None, None, None]]), X, R.E_CODE))
    out.append(("copy_before_first", _file(4, 4, ops=[("copy", 1, 121)] + C.literals(px[:15])), X, R.E_COPY))
    out.append(("copy_past_end", _file(2, 2, ops=[("px", px[0]), ("copy", 4, 121)]), X, R.E_COPY))
    out.append(("cache_bits_0", _file(4, 4, ops=C.literals(px), cache_field=0), X, R.E_CACHE))
    out.append(("cache_bits_12", _file(4, 4, ops=C.literals(px), cache_field=12), X, R.E_CACHE))
    out.append(("transform_twice", _file(4, 4, transforms=[(R.T_GREEN,), (R.T_GREEN,)], ops=C.literals(px)), X, R.E_TRANSFORM))
    out.append(("data_ends_early", C.simple_file(C.vp8l(8, 8, 1, ops=C.literals(_noise(64, 41)))[:-20]), X, R.E_BITS))
    w, h = 172, 12
    mw = (w + 3) // 4
    meta = list(range(mw * 3))
    assert len(meta) == R.MAX_GROUPS + 1
    ops = [("px", 0xFF000000 | meta[(y // 4) * mw + x // 4]) for y in range(h) for x in range(w)]
    out.append(("groups_over_limit", _file(w, h, ops=ops, meta=meta, meta_bits=2), U, R.E_GROUPS))
    return out


SIMPLE_LOSSY = C.riff([C.chunk(b"VP8 ", b"\x30\x01\x00\x9d\x01\x2a\x04\x00\x04\x00")])  # not named by the sniff: an unknown format
