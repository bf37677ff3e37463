"""ref_webp.py: plain Python restatement of the WebP container walk and the VP8L
(lossless) decode, with the library's status rules (option "webp").

decode(data) -> Result(status, why, mode, pixels, report):
  status   "OK" / "UNSUPPORTED" / "CORRUPT" (the library's dg_status names)
  why      the text dg_last_error carries
  mode     "RGB" or "RGBA" (the VP8L header's alpha bit, or the VP8X alpha flag)
  pixels   uint8 array (h, w, 3 or 4)
  report   what the file uses: transforms in order, cache bits, prefix bits, group
           count, the colour-indexing packing bits, counts of literals / copies /
           cache hits of the main image

parse(data) -> dict of the container fields host/webp_header.cpp reports.
The pin is Pillow (libwebp): tests/test_webp_cpu.py compares byte for byte.
"""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "status why mode pixels report")

MAX_GROUPS = 128  # kVp8lMaxGroups of dg_vp8l.h

T_PREDICTOR, T_COLOR, T_GREEN, T_INDEX = 0, 1, 2, 3
TRANSFORM_NAMES = ("predictor", "color", "green", "index")

E_BITS = "WebP: image data ends before the image is complete"
E_CODE = "WebP: prefix code neither complete nor single-symbol"
E_COPY = "WebP: copy reaches before the first or past the last pixel"
E_CACHE = "WebP: colour-cache index or size outside the format"
E_TRANSFORM = "WebP: transform used twice"
E_GROUPS = "WebP: more prefix-code groups than the GPU path holds"

# (x, y) offsets of distance codes 1..120 as (y << 4) | (8 - x)
_PLANE = bytes([
    0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
    0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
    0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
    0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
    0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
    0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70])
assert len(_PLANE) == 120 and len(set(_PLANE)) == 120

CODE_LENGTH_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)


class Fail(Exception):
    def __init__(self, status, why):
        Exception.__init__(self, why)
        self.status, self.why = status, why


def corrupt(why):
    return Fail("CORRUPT", why)


# ------------------------------------------------------------ container

def is_webp(d):
    return len(d) >= 16 and d[:4] == b"RIFF" and d[8:12] == b"WEBP" and d[12:16] in (b"VP8L", b"VP8X")


def parse(d):
    """The RIFF walk of host/webp_header.cpp: raises Fail, else the fields."""
    d = bytes(d)
    if not is_webp(d):
        raise corrupt("not a WebP")
    riff = int.from_bytes(d[4:8], "little")
    if riff < 4 or 8 + riff > len(d):
        raise corrupt("WebP: truncated chunk")
    end = 8 + riff
    pos = 12
    f = dict(extended=0, alpha=0, canvas_w=0, canvas_h=0, width=0, height=0, data_off=0, nbytes=0)
    first = True
    unsup = None
    while True:
        if pos + 8 > end:
            if unsup:
                raise Fail("UNSUPPORTED", unsup)
            raise corrupt("WebP: no image chunk" if pos >= end else "WebP: truncated chunk")
        cc = d[pos:pos + 4]
        n = int.from_bytes(d[pos + 4:pos + 8], "little")
        body = pos + 8
        if body + n > end:
            raise corrupt("WebP: truncated chunk")
        if first and cc == b"VP8X":
            if n < 10:
                raise corrupt("WebP: truncated chunk")
            flags = d[body]
            f["extended"] = 1
            f["alpha"] = 1 if flags & 0x10 else 0
            f["canvas_w"] = 1 + int.from_bytes(d[body + 4:body + 7], "little")
            f["canvas_h"] = 1 + int.from_bytes(d[body + 7:body + 10], "little")
            if flags & 0x02:
                unsup = "WebP: animated WebP"
        elif cc in (b"ANIM", b"ANMF"):
            unsup = unsup or "WebP: animated WebP"
        elif cc in (b"VP8 ", b"ALPH"):
            unsup = unsup or "WebP: lossy WebP"
        elif cc == b"VP8L":
            if unsup:
                raise Fail("UNSUPPORTED", unsup)
            if n < 5:
                raise corrupt("WebP: truncated chunk")
            if d[body] != 0x2F:
                raise corrupt("WebP: bad VP8L signature")
            v = int.from_bytes(d[body + 1:body + 5], "little")
            f["width"] = 1 + (v & 0x3FFF)
            f["height"] = 1 + ((v >> 14) & 0x3FFF)
            if (v >> 29) & 7:
                raise corrupt("WebP: bad VP8L version")
            if f["extended"]:
                if (f["canvas_w"], f["canvas_h"]) != (f["width"], f["height"]):
                    raise corrupt("WebP: VP8X canvas size differs from the VP8L size")
            else:
                f["alpha"] = (v >> 28) & 1
            f["data_off"] = body + 5
            f["nbytes"] = n - 5
            return f
        first = False
        pos = body + n + (n & 1)


# ------------------------------------------------------------ bits and codes

class Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.n = 8 * len(data)
        self.pos = 0

    def read(self, k):
        r = (self.v >> self.pos) & ((1 << k) - 1)
        self.pos += k
        return r

    def check(self):
        if self.pos > self.n:
            raise corrupt(E_BITS)


def _rev(c, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (c & 1)
        c >>= 1
    return r


class Code:
    """A canonical prefix code read LSB-first (codes stored bit-reversed)."""

    def __init__(self, lens):
        used = [(l, s) for s, l in enumerate(lens) if l]
        if not used:
            raise corrupt(E_CODE)
        self.single = used[0][1] if len(used) == 1 else None
        self.map = {}
        self.maxlen = 0
        if self.single is not None:
            return
        count = [0] * 16
        for l, _ in used:
            count[l] += 1
        left = 1
        for l in range(1, 16):
            left = 2 * left - count[l]
            if left < 0:
                raise corrupt(E_CODE)
        if left:
            raise corrupt(E_CODE)
        nxt = [0] * 16
        c = 0
        for l in range(1, 16):
            c = (c + count[l - 1]) << 1
            nxt[l] = c
        for s, l in enumerate(lens):
            if l:
                self.map[(l, _rev(nxt[l], l))] = s
                nxt[l] += 1
        self.maxlen = max(l for l, _ in used)
        self.first = [None] * 256
        for (l, r), s in self.map.items():
            if l <= 8:
                for k in range(r, 256, 1 << l):
                    self.first[k] = (l, s)

    def read(self, b):
        if self.single is not None:
            return self.single
        p = b.v >> b.pos
        e = self.first[p & 255]
        if e is not None:
            b.pos += e[0]
            return e[1]
        for l in range(9, self.maxlen + 1):
            s = self.map.get((l, p & ((1 << l) - 1)))
            if s is not None:
                b.pos += l
                return s
        raise corrupt(E_BITS)  # only past the data's end (the code is complete)


def read_code(b, alphabet):
    lens = [0] * alphabet
    if b.read(1):  # simple
        n = b.read(1) + 1
        s0 = b.read(8 if b.read(1) else 1)
        syms = [s0]
        if n == 2:
            syms.append(b.read(8))
        for s in syms:
            if s >= alphabet:
                raise corrupt(E_CODE)
            lens[s] = 1
    else:
        cl = [0] * 19
        n = 4 + b.read(4)
        for i in range(n):
            cl[CODE_LENGTH_ORDER[i]] = b.read(3)
        b.check()
        clc = Code(cl)
        max_symbol = alphabet
        if b.read(1):
            nb = 2 + 2 * b.read(3)
            max_symbol = 2 + b.read(nb)
            if max_symbol > alphabet:
                raise corrupt(E_CODE)
        s, prev = 0, 8
        while s < alphabet:
            if max_symbol == 0:
                break
            max_symbol -= 1
            b.check()
            c = clc.read(b)
            if c < 16:
                lens[s] = c
                s += 1
                if c:
                    prev = c
            else:
                rep = b.read((2, 3, 7)[c - 16]) + (3, 3, 11)[c - 16]
                if s + rep > alphabet:
                    raise corrupt(E_CODE)
                if c == 16:
                    lens[s:s + rep] = [prev] * rep
                s += rep
    b.check()
    return Code(lens)


def prefix_value(b, sym):
    if sym < 4:
        return sym + 1
    extra = (sym - 2) >> 1
    return ((2 + (sym & 1)) << extra) + b.read(extra) + 1


def plane_distance(width, code):
    if code > 120:
        return code - 120
    m = _PLANE[code - 1]
    d = (m >> 4) * width + 8 - (m & 15)
    return d if d >= 1 else 1


def cache_slot(argb, bits):
    return ((0x1E35A7BD * argb) & 0xFFFFFFFF) >> (32 - bits)


# ------------------------------------------------------------ the entropy-coded image

def read_cache_bits(b):
    if not b.read(1):
        return 0
    bits = b.read(4)
    if bits < 1 or bits > 11:
        raise corrupt(E_CACHE)
    return bits


def read_groups(b, n, cache_bits):
    sizes = (256 + 24 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    return [[read_code(b, a) for a in sizes] for _ in range(n)]


def decode_pixels(b, w, h, groups, cache_bits, meta=None, meta_bits=0, counts=None):
    n = w * h
    out = [0] * n
    cache = [0] * (1 << cache_bits) if cache_bits else None
    mw = (w + (1 << meta_bits) - 1) >> meta_bits if meta is not None else 0
    pos = x = y = 0
    lit = cop = hit = 0
    g = groups[0]
    while pos < n:
        if meta is not None:
            g = groups[meta[(y >> meta_bits) * mw + (x >> meta_bits)]]
        b.check()
        s = g[0].read(b)
        if s < 256:
            r = g[1].read(b)
            bl = g[2].read(b)
            a = g[3].read(b)
            p = (a << 24) | (r << 16) | (s << 8) | bl
            out[pos] = p
            if cache is not None:
                cache[cache_slot(p, cache_bits)] = p
            pos += 1
            x += 1
            lit += 1
        elif s < 280:
            length = prefix_value(b, s - 256)
            dist = plane_distance(w, prefix_value(b, g[4].read(b)))
            b.check()
            if dist > pos or length > n - pos:
                raise corrupt(E_COPY)
            for k in range(length):
                p = out[pos + k - dist]
                out[pos + k] = p
                if cache is not None:
                    cache[cache_slot(p, cache_bits)] = p
            pos += length
            x += length
            cop += 1
        else:
            if cache is None:
                raise corrupt(E_CACHE)
            p = cache[s - 280]
            out[pos] = p
            cache[cache_slot(p, cache_bits)] = p
            pos += 1
            x += 1
            hit += 1
        while x >= w:
            x -= w
            y += 1
    b.check()
    if counts is not None:
        counts.update(literals=lit, copies=cop, cache_hits=hit)
    return out


def sub_image(b, w, h):
    cb = read_cache_bits(b)
    return decode_pixels(b, w, h, read_groups(b, 1, cb), cb)


# ------------------------------------------------------------ inverse transforms

def _addpx(a, b):
    return (((a & 0xFF00FF00) + (b & 0xFF00FF00)) & 0xFF00FF00) | (((a & 0x00FF00FF) + (b & 0x00FF00FF)) & 0x00FF00FF)


def _avg2(a, b):
    return (((a ^ b) & 0xFEFEFEFE) >> 1) + (a & b)


def _ch(p):
    return ((p >> 24) & 255, (p >> 16) & 255, (p >> 8) & 255, p & 255)


def _pack(c):
    return (c[0] << 24) | (c[1] << 16) | (c[2] << 8) | c[3]


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _select(L, T, TL):
    pl = sum(abs(t - tl) for t, tl in zip(_ch(T), _ch(TL)))
    pt = sum(abs(l - tl) for l, tl in zip(_ch(L), _ch(TL)))
    return L if pl < pt else T


def _half(a, b):  # C division: towards zero
    d = a - b
    return _clip(a + (d // 2 if d >= 0 else -((-d) // 2)))


def predict(mode, L, T, TL, TR):
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg2(_avg2(L, TR), T)
    if mode == 6:
        return _avg2(L, TL)
    if mode == 7:
        return _avg2(L, T)
    if mode == 8:
        return _avg2(TL, T)
    if mode == 9:
        return _avg2(T, TR)
    if mode == 10:
        return _avg2(_avg2(L, TL), _avg2(T, TR))
    if mode == 11:
        return _select(L, T, TL)
    if mode == 12:
        return _pack([_clip(l + t - tl) for l, t, tl in zip(_ch(L), _ch(T), _ch(TL))])
    if mode == 13:
        return _pack([_half(a, tl) for a, tl in zip(_ch(_avg2(L, T)), _ch(TL))])
    return 0xFF000000  # 0, and 14 / 15 as libwebp


def inv_predictor(px, w, h, bits, sub):
    bw = (w + (1 << bits) - 1) >> bits
    out = [0] * (w * h)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                pr = 0xFF000000 if x == 0 else out[i - 1]
            elif x == 0:
                pr = out[i - w]
            else:
                mode = (sub[(y >> bits) * bw + (x >> bits)] >> 8) & 15
                pr = predict(mode, out[i - 1], out[i - w], out[i - w - 1], out[i - w + 1])
            out[i] = _addpx(px[i], pr)
    return out


def _s8(v):
    return v - 256 if v & 128 else v


def _delta(t, c):
    return (_s8(t) * _s8(c)) >> 5


def inv_color(px, w, h, bits, sub):
    bw = (w + (1 << bits) - 1) >> bits
    out = [0] * (w * h)
    for y in range(h):
        for x in range(w):
            m = sub[(y >> bits) * bw + (x >> bits)]
            p = px[y * w + x]
            g = (p >> 8) & 255
            r = ((p >> 16) + _delta(m & 255, g)) & 255
            bl = (p + _delta((m >> 8) & 255, g) + _delta((m >> 16) & 255, r)) & 255
            out[y * w + x] = (p & 0xFF00FF00) | (r << 16) | bl
    return out


def inv_green(px):
    out = []
    for p in px:
        g = (p >> 8) & 255
        out.append((p & 0xFF00FF00) | ((((p >> 16) + g) & 255) << 16) | ((p + g) & 255))
    return out


def index_bits(n):
    return 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3


def inv_index(px, w, h, bits, table):
    pw = (w + (1 << bits) - 1) >> bits
    bpp = 8 >> bits
    out = [0] * (w * h)
    for y in range(h):
        for x in range(w):
            g = (px[y * pw + (x >> bits)] >> 8) & 255
            i = (g >> ((x & ((1 << bits) - 1)) * bpp)) & ((1 << bpp) - 1)
            out[y * w + x] = table[i] if i < len(table) else 0
    return out


# ------------------------------------------------------------ the whole stream

def decode_vp8l(data, w, h, report=None, groups_only=False):
    """data: the VP8L chunk's bytes after the 5-byte header -> ARGB list (w * h).
    groups_only: stop after the prefix image and return the group count."""
    b = Bits(data)
    transforms = []
    seen = set()
    xs = w
    while b.read(1):
        t = b.read(2)
        if t in seen:
            raise corrupt(E_TRANSFORM)
        seen.add(t)
        if t in (T_PREDICTOR, T_COLOR):
            bits = b.read(3) + 2
            sub = sub_image(b, (xs + (1 << bits) - 1) >> bits, (h + (1 << bits) - 1) >> bits)
            transforms.append((t, xs, bits, sub))
        elif t == T_GREEN:
            transforms.append((t, xs, 0, None))
        else:
            n = b.read(8) + 1
            bits = index_bits(n)
            tab = sub_image(b, n, 1)
            for i in range(1, n):
                tab[i] = _addpx(tab[i], tab[i - 1])
            transforms.append((t, xs, bits, tab))
            xs = (xs + (1 << bits) - 1) >> bits
        b.check()
    cb = read_cache_bits(b)
    meta, mbits, ngroups = None, 0, 1
    if b.read(1):
        mbits = b.read(3) + 2
        meta = [(p >> 8) & 0xFFFF for p in sub_image(b, (xs + (1 << mbits) - 1) >> mbits, (h + (1 << mbits) - 1) >> mbits)]
        ngroups = max(meta) + 1
    b.check()
    if groups_only:
        return ngroups
    if ngroups > MAX_GROUPS:
        raise Fail("UNSUPPORTED", E_GROUPS)
    counts = {}
    groups = read_groups(b, ngroups, cb)
    px = decode_pixels(b, xs, h, groups, cb, meta, mbits, counts)
    if report is not None:
        report.update(transforms=[TRANSFORM_NAMES[t[0]] for t in transforms], cache_bits=cb,
                      index_bits=[t[2] for t in transforms if t[0] == T_INDEX],
                      prefix_bits=mbits if meta is not None else 0, groups=ngroups, **counts)
    for t, tw, bits, sub in reversed(transforms):
        if t == T_PREDICTOR:
            px = inv_predictor(px, tw, h, bits, sub)
        elif t == T_COLOR:
            px = inv_color(px, tw, h, bits, sub)
        elif t == T_GREEN:
            px = inv_green(px)
        else:
            px = inv_index(px, tw, h, bits, sub)
    return px


def group_count(data):
    """Prefix-code groups of a file's main image (what the encoder chose)."""
    f = parse(bytes(data))
    return decode_vp8l(data[f["data_off"]:f["data_off"] + f["nbytes"]], f["width"], f["height"], groups_only=True)


def decode(data):
    data = bytes(data)
    report = {}
    try:
        f = parse(data)
        px = decode_vp8l(data[f["data_off"]:f["data_off"] + f["nbytes"]], f["width"], f["height"], report)
    except Fail as e:
        return Result(e.status, e.why, None, None, report)
    a = np.array(px, dtype=np.uint32).reshape(f["height"], f["width"])
    rgba = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], axis=-1).astype(np.uint8)
    if f["alpha"]:
        return Result("OK", "", "RGBA", rgba, report)
    return Result("OK", "", "RGB", np.ascontiguousarray(rgba[..., :3]), report)
