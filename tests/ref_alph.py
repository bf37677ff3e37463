"""ref_alph.py — a plain Python restatement of the lossy WebP path with context options
"webp_lossy" and "webp_alpha" both on: ref_vp8's frame decode plus the ALPH rules of
parse_webp_lossy (host/webp_header.cpp) and dg_alph.h, with the library's statuses and texts.
It is pinned to Pillow (libwebp, MODE_RGBA) byte for byte in tests/test_alph_cpu.py.

decode(data) -> Result(status, why, width, height, channels, pixels): Rgba8 bytes for a file
with an ALPH chunk before its image chunk, Rgb8 bytes (ref_vp8's) for any other file.
`cover`, when given, is a set that receives ("alph", compression, filter) and, for the
gradient filter, ("grad", "first strip") / ("grad", "row above from the plane").

An ALPH payload is a header byte (bits 0-1 compression: 0 raw, 1 VP8L; bits 2-3 filter:
0 none, 1 horizontal, 2 vertical, 3 gradient; bits 4-5 pre-processing, 0 or 1 and ignored;
bits 6-7 reserved) and then the filtered plane g: raw bytes, or the green channel of a header-less
VP8L stream of the frame's size.  Mod 256, o[y][x] = g[y][x] + p.

End-of-data rule of the VP8L-coded plane.  libwebp decodes the stream its encoder writes for
few alpha levels (colour indexing as the only transform, no colour cache, one-symbol red,
blue and alpha codes in every group) through a path of its own, which looks for the end of
its data after each pixel or copy and only while pixels are missing: for such a stream the
main image is read by ref_webp's loop without the check inside a copy and without the
check after the last pixel (reads past the end give zeros).  Every other stream, and every
sub-image, keeps ref_webp's rule: refused wherever ref_webp looks and finds the reader past
the end.
"""
import functools
from collections import namedtuple

import numpy as np

import ref_vp8 as RV
import ref_webp as RW

OK, UNSUPPORTED, CORRUPT = RV.OK, RV.UNSUPPORTED, RV.CORRUPT
Result = namedtuple("Result", "status why width height channels pixels")

E_TWO = "WebP: more than one ALPH chunk"
E_FLAG = "WebP: ALPH chunk in a file whose VP8X alpha flag is clear"
E_SHORT_CHUNK = "WebP: ALPH chunk of fewer than 2 bytes"
E_HEADER = "WebP: bad ALPH header byte"
E_RAW = "WebP: raw alpha plane shorter than the image"
E_STREAM = "WebP: ALPH lossless stream does not decode"
E_GROUPS = "WebP: ALPH stream with more prefix-code groups than the GPU path holds"

NONE, HORIZONTAL, VERTICAL, GRADIENT = range(4)
RAW, VP8L = 0, 1


def parse(data):
    """The container walk with webp_lossy and webp_alpha on: ref_vp8.parse's fields plus
    has_alph, alpha_flag, alph_off, alph_len, alph_hdr."""
    d, n = data, len(data)
    le = RV.le
    h = dict(claim=False, status=CORRUPT, why="not a WebP", width=0, height=0, off=0, len=0, part0=0, extended=0,
             has_alph=0, alpha_flag=0, alph_off=0, alph_len=0, alph_hdr=0)
    if n < 16 or d[:4] != b"RIFF" or d[8:12] != b"WEBP" or d[12:16] not in (b"VP8 ", b"VP8X"):
        return h
    h["claim"] = True

    def fail(st, why):
        h["status"], h["why"] = st, why
        return h

    riff = le(d, 4, 4)
    if riff < 4 or 8 + riff > n:
        return fail(CORRUPT, "WebP: truncated chunk")
    end, pos, first, unsup = 8 + riff, 12, True, None
    cw = ch = 0
    while True:
        if pos + 8 > end:
            if unsup:
                return fail(UNSUPPORTED, unsup)
            return fail(CORRUPT, "WebP: no image chunk" if pos >= end else "WebP: truncated chunk")
        cc, ln, body = d[pos:pos + 4], le(d, pos + 4, 4), pos + 8
        if body + ln > end:
            return fail(CORRUPT, "WebP: truncated chunk")
        if first and cc == b"VP8X":
            if ln < 10:
                return fail(CORRUPT, "WebP: truncated chunk")
            h["extended"] = 1
            h["alpha_flag"] = 1 if d[body] & 0x10 else 0
            cw, ch = 1 + le(d, body + 4, 3), 1 + le(d, body + 7, 3)
            if d[body] & 2:
                unsup = "WebP: animated WebP"
        elif cc in (b"ANIM", b"ANMF"):
            unsup = unsup or "WebP: animated WebP"
        elif cc == b"ALPH":
            if h["has_alph"]:
                unsup = unsup or E_TWO
            else:
                h.update(has_alph=1, alph_off=body, alph_len=ln, alph_hdr=d[body] if ln else 0)
        elif cc == b"VP8L":
            h["claim"] = False
            return fail(CORRUPT, "not a lossy WebP")
        elif cc == b"VP8 ":
            if unsup:
                return fail(UNSUPPORTED, unsup)
            if ln < 10:
                return fail(CORRUPT, "WebP: truncated VP8 frame header")
            bits = le(d, body, 3)
            if bits & 1:
                return fail(CORRUPT, "WebP: VP8 frame is not a key frame")
            if (bits >> 1) & 7 > 3:
                return fail(CORRUPT, "WebP: VP8 version above 3")
            if not (bits >> 4) & 1:
                return fail(CORRUPT, "WebP: VP8 frame is not shown")
            if d[body + 3:body + 6] != b"\x9d\x01\x2a":
                return fail(CORRUPT, "WebP: bad VP8 start code")
            w, hh = le(d, body + 6, 2) & 0x3fff, le(d, body + 8, 2) & 0x3fff
            if w == 0 or hh == 0:
                return fail(CORRUPT, "WebP: VP8 frame of no size")
            if (bits >> 5) > ln - 10:
                return fail(CORRUPT, "WebP: VP8 first partition reaches past the chunk")
            if h["extended"] and (cw, ch) != (w, hh):
                return fail(CORRUPT, "WebP: VP8X canvas size differs from the VP8 frame size")
            if h["has_alph"]:
                hdr = h["alph_hdr"]
                if not h["alpha_flag"]:
                    return fail(UNSUPPORTED, E_FLAG)
                if h["alph_len"] < 2:
                    return fail(CORRUPT, E_SHORT_CHUNK)
                if (hdr & 3) > VP8L or hdr & 0xe0:
                    return fail(CORRUPT, E_HEADER)
                if (hdr & 3) == RAW and h["alph_len"] - 1 < w * hh:
                    return fail(CORRUPT, E_RAW)
            if w * hh * 4 >= 1 << 31 or ln >= 1 << 28:
                return fail(UNSUPPORTED, "WebP: image too large for the GPU path")
            h.update(status=OK, why="", width=w, height=hh, off=body, len=ln, part0=bits >> 5)
            return h
        first = False
        pos = body + ln + (ln & 1)


def _few_levels_image(b, w, h, groups, cache_bits, meta, meta_bits):
    """ref_webp.decode_pixels with the end of the data looked for before each pixel or copy only."""
    n = w * h
    out = [0] * n
    cache = [0] * (1 << cache_bits) if cache_bits else None
    mw = (w + (1 << meta_bits) - 1) >> meta_bits if meta is not None else 0
    pos = x = y = 0
    g = groups[0]
    while pos < n:
        if meta is not None:
            g = groups[meta[(y >> meta_bits) * mw + (x >> meta_bits)]]
        b.check()
        s = g[0].read(b)
        if s < 256:
            r, bl, a = g[1].read(b), g[2].read(b), g[3].read(b)
            p = (a << 24) | (r << 16) | (s << 8) | bl
            out[pos] = p
            if cache is not None:
                cache[RW.cache_slot(p, cache_bits)] = p
            step = 1
        elif s < 280:
            step = RW.prefix_value(b, s - 256)
            dist = RW.plane_distance(w, RW.prefix_value(b, g[4].read(b)))
            if dist > pos or step > n - pos:
                raise RW.corrupt(RW.E_COPY)
            for k in range(step):
                p = out[pos + k - dist]
                out[pos + k] = p
                if cache is not None:
                    cache[RW.cache_slot(p, cache_bits)] = p
        else:
            if cache is None:
                raise RW.corrupt(RW.E_CACHE)
            p = cache[s - 280]
            out[pos] = p
            cache[RW.cache_slot(p, cache_bits)] = p
            step = 1
        pos += step
        x += step
        while x >= w:
            x -= w
            y += 1
    return out


def vp8l_green(data, w, h):
    """ref_webp.decode_vp8l with the end-of-data rule of the module's head: the green channel of the
    w x h image, as a list."""
    b = RW.Bits(data)
    transforms, seen, xs = [], set(), w
    up = lambda v, bits: (v + (1 << bits) - 1) >> bits
    while b.read(1):
        t = b.read(2)
        if t in seen:
            raise RW.corrupt(RW.E_TRANSFORM)
        seen.add(t)
        if t in (RW.T_PREDICTOR, RW.T_COLOR):
            bits = b.read(3) + 2
            transforms.append((t, xs, bits, RW.sub_image(b, up(xs, bits), up(h, bits))))
        elif t == RW.T_GREEN:
            transforms.append((t, xs, 0, None))
        else:
            n = b.read(8) + 1
            bits = RW.index_bits(n)
            tab = RW.sub_image(b, n, 1)
            for i in range(1, n):
                tab[i] = RW._addpx(tab[i], tab[i - 1])
            transforms.append((t, xs, bits, tab))
            xs = up(xs, bits)
        b.check()
    cb = RW.read_cache_bits(b)
    meta, mbits, ngroups = None, 0, 1
    if b.read(1):
        mbits = b.read(3) + 2
        meta = [(p >> 8) & 0xFFFF for p in RW.sub_image(b, up(xs, mbits), up(h, mbits))]
        ngroups = max(meta) + 1
    b.check()
    if ngroups > min(RW.MAX_GROUPS, up(w, 2) * up(h, 2)):  # vp8l_groups_cap
        raise RW.Fail("UNSUPPORTED", RW.E_GROUPS)
    groups = RW.read_groups(b, ngroups, cb)
    few = [t[0] for t in transforms] == [RW.T_INDEX] and not cb and all(g[k].single is not None for g in groups for k in (1, 2, 3))
    px = (_few_levels_image if few else RW.decode_pixels)(b, xs, h, groups, cb, meta, mbits)
    for t, tw, bits, sub in reversed(transforms):
        if t == RW.T_PREDICTOR:
            px = RW.inv_predictor(px, tw, h, bits, sub)
        elif t == RW.T_COLOR:
            px = RW.inv_color(px, tw, h, bits, sub)
        elif t == RW.T_GREEN:
            px = RW.inv_green(px)
        else:
            px = RW.inv_index(px, tw, h, bits, sub)
    return [(p >> 8) & 255 for p in px]


def unfilter(g, w, h, filt):
    """g: the filtered plane (h x w uint8) -> the alpha plane."""
    g = np.asarray(g, np.uint8).reshape(h, w)
    if filt == NONE:
        return g.copy()
    o = np.zeros((h, w), np.uint8)
    o[0] = np.cumsum(g[0], dtype=np.int64).astype(np.uint8)
    if h > 1:
        o[1:, 0] = (np.cumsum(g[1:, 0], dtype=np.int64) + int(o[0, 0])).astype(np.uint8)
    if filt == HORIZONTAL:
        for y in range(1, h):
            o[y] = (np.cumsum(g[y], dtype=np.int64) + (int(o[y, 0]) - int(g[y, 0]))).astype(np.uint8)
    elif filt == VERTICAL:
        o[1:, 1:] = (np.cumsum(g[1:, 1:], axis=0, dtype=np.int64) + o[0, 1:].astype(np.int64)).astype(np.uint8)
    else:
        gi = g.astype(int).tolist()
        for y in range(1, h):
            above, row, src = [int(v) for v in o[y - 1]], [int(o[y, 0])], gi[y]
            for x in range(1, w):
                row.append((src[x] + min(255, max(0, row[x - 1] + above[x] - above[x - 1]))) & 255)
            o[y] = row
    return o


@functools.lru_cache(maxsize=64)
def _frame(chunk, w, h, part0):
    """(why, rgb) of a VP8 chunk: the cases of one size share one chunk."""
    return RV.decode_frame(chunk, 0, len(chunk), w, h, part0, set())


def alpha_plane(data, h, cover=None):
    """The unfiltered plane of a parsed file (status OK, has_alph), or raises RW.Fail."""
    w, hh, hdr = h["width"], h["height"], h["alph_hdr"]
    payload = data[h["alph_off"] + 1:h["alph_off"] + h["alph_len"]]
    comp, filt = hdr & 3, (hdr >> 2) & 3
    g = list(payload[:w * hh]) if comp == RAW else vp8l_green(payload, w, hh)
    if cover is not None:
        cover.add(("alph", comp, filt))
        if filt == GRADIENT:
            cover.add(("grad", "first strip"))
            if hh > 64:
                cover.add(("grad", "row above from the plane"))
    return unfilter(g, w, hh, filt)


def decode(data, cover=None):
    """What the library answers with webp_lossy and webp_alpha on."""
    data = bytes(data)
    h = parse(data)
    if not h["claim"]:
        return Result(CORRUPT, "", 0, 0, 0, None)
    if h["status"] != OK:
        return Result(h["status"], h["why"], 0, 0, 0, None)
    w, hh = h["width"], h["height"]
    why, rgb = _frame(data[h["off"]:h["off"] + h["len"]], w, hh, h["part0"])
    if why:
        return Result(CORRUPT, why, w, hh, 0, None)
    if not h["has_alph"]:
        return Result(OK, "", w, hh, 3, rgb)
    try:
        a = alpha_plane(data, h, cover)
    except RW.Fail as e:
        if e.status == "UNSUPPORTED":
            return Result(UNSUPPORTED, E_GROUPS, w, hh, 0, None)
        return Result(CORRUPT, E_STREAM, w, hh, 0, None)
    rgba = np.dstack([np.frombuffer(rgb, np.uint8).reshape(hh, w, 3), a])
    return Result(OK, "", w, hh, 4, rgba.tobytes())
