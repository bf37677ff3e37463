"""ref_vp8.py — a plain Python restatement of the lossy WebP path of context option
"webp_lossy": the container rules of parse_webp_lossy (host/webp_header.cpp) and the whole
VP8 key-frame decode (dg_vp8.h / dg_vp8.hip), with the library's status rules.

It follows libwebp's decoder statement by statement where the format leaves a choice
(border samples, int16 coefficient storage, fancy upsampling, the end-of-partition
rule) and is pinned to Pillow byte for byte in tests/test_vp8_cpu.py.  The constant
tables are the format's; they are read from datago_amd/csrc/dg_vp8_tables.h, and the pin
to Pillow is what checks them.

decode(data) -> Result(status, why, width, height, rgb).  `cover`, when given, is a set
that receives what the decode touched (see universe()).

End-of-partition rule: a bool reader that needs a byte past its partition's end takes a
zero byte and is marked; the decode runs to its end all the same (every loop is
bounded by MB counts) and is DG_ERR_CORRUPT when any reader is marked, as libwebp
refuses such a frame after the MB that met it.
"""
import os
import re
from collections import namedtuple

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
Result = namedtuple("Result", "status why width height rgb")

_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "datago_amd", "csrc", "dg_vp8_tables.h")


def _tables():
    text = open(_HDR).read() + "\n\n"
    out = {}
    for name in ("VP8_COEF0", "VP8_UPD", "VP8_BMODES", "VP8_DC", "VP8_AC"):
        m = re.search(r"#define %s \\\n(.*?)\n\n" % name, text, re.S)
        out[name] = [int(v) for v in re.findall(r"\d+", m.group(1))]
    return out


_T = _tables()
COEF0, UPD, BMODES, DCQ, ACQ = _T["VP8_COEF0"], _T["VP8_UPD"], _T["VP8_BMODES"], _T["VP8_DC"], _T["VP8_AC"]
assert (len(COEF0), len(UPD), len(BMODES), len(DCQ), len(ACQ)) == (1056, 1056, 900, 128, 128)

DC_PRED, TM_PRED, V_PRED, H_PRED, B_PRED = 0, 1, 2, 3, 4
B_DC, B_TM, B_VE, B_HE, B_RD, B_VR, B_LD, B_VL, B_HD, B_HU = range(10)
BMODE_TREE = [-B_DC, 1, -B_TM, 2, -B_VE, 3, 4, 6, -B_HE, 5, -B_RD, -B_VR, -B_LD, 7, -B_VL, 8, -B_HD, -B_HU]
ZIGZAG = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]
BANDS = [0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0]
CAT = [[173, 148, 140], [176, 155, 140, 135], [180, 157, 141, 134, 130], [254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129]]

FAIL_BITS = "WebP: VP8 data ends before the image is complete"
FAIL_PARTS = "WebP: VP8 token-partition table reaches past the chunk"


def le(d, at, n):
    return int.from_bytes(d[at:at + n], "little")


def parse(data):
    """The container walk with webp_lossy on: dict(claim, status, why, width, height, off, len, part0).
    claim False: the file is not the lossy path's (no WebP, or its image chunk is VP8L)."""
    d, n = data, len(data)
    h = dict(claim=False, status=CORRUPT, why="not a WebP", width=0, height=0, off=0, len=0, part0=0, extended=0)
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
            cw, ch = 1 + le(d, body + 4, 3), 1 + le(d, body + 7, 3)
            if d[body] & 2:
                unsup = "WebP: animated WebP"
        elif cc in (b"ANIM", b"ANMF"):
            unsup = unsup or "WebP: animated WebP"
        elif cc == b"ALPH":
            unsup = unsup or "WebP: lossy WebP with alpha"
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
            if w * hh * 4 >= 1 << 31 or ln >= 1 << 28:
                return fail(UNSUPPORTED, "WebP: image too large for the GPU path")
            h.update(status=OK, why="", width=w, height=hh, off=body, len=ln, part0=bits >> 5)
            return h
        first = False
        pos = body + ln + (ln & 1)


class BoolDec:
    def __init__(self, d, start, end):
        self.d, self.pos, self.end = d, start, end
        self.value, self.range, self.bits, self.eof = 0, 254, -8, False
        self._load()

    def _load(self):
        if self.pos < self.end:
            self.value = (self.value << 8) | self.d[self.pos]
            self.pos += 1
            self.bits += 8
        elif not self.eof:
            self.value <<= 8
            self.bits += 8
            self.eof = True
        else:
            self.bits = 0

    def bit(self, prob):
        rng = self.range
        if self.bits < 0:
            self._load()
        pos = self.bits
        split = (rng * prob) >> 8
        value = self.value >> pos
        if value > split:
            rng -= split
            self.value -= (split + 1) << pos
            b = 1
        else:
            rng = split + 1
            b = 0
        shift = 7 ^ (rng.bit_length() - 1)
        rng <<= shift
        self.bits -= shift
        self.range = rng - 1
        return b

    def get(self, n):
        v = 0
        while n > 0:
            n -= 1
            v |= self.bit(128) << n
        return v

    def signed(self, n):
        v = self.get(n)
        return -v if self.get(1) else v


def i16(v):
    return ((v + 32768) & 0xffff) - 32768


def clip8(v):
    return 0 if v < 0 else 255 if v > 255 else v


def clipq(v, m):
    return 0 if v < 0 else m if v > m else v


def mb_pos(x, y, mbw):
    return "corner" if x == 0 and y == 0 else "top" if y == 0 else "left" if x == 0 else "right" if x == mbw - 1 else "interior"


def universe():
    """Everything the case set has to reach."""
    u = set()
    for p in ("corner", "top", "left", "right", "interior"):
        for m in range(5):
            u.add(("ymode", m, p))
        for m in range(4):
            u.add(("uvmode", m, p))
        for m in range(10):
            u.add(("bmode", m, p))
    for t in ("zero", "one", "two", "three", "four", "cat1", "cat2", "cat3", "cat4", "cat5", "cat6"):
        u.add(("token", t))
    for b in range(8):
        u.add(("eob", b))
        u.add(("band", b))
    for t in range(4):
        for c in range(3):
            u.add(("ctx", t, c))
    for f in ("simple", "normal"):
        u.add(("filter", f))
    for t in (0, 1, 2):
        u.add(("hev", t))
    for k in ("mb", "inner", "hev", "nohev"):
        u.add(("edge", k))
    for n in (1, 2, 4, 8):
        u.add(("parts", n))
    for k in ("segmap", "segnomap", "segdelta", "segabs", "qclip0", "qclip127", "noskipprob", "skipprob", "skipmb",
              "probupdate", "noprobupdate", "lfdelta", "level0", "sharp", "colorspace", "clamp", "eof"):
        u.add(("hdr", k))
    return u


def get_coeffs(br, probs, typ, ctx, dq, n, out, cover):
    """libwebp's GetCoeffs: tokens of one block from position n; returns 1 + the last non-zero position."""
    def P(nn, c):
        return probs[((typ * 8 + BANDS[nn]) * 3 + c) * 11:][:11]
    cover.add(("ctx", typ, ctx))
    p = P(n, ctx)
    while n < 16:
        cover.add(("band", BANDS[n]))
        if not br.bit(p[0]):
            cover.add(("eob", BANDS[n]))
            return n
        while not br.bit(p[1]):
            cover.add(("token", "zero"))
            n += 1
            p = P(n, 0)
            if n == 16:
                return 16
        if not br.bit(p[2]):
            v, nc = 1, 1
            cover.add(("token", "one"))
        else:
            nc = 2
            if not br.bit(p[3]):
                if not br.bit(p[4]):
                    v = 2
                    cover.add(("token", "two"))
                else:
                    v = 3 + br.bit(p[5])
                    cover.add(("token", "three" if v == 3 else "four"))
            elif not br.bit(p[6]):
                if not br.bit(p[7]):
                    v = 5 + br.bit(159)
                    cover.add(("token", "cat1"))
                else:
                    v = 7 + 2 * br.bit(165)
                    v += br.bit(145)
                    cover.add(("token", "cat2"))
            else:
                b1 = br.bit(p[8])
                b0 = br.bit(p[9 + b1])
                cat = 2 * b1 + b0
                v = 0
                for pr in CAT[cat]:
                    v += v + br.bit(pr)
                v += 3 + (8 << cat)
                cover.add(("token", "cat%d" % (cat + 3)))
        if br.bit(128):
            v = -v
        out[ZIGZAG[n]] = i16(v * dq[1 if n > 0 else 0])
        n += 1
        p = P(n, nc)
    return 16


def wht(dc):
    tmp = [0] * 16
    for i in range(4):
        a0, a1 = dc[i] + dc[12 + i], dc[4 + i] + dc[8 + i]
        a2, a3 = dc[4 + i] - dc[8 + i], dc[i] - dc[12 + i]
        tmp[i], tmp[8 + i], tmp[4 + i], tmp[12 + i] = a0 + a1, a0 - a1, a3 + a2, a3 - a2
    out = [0] * 16
    for i in range(4):
        d0 = tmp[i * 4] + 3
        a0, a1 = d0 + tmp[3 + i * 4], tmp[1 + i * 4] + tmp[2 + i * 4]
        a2, a3 = tmp[1 + i * 4] - tmp[2 + i * 4], d0 - tmp[3 + i * 4]
        out[i * 4 + 0], out[i * 4 + 1] = i16((a0 + a1) >> 3), i16((a3 + a2) >> 3)
        out[i * 4 + 2], out[i * 4 + 3] = i16((a0 - a1) >> 3), i16((a3 - a2) >> 3)
    return out


def mul1(a):
    return ((a * 20091) >> 16) + a


def mul2(a):
    return (a * 35468) >> 16


def idct_add(c, B, r0, c0):
    """The inverse DCT of the 16 coefficients c added to B[r0..r0+3][c0..c0+3]."""
    tmp = [0] * 16
    for i in range(4):
        a, b = c[i] + c[8 + i], c[i] - c[8 + i]
        cc = mul2(c[4 + i]) - mul1(c[12 + i])
        d = mul1(c[4 + i]) + mul2(c[12 + i])
        tmp[4 * i], tmp[4 * i + 1], tmp[4 * i + 2], tmp[4 * i + 3] = a + d, b + cc, b - cc, a - d
    for i in range(4):
        dc = tmp[i] + 4
        a, b = dc + tmp[8 + i], dc - tmp[8 + i]
        cc = mul2(tmp[4 + i]) - mul1(tmp[12 + i])
        d = mul1(tmp[4 + i]) + mul2(tmp[12 + i])
        row = B[r0 + i]
        row[c0] = clip8(row[c0] + ((a + d) >> 3))
        row[c0 + 1] = clip8(row[c0 + 1] + ((b + cc) >> 3))
        row[c0 + 2] = clip8(row[c0 + 2] + ((b - cc) >> 3))
        row[c0 + 3] = clip8(row[c0 + 3] + ((a - d) >> 3))


def pred_block(B, r0, c0, n, mode, x, y):
    """16x16 / 8x8 prediction (n = 16 or 8) into B, whose row r0 - 1 and column c0 - 1 hold the border."""
    top = B[r0 - 1][c0:c0 + n]
    left = [B[r0 + j][c0 - 1] for j in range(n)]
    sh = 4 if n == 16 else 3
    if mode == DC_PRED:
        if x and y:
            v = (sum(top) + sum(left) + n) >> (sh + 1)
        elif y:
            v = (sum(top) + (n >> 1)) >> sh
        elif x:
            v = (sum(left) + (n >> 1)) >> sh
        else:
            v = 128
        for j in range(n):
            B[r0 + j][c0:c0 + n] = [v] * n
    elif mode == TM_PRED:
        tl = B[r0 - 1][c0 - 1]
        for j in range(n):
            B[r0 + j][c0:c0 + n] = [clip8(t + left[j] - tl) for t in top]
    elif mode == V_PRED:
        for j in range(n):
            B[r0 + j][c0:c0 + n] = top
    else:
        for j in range(n):
            B[r0 + j][c0:c0 + n] = [left[j]] * n


def pred4(B, r0, c0, mode):
    def a3(a, b, c):
        return (a + 2 * b + c + 2) >> 2

    def a2(a, b):
        return (a + b + 1) >> 1
    T = B[r0 - 1]
    X = T[c0 - 1]
    A, Bb, C, D, E, F, G, H = T[c0:c0 + 8]
    I, J, K, L = (B[r0 + j][c0 - 1] for j in range(4))
    o = [[0] * 4 for _ in range(4)]  # o[y][x]
    if mode == B_DC:
        v = (A + Bb + C + D + I + J + K + L + 4) >> 3
        o = [[v] * 4 for _ in range(4)]
    elif mode == B_TM:
        o = [[clip8(t + l - X) for t in (A, Bb, C, D)] for l in (I, J, K, L)]
    elif mode == B_VE:
        r = [a3(X, A, Bb), a3(A, Bb, C), a3(Bb, C, D), a3(C, D, E)]
        o = [list(r) for _ in range(4)]
    elif mode == B_HE:
        o = [[a3(X, I, J)] * 4, [a3(I, J, K)] * 4, [a3(J, K, L)] * 4, [a3(K, L, L)] * 4]
    elif mode == B_RD:
        e = [a3(J, K, L), a3(I, J, K), a3(X, I, J), a3(A, X, I), a3(Bb, A, X), a3(C, Bb, A), a3(D, C, Bb)]
        for yy in range(4):
            for xx in range(4):
                o[yy][xx] = e[3 - yy + xx]
    elif mode == B_VR:
        o[0][0] = o[2][1] = a2(X, A)
        o[0][1] = o[2][2] = a2(A, Bb)
        o[0][2] = o[2][3] = a2(Bb, C)
        o[0][3] = a2(C, D)
        o[3][0] = a3(K, J, I)
        o[2][0] = a3(J, I, X)
        o[1][0] = o[3][1] = a3(I, X, A)
        o[1][1] = o[3][2] = a3(X, A, Bb)
        o[1][2] = o[3][3] = a3(A, Bb, C)
        o[1][3] = a3(Bb, C, D)
    elif mode == B_LD:
        e = [a3(A, Bb, C), a3(Bb, C, D), a3(C, D, E), a3(D, E, F), a3(E, F, G), a3(F, G, H), a3(G, H, H)]
        for yy in range(4):
            for xx in range(4):
                o[yy][xx] = e[xx + yy]
    elif mode == B_VL:
        o[0][0] = a2(A, Bb)
        o[0][1] = o[2][0] = a2(Bb, C)
        o[0][2] = o[2][1] = a2(C, D)
        o[0][3] = o[2][2] = a2(D, E)
        o[1][0] = a3(A, Bb, C)
        o[1][1] = o[3][0] = a3(Bb, C, D)
        o[1][2] = o[3][1] = a3(C, D, E)
        o[1][3] = o[3][2] = a3(D, E, F)
        o[2][3] = a3(E, F, G)
        o[3][3] = a3(F, G, H)
    elif mode == B_HD:
        o[0][0] = o[1][2] = a2(I, X)
        o[1][0] = o[2][2] = a2(J, I)
        o[2][0] = o[3][2] = a2(K, J)
        o[3][0] = a2(L, K)
        o[0][3] = a3(A, Bb, C)
        o[0][2] = a3(X, A, Bb)
        o[0][1] = o[1][3] = a3(I, X, A)
        o[1][1] = o[2][3] = a3(J, I, X)
        o[2][1] = o[3][3] = a3(K, J, I)
        o[3][1] = a3(L, K, J)
    else:  # B_HU
        o[0][0] = a2(I, J)
        o[0][2] = o[1][0] = a2(J, K)
        o[1][2] = o[2][0] = a2(K, L)
        o[0][1] = a3(I, J, K)
        o[0][3] = o[1][1] = a3(J, K, L)
        o[1][3] = o[2][1] = a3(K, L, L)
        o[2][2] = o[2][3] = o[3][0] = o[3][1] = o[3][2] = o[3][3] = L
    for yy in range(4):
        B[r0 + yy][c0:c0 + 4] = o[yy]


# ------------------------------------------------------------ the loop filter

def _sc1(v):
    return -128 if v < -128 else 127 if v > 127 else v


def _sc2(v):
    return -16 if v < -16 else 15 if v > 15 else v


class _Px:
    """A plane addressed as p[at + k * step]."""

    def __init__(self, buf):
        self.b = buf


def _filter2(b, p, s):
    p1, p0, q0, q1 = b[p - 2 * s], b[p - s], b[p], b[p + s]
    a = 3 * (q0 - p0) + _sc1(p1 - q1)
    a1, a2 = _sc2((a + 4) >> 3), _sc2((a + 3) >> 3)
    b[p - s] = clip8(p0 + a2)
    b[p] = clip8(q0 - a1)


def _filter4(b, p, s):
    p1, p0, q0, q1 = b[p - 2 * s], b[p - s], b[p], b[p + s]
    a = 3 * (q0 - p0)
    a1, a2 = _sc2((a + 4) >> 3), _sc2((a + 3) >> 3)
    a3 = (a1 + 1) >> 1
    b[p - 2 * s] = clip8(p1 + a3)
    b[p - s] = clip8(p0 + a2)
    b[p] = clip8(q0 - a1)
    b[p + s] = clip8(q1 - a3)


def _filter6(b, p, s):
    p2, p1, p0, q0, q1, q2 = b[p - 3 * s], b[p - 2 * s], b[p - s], b[p], b[p + s], b[p + 2 * s]
    a = _sc1(3 * (q0 - p0) + _sc1(p1 - q1))
    a1, a2, a3 = (27 * a + 63) >> 7, (18 * a + 63) >> 7, (9 * a + 63) >> 7
    b[p - 3 * s] = clip8(p2 + a3)
    b[p - 2 * s] = clip8(p1 + a2)
    b[p - s] = clip8(p0 + a1)
    b[p] = clip8(q0 - a1)
    b[p + s] = clip8(q1 - a2)
    b[p + 2 * s] = clip8(q2 - a3)


def _needs(b, p, s, t):
    return 4 * abs(b[p - s] - b[p]) + abs(b[p - 2 * s] - b[p + s]) <= t


def _needs2(b, p, s, t, it):
    p3, p2, p1, p0 = b[p - 4 * s], b[p - 3 * s], b[p - 2 * s], b[p - s]
    q0, q1, q2, q3 = b[p], b[p + s], b[p + 2 * s], b[p + 3 * s]
    if 4 * abs(p0 - q0) + abs(p1 - q1) > t:
        return False
    return (abs(p3 - p2) <= it and abs(p2 - p1) <= it and abs(p1 - p0) <= it and abs(q3 - q2) <= it
            and abs(q2 - q1) <= it and abs(q1 - q0) <= it)


def _hev(b, p, s, t):
    return abs(b[p - 2 * s] - b[p - s]) > t or abs(b[p + s] - b[p]) > t


def _edge(b, p, hs, vs, size, thresh, ithresh, hevt, kind, cover):
    """kind 0: simple, 1: macroblock edge, 2: inner edge.  hs: step across the edge, vs: along it."""
    t2 = 2 * thresh + 1
    for _ in range(size):
        if kind == 0:
            if _needs(b, p, hs, t2):
                _filter2(b, p, hs)
        elif _needs2(b, p, hs, t2, ithresh):
            if _hev(b, p, hs, hevt):
                cover.add(("edge", "hev"))
                _filter2(b, p, hs)
            else:
                cover.add(("edge", "nohev"))
                (_filter6 if kind == 1 else _filter4)(b, p, hs)
        p += vs


def filter_mb(Y, U, V, ys, uvs, x, y, simple, limit, ilevel, hevt, inner, cover):
    if limit == 0:
        return
    yp, up = 16 * y * ys + 16 * x, 8 * y * uvs + 8 * x
    cover.add(("filter", "simple" if simple else "normal"))
    if not simple:
        cover.add(("hev", hevt))
    if inner:
        cover.add(("edge", "inner"))
    if x > 0 or y > 0:
        cover.add(("edge", "mb"))
    k = 0 if simple else 1
    if x > 0:
        _edge(Y, yp, 1, ys, 16, limit + 4, ilevel, hevt, k, cover)
        if not simple:
            _edge(U, up, 1, uvs, 8, limit + 4, ilevel, hevt, 1, cover)
            _edge(V, up, 1, uvs, 8, limit + 4, ilevel, hevt, 1, cover)
    if inner:
        for c in (4, 8, 12):
            _edge(Y, yp + c, 1, ys, 16, limit, ilevel, hevt, 2 * k, cover)
        if not simple:
            _edge(U, up + 4, 1, uvs, 8, limit, ilevel, hevt, 2, cover)
            _edge(V, up + 4, 1, uvs, 8, limit, ilevel, hevt, 2, cover)
    if y > 0:
        _edge(Y, yp, ys, 1, 16, limit + 4, ilevel, hevt, k, cover)
        if not simple:
            _edge(U, up, uvs, 1, 8, limit + 4, ilevel, hevt, 1, cover)
            _edge(V, up, uvs, 1, 8, limit + 4, ilevel, hevt, 1, cover)
    if inner:
        for r in (4, 8, 12):
            _edge(Y, yp + r * ys, ys, 1, 16, limit, ilevel, hevt, 2 * k, cover)
        if not simple:
            _edge(U, up + 4 * uvs, uvs, 1, 8, limit, ilevel, hevt, 2, cover)
            _edge(V, up + 4 * uvs, uvs, 1, 8, limit, ilevel, hevt, 2, cover)


# ------------------------------------------------------------ upsampling and colour

def yuv_rgb(y, u, v):
    def c(v):
        return v >> 6 if 0 <= v <= 16383 else 0 if v < 0 else 255
    yy = (y * 19077) >> 8
    return (c(yy + ((v * 26149) >> 8) - 14234), c(yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708),
            c(yy + ((u * 33050) >> 8) - 17685))


def to_rgb(Y, U, V, ys, uvs, w, h):
    out = bytearray(w * h * 3)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    for y in range(h):
        nr = y >> 1
        fr = min(max(nr + (1 if y & 1 else -1), 0), ch - 1)
        for x in range(w):
            nc = x >> 1
            fc = min(max(nc + (1 if x & 1 else -1), 0), cw - 1)
            uv = []
            for P in (U, V):
                a, b, c, d = P[nr * uvs + nc], P[nr * uvs + fc], P[fr * uvs + nc], P[fr * uvs + fc]
                uv.append((((a + 3 * b + 3 * c + d + 8) >> 3) + a) >> 1)
            out[(y * w + x) * 3:(y * w + x) * 3 + 3] = bytes(yuv_rgb(Y[y * ys + x], uv[0], uv[1]))
    return bytes(out)


# ------------------------------------------------------------ the frame

def decode_frame(d, off, ln, w, h, part0, cover):
    """-> (fail text or None, rgb)"""
    mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
    br = BoolDec(d, off + 10, off + 10 + part0)
    if br.get(1):
        cover.add(("hdr", "colorspace"))
    if br.get(1):
        cover.add(("hdr", "clamp"))
    use_seg, update_map, abs_delta = br.get(1), 0, 1
    seg_q, seg_f, seg_p = [0] * 4, [0] * 4, [255] * 3
    if use_seg:
        update_map = br.get(1)
        if br.get(1):
            abs_delta = br.get(1)
            cover.add(("hdr", "segabs" if abs_delta else "segdelta"))
            seg_q = [br.signed(7) if br.get(1) else 0 for _ in range(4)]
            seg_f = [br.signed(6) if br.get(1) else 0 for _ in range(4)]
        if update_map:
            seg_p = [br.get(8) if br.get(1) else 255 for _ in range(3)]
        cover.add(("hdr", "segmap" if update_map else "segnomap"))
    simple, level, sharp = br.get(1), br.get(6), br.get(3)
    use_lf = br.get(1)
    ref_lf, mode_lf = [0] * 4, [0] * 4
    if use_lf and br.get(1):
        for i in range(4):
            if br.get(1):
                ref_lf[i] = br.signed(6)
        for i in range(4):
            if br.get(1):
                mode_lf[i] = br.signed(6)
    if use_lf:
        cover.add(("hdr", "lfdelta"))
    if sharp:
        cover.add(("hdr", "sharp"))
    filter_type = 0 if level == 0 else 1 if simple else 2
    nparts = 1 << br.get(2)
    cover.add(("parts", nparts))
    # the token partitions: 3-byte sizes after the first partition, the last one takes the rest
    tab = off + 10 + part0
    end = off + ln
    if tab + 3 * (nparts - 1) > end:
        return FAIL_PARTS, None
    pstart = tab + 3 * (nparts - 1)
    parts = []
    for p in range(nparts):
        left = end - pstart
        sz = min(le(d, tab + 3 * p, 3), left) if p < nparts - 1 else left  # a size past the chunk is cut to it
        if p == nparts - 1 and sz == 0:  # the last partition starts at the chunk's end
            return FAIL_PARTS, None
        parts.append(BoolDec(d, pstart, pstart + sz))
        pstart += sz
    base_q = br.get(7)
    dq = [br.signed(4) if br.get(1) else 0 for _ in range(5)]  # y1dc, y2dc, y2ac, uvdc, uvac
    qm = []
    for s in range(4):
        q = (seg_q[s] + (0 if abs_delta else base_q)) if use_seg else base_q
        if use_seg and (q < 0 or q + min(dq) < 0):
            cover.add(("hdr", "qclip0"))
        if use_seg and (q > 127 or q + max(dq) > 127):
            cover.add(("hdr", "qclip127"))
        y2ac = (ACQ[clipq(q + dq[2], 127)] * 101581) >> 16
        qm.append(((DCQ[clipq(q + dq[0], 127)], ACQ[clipq(q, 127)]), (DCQ[clipq(q + dq[1], 127)] * 2, max(y2ac, 8)),
                   (DCQ[clipq(q + dq[3], 117)], ACQ[clipq(q + dq[4], 127)])))
    br.get(1)  # refresh entropy probabilities: nothing follows a key frame here
    probs = list(COEF0)
    upd = False
    for i in range(1056):
        if br.bit(UPD[i]):
            probs[i] = br.get(8)
            upd = True
    cover.add(("hdr", "probupdate" if upd else "noprobupdate"))
    use_skip = br.get(1)
    skip_p = br.get(8) if use_skip else 0
    cover.add(("hdr", "skipprob" if use_skip else "noskipprob"))
    # per-segment filter strengths
    fs = [[None, None] for _ in range(4)]
    for s in range(4):
        base = (seg_f[s] + (0 if abs_delta else level)) if use_seg else level
        for i4 in range(2):
            lv = base
            if use_lf:
                lv += ref_lf[0] + (mode_lf[0] if i4 else 0)
            lv = clipq(lv, 63)
            limit = il = hv = 0
            if lv > 0:
                il = lv
                if sharp > 0:
                    il >>= 2 if sharp > 4 else 1
                    il = min(il, 9 - sharp)
                il = max(il, 1)
                limit = 2 * lv + il
                hv = 2 if lv >= 40 else 1 if lv >= 15 else 0
            fs[s][i4] = (limit, il, hv)

    ys, uvs = mbw * 16, mbw * 8
    Y, U, V = bytearray(ys * mbh * 16), bytearray(uvs * mbh * 8), bytearray(uvs * mbh * 8)
    finfo = [None] * (mbw * mbh)
    top_modes = [B_DC] * (4 * mbw)
    top_nz, top_dc = [0] * mbw, [0] * mbw
    for my in range(mbh):
        tb = parts[my & (nparts - 1)]
        left_modes = [B_DC] * 4
        left_nz = left_dc = 0
        for mx in range(mbw):
            pos = mb_pos(mx, my, mbw)
            # ---- modes (first partition)
            seg = 0
            if update_map:
                seg = (2 + br.bit(seg_p[2])) if br.bit(seg_p[0]) else br.bit(seg_p[1])
            skip = br.bit(skip_p) if use_skip else 0
            i4 = 0 if br.bit(145) else 1
            modes = [0] * 16
            if not i4:
                ym = (TM_PRED if br.bit(128) else H_PRED) if br.bit(156) else (V_PRED if br.bit(163) else DC_PRED)
                modes[0] = ym
                top_modes[4 * mx:4 * mx + 4] = [ym] * 4
                left_modes = [ym] * 4
                cover.add(("ymode", ym, pos))
            else:
                cover.add(("ymode", B_PRED, pos))
                for yy in range(4):
                    m = left_modes[yy]
                    for xx in range(4):
                        pr = BMODES[(top_modes[4 * mx + xx] * 10 + m) * 9:][:9]
                        i = BMODE_TREE[br.bit(pr[0])]
                        while i > 0:
                            i = BMODE_TREE[2 * i + br.bit(pr[i])]
                        m = -i
                        top_modes[4 * mx + xx] = m
                        modes[4 * yy + xx] = m
                        cover.add(("bmode", m, pos))
                    left_modes[yy] = m
            uvm = DC_PRED if not br.bit(142) else V_PRED if not br.bit(114) else TM_PRED if br.bit(183) else H_PRED
            cover.add(("uvmode", uvm, pos))
            # ---- tokens
            coef = [0] * 384
            if skip:
                cover.add(("hdr", "skipmb"))
                left_nz = top_nz[mx] = 0
                if not i4:
                    left_dc = top_dc[mx] = 0
            else:
                q = qm[seg]
                nzy = nzuv = 0
                if not i4:
                    dc = [0] * 16
                    nz = get_coeffs(tb, probs, 1, top_dc[mx] + left_dc, q[1], 0, dc, cover)
                    top_dc[mx] = left_dc = 1 if nz > 0 else 0
                    if nz > 1:
                        o = wht(dc)
                    else:
                        o = [i16((dc[0] + 3) >> 3)] * 16
                    for k in range(16):
                        coef[k * 16] = o[k]
                    first, typ = 1, 0
                else:
                    first, typ = 0, 3
                tnz, lnz = top_nz[mx] & 15, left_nz & 15
                for yy in range(4):
                    l = lnz & 1
                    for xx in range(4):
                        blk = [0] * 16
                        blk[0] = coef[(4 * yy + xx) * 16]
                        nz = get_coeffs(tb, probs, typ, l + (tnz & 1), q[0], first, blk, cover)
                        coef[(4 * yy + xx) * 16:(4 * yy + xx) * 16 + 16] = blk
                        l = 1 if nz > first else 0
                        tnz = (tnz >> 1) | (l << 7)
                        nzy |= 1 if (nz > 1 or blk[0] != 0) else 0
                    tnz >>= 4
                    lnz = (lnz >> 1) | (l << 7)
                out_t, out_l = tnz, lnz >> 4
                for ch in (0, 2):
                    tnz, lnz = top_nz[mx] >> (4 + ch), left_nz >> (4 + ch)
                    for yy in range(2):
                        l = lnz & 1
                        for xx in range(2):
                            at = (16 + 2 * ch + 2 * yy + xx) * 16
                            blk = [0] * 16
                            nz = get_coeffs(tb, probs, 2, l + (tnz & 1), q[2], 0, blk, cover)
                            coef[at:at + 16] = blk
                            l = 1 if nz > 0 else 0
                            tnz = (tnz >> 1) | (l << 3)
                            nzuv |= 1 if (nz > 1 or blk[0] != 0) else 0
                        tnz >>= 2
                        lnz = (lnz >> 1) | (l << 5)
                    out_t |= (tnz << 4) << ch
                    out_l |= (lnz & 0xf0) << ch
                top_nz[mx], left_nz = out_t & 0xff, out_l & 0xff
                skip = 0 if (nzy | nzuv) else 1
            if filter_type:
                limit, il, hv = fs[seg][i4]
                if limit == 0:
                    cover.add(("hdr", "level0"))
                finfo[my * mbw + mx] = (limit, il, hv, 1 if (i4 or not skip) else 0)
            # ---- reconstruction (unfiltered planes)
            B = [[0] * 21 for _ in range(17)]  # B[r + 1][c + 1], r = -1..15, c = -1..19
            if my == 0:
                B[0] = [127] * 21
            else:
                r = (16 * my - 1) * ys + 16 * mx
                B[0][1:17] = Y[r:r + 16]
                B[0][0] = 129 if mx == 0 else Y[r - 1]
                B[0][17:21] = [Y[r + 15]] * 4 if mx == mbw - 1 else Y[r + 16:r + 20]
            for j in range(16):
                B[j + 1][0] = 129 if mx == 0 else Y[(16 * my + j) * ys + 16 * mx - 1]
            if i4:
                for r in (4, 8, 12):
                    B[r][17:21] = B[0][17:21]
                for k in range(16):
                    pred4(B, 1 + 4 * (k >> 2), 1 + 4 * (k & 3), modes[k])
                    idct_add(coef[16 * k:16 * k + 16], B, 1 + 4 * (k >> 2), 1 + 4 * (k & 3))
            else:
                pred_block(B, 1, 1, 16, modes[0], mx, my)
                for k in range(16):
                    idct_add(coef[16 * k:16 * k + 16], B, 1 + 4 * (k >> 2), 1 + 4 * (k & 3))
            for j in range(16):
                Y[(16 * my + j) * ys + 16 * mx:(16 * my + j) * ys + 16 * mx + 16] = bytes(B[j + 1][1:17])
            for ci, P in enumerate((U, V)):
                B = [[0] * 9 for _ in range(9)]
                if my == 0:
                    B[0] = [127] * 9
                else:
                    r = (8 * my - 1) * uvs + 8 * mx
                    B[0][1:9] = P[r:r + 8]
                    B[0][0] = 129 if mx == 0 else P[r - 1]
                for j in range(8):
                    B[j + 1][0] = 129 if mx == 0 else P[(8 * my + j) * uvs + 8 * mx - 1]
                pred_block(B, 1, 1, 8, uvm, mx, my)
                for k in range(4):
                    at = (16 + 4 * ci + k) * 16
                    idct_add(coef[at:at + 16], B, 1 + 4 * (k >> 1), 1 + 4 * (k & 1))
                for j in range(8):
                    P[(8 * my + j) * uvs + 8 * mx:(8 * my + j) * uvs + 8 * mx + 8] = bytes(B[j + 1][1:9])
    if br.eof or any(p.eof for p in parts):
        cover.add(("hdr", "eof"))
        return FAIL_BITS, None
    if filter_type:
        for my in range(mbh):
            for mx in range(mbw):
                limit, il, hv, inner = finfo[my * mbw + mx]
                filter_mb(Y, U, V, ys, uvs, mx, my, filter_type == 1, limit, il, hv, inner, cover)
    return None, to_rgb(Y, U, V, ys, uvs, w, h)


def decode(data, cover=None):
    """What the library answers with webp_lossy on (and webp off)."""
    cover = set() if cover is None else cover
    h = parse(data)
    if not h["claim"]:
        return Result(CORRUPT, "", 0, 0, None)
    if h["status"] != OK:
        return Result(h["status"], h["why"], 0, 0, None)
    why, rgb = decode_frame(data, h["off"], h["len"], h["width"], h["height"], h["part0"], cover)
    if why:
        return Result(CORRUPT, why, h["width"], h["height"], None)
    return Result(OK, "", h["width"], h["height"], rgb)
