"""Plain restatement of the PNG re-encoder's format under context option
"penc_match" (DESIGN.md "Matches (option penc_match)"), for tests: written from
that section's list and RFC 1951, not from the kernels.

Filtering is ref_penc's.  The stream is parsed a second time with LZ77 matches:

  * pieces of 1,024 bytes; a match ends inside its piece; its source may lie up
    to 7,168 bytes before the piece's start (ws)
  * H(q) = (le32(s[q..q+4)) * 0x9E3779B1 mod 2^32) >> 20 where q + 3 < N; the
    table keeps the largest inserted q per hash; [ws, p0) is inserted first
  * the piece goes in groups of 64 positions: the whole group looks up, then
    the whole group is inserted
  * at p, lim = min(258, p1 - p): distances 1, C, 2C (ascending, p - d >= 0), a
    length >= 3 that beats the best so far; then the table's q, a length >= 6
    that is >= best + 2; nothing where lim < 3
  * greedy from p0
  * the block: one final block, fixed (5-bit distance codes) or dynamic (both
    alphabets by package-merge, L = 15; HDIST = highest used distance symbol;
    the lengths of both run-length coded as one sequence)
  * the choice: parent tokens fixed, parent tokens dynamic, match tokens fixed,
    match tokens dynamic -- the shortest in bits, the earlier on a tie; without
    "penc_dynamic" only the two fixed blocks stand

A helper module (no fixtures).
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

import ref_penc
import ref_penc_dyn as D

PIECE, WINDOW, GROUP = 1024, 7168, 64
FAR_MIN, FAR_MARGIN = 6, 2
PARENT_FIXED, PARENT_DYN, MATCH_FIXED, MATCH_DYN = range(4)

# RFC 1951 3.2.5: distance symbols 0..29 -> base distance; extra bits
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
              4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]

MatchRef = namedtuple("MatchRef", "file which tokens bits litlen distlen hdr_bits lit_freq dist_freq stream")
MatchRef.__doc__ = """encode()'s result: the PNG file; which block won (PARENT_FIXED .. MATCH_DYN); the match parse
[(position, length or 0, distance)]; the four blocks' lengths in bits (None: not a candidate); the match tokens'
code lengths and the dynamic header's bit count (None without "penc_dynamic" or without a match); the two
histograms; the filtered stream."""


def distance_symbol(d):
    """(symbol, extra bits, extra value) of a distance 1..32768."""
    sym = max(i for i in range(30) if _DIST_BASE[i] <= d)
    return sym, _DIST_EXTRA[sym], d - _DIST_BASE[sym]


def _hash(s, q):
    return ((int.from_bytes(s[q:q + 4], "little") * 0x9E3779B1) & 0xFFFFFFFF) >> 20


def _common(s, a, b, lim):
    """How many of s[a..a+lim) equal s[b..b+lim) from the front."""
    if s[a] != s[b]:
        return 0
    lo, hi = 1, lim  # s[a..a+lo) equals s[b..b+lo); bisect for the longest such lo
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if s[a + lo:a + mid] == s[b + lo:b + mid]:
            lo = mid
        else:
            hi = mid - 1
    return lo


def parse(stream, c):
    """[(position, match length or 0, distance or 0)] of the filtered stream, C = c bytes per pixel."""
    s = bytes(stream)
    n = len(s)
    near = sorted({1, c, 2 * c})
    out = []
    for p0 in range(0, n, PIECE):
        p1, ws = min(p0 + PIECE, n), max(0, p0 - WINDOW)
        table = {}
        for q in range(ws, p0):
            if q + 3 < n:
                table[_hash(s, q)] = q
        best = {}
        for g0 in range(p0, p1, GROUP):
            group = [p for p in range(g0, min(g0 + GROUP, p1))]
            far = {p: table.get(_hash(s, p)) for p in group if p + 3 < n}
            for p in group:
                if p + 3 < n:
                    table[_hash(s, p)] = p
            for p in group:
                lim, k, d = min(258, p1 - p), 0, 0
                if lim < 3:
                    continue
                for dd in near:
                    if p - dd >= 0:
                        kk = _common(s, p, p - dd, lim)
                        if kk >= 3 and kk > k:
                            k, d = kk, dd
                q = far.get(p)
                if q is not None:
                    kk = _common(s, p, q, lim)
                    if kk >= FAR_MIN and kk >= k + FAR_MARGIN:
                        k, d = kk, p - q
                if k:
                    best[p] = (k, d)
        p = p0
        while p < p1:
            k, d = best.get(p, (0, 0))
            out.append((p, k, d))
            p += k or 1
    return out


def histograms(s, tokens):
    lit, dist = [0] * 286, [0] * 30
    for pos, k, d in tokens:
        if k:
            lit[ref_penc.length_symbol(k)[0]] += 1
            dist[distance_symbol(d)[0]] += 1
        else:
            lit[s[pos]] += 1
    lit[256] = 1
    return lit, dist


def header(litlen, distlen):
    """(bit writer holding the dynamic block's header, code-length lengths, HLIT + 257, HDIST + 1)"""
    nlit = max(257, max(s for s in range(286) if litlen[s]) + 1)
    ndist = max(s for s in range(30) if distlen[s]) + 1
    toks = D.rle(list(litlen[:nlit]) + list(distlen[:ndist]))
    clfreq = [0] * 19
    for s, _ in toks:
        clfreq[s] += 1
    cllen = D.package_merge(clfreq, 7)
    clcode = D.canonical(cllen)
    nclen = max(4, max(i for i, s in enumerate(D.CL_ORDER) if cllen[s]) + 1)
    b = D._Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(nlit - 257, 5)
    b.put(ndist - 1, 5)
    b.put(nclen - 4, 4)
    for s in D.CL_ORDER[:nclen]:
        b.put(cllen[s], 3)
    for s, x in toks:
        b.code(clcode[s])
        if s >= 16:
            b.put(x, D._EXTRA_BITS[s])
    return b, cllen, nlit, ndist


def _write(b, s, tokens, lit, dist):
    """The tokens and the end-of-block under {symbol: (value to put LSB-first, bits)} for both alphabets."""
    for pos, k, d in tokens:
        if k:
            sym, eb, ev = ref_penc.length_symbol(k)
            b.put(*lit[sym])
            if eb:
                b.put(ev, eb)
            sym, eb, ev = distance_symbol(d)
            b.put(*dist[sym])
            if eb:
                b.put(ev, eb)
        else:
            b.put(*lit[s[pos]])
    b.put(*lit[256])
    return b


def _turned(lens):
    return {sym: (ref_penc._rev(v, n), n) for sym, (v, n) in D.canonical(lens).items()}


_FIXED_LIT = dict(enumerate(ref_penc._FIXED))
_FIXED_DIST = {d: (ref_penc._rev(d, 5), 5) for d in range(30)}


def deflate(stream, c, dynamic):
    """(deflate bytes, which, tokens, bits of the four blocks, litlen, distlen, header bits, histograms)"""
    s = np.asarray(stream, np.uint8).reshape(-1)
    sl = s.tolist()
    tokens = parse(s, c)
    lit_f, dist_f = histograms(sl, tokens)
    bits = [None] * 4
    if dynamic:
        pd = D.deflate(s)
        parent_body, bits[PARENT_DYN], bits[PARENT_FIXED] = pd[0], pd[8], pd[9]
    else:
        parent_body = ref_penc.deflate_fixed(s)[0]
        bits[PARENT_FIXED] = 3 + 7 + sum(ref_penc._FIXED[ref_penc.length_symbol(k)[0]][1] + ref_penc.length_symbol(k)[1]
                                         + 5 if k else ref_penc._FIXED[sl[pos]][1] for pos, k in ref_penc.parse(s))
    litlen = distlen = hdr_bits = None
    blocks = {}
    if any(dist_f):  # without a match the parse is the parent's: no candidate
        fb = D._Bits()
        fb.put(3, 3)
        blocks[MATCH_FIXED] = _write(fb, sl, tokens, _FIXED_LIT, _FIXED_DIST)
        if dynamic:
            litlen, distlen = D.package_merge(lit_f, 15), D.package_merge(dist_f, 15)
            db = header(litlen, distlen)[0]
            hdr_bits = db.nbits()
            blocks[MATCH_DYN] = _write(db, sl, tokens, _turned(litlen), _turned(distlen))
        for k, b in blocks.items():
            bits[k] = b.nbits()
    which = min((k for k in range(4) if bits[k] is not None), key=lambda k: (bits[k], k))
    body = blocks[which].tobytes() if which >= MATCH_FIXED else parent_body
    return body, which, tokens, bits, litlen, distlen, hdr_bits, lit_f, dist_f


def encode_rows(rows, depth, dynamic):
    """The file of H x W x C row bytes (depth 16: C = 2 x samples, high bytes first, as ref_penc16.be_rows)."""
    h, w, c = rows.shape
    _, filtered = ref_penc.filter_rows(rows)
    stream = filtered.reshape(-1)
    body, which, tokens, bits, litlen, distlen, hdr_bits, lit_f, dist_f = deflate(stream, c, dynamic)
    z = b"\x78\x01" + body + struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", w, h, depth, {1: 0, 2: 4, 3: 2, 4: 6}[c * 8 // depth], 0, 0, 0)
    ch = ref_penc._chunk
    data = b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", ihdr) + ch(b"IDAT", z) + ch(b"IEND", b"")
    return MatchRef(data, which, tokens, bits, litlen, distlen, hdr_bits, lit_f, dist_f, stream)


def encode(arr, dynamic):
    """The PNG file of an H x W x C uint8 array (C = 1..4) with the option on, and which block won: a MatchRef."""
    arr = np.ascontiguousarray(arr, np.uint8)
    return encode_rows(arr[:, :, None] if arr.ndim == 2 else arr, 8, dynamic)


def parent(arr, dynamic):
    """The parent's file of the same array: ref_penc_dyn's with "penc_dynamic", ref_penc's without."""
    return D.encode(arr).file if dynamic else ref_penc.encode(arr).file
