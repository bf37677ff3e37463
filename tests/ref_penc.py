"""Plain restatement of the PNG re-encoder's format (datago_amd/csrc/dg_penc.hip),
for tests: written from the PNG specification and RFC 1950 / 1951 plus the
choices the kernel file's header comment documents, not from the kernel code.

  * signature, IHDR (8-bit; colour type 0 / 4 / 2 / 6 for 1 / 2 / 3 / 4 channels)
  * per row the five filters (spec 9.2); the one with the smallest sum of
    |byte as int8| is kept (spec 12.8), a tie going to the lower type
  * the filtered stream as ONE fixed-Huffman block (RFC 1951 3.2.6): a greedy
    parse whose only matches are at distance 1 (a byte repeated), 3..258
    long; the parse restarts at every 1 KiB of the stream (a match never
    crosses such an edge, but may begin on it, pointing at the byte before),
    and the stream's first byte is always a literal
  * bits LSB-first, a 7-bit end-of-block, zlib header 78 01, Adler-32
  * one IDAT chunk, IEND

A helper module (no fixtures).  encode() loops in Python over the stream: it
is meant for images of a few hundred KB at the most.
"""
import binascii
import struct
import zlib
from collections import namedtuple

import numpy as np

PIECE = 1024

# RFC 1951 3.2.5: length symbols 257..285 -> (base length, extra bits)
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]

Ref = namedtuple("Ref", "file filters len_syms stream matches cn")
Ref.__doc__ = """encode()'s result: the PNG file, the filter type of every row, the length symbols
(257..285) in stream order, the filtered stream, the matches as (stream position, length), and the
number of bytes under the IDAT chunk's CRC (4 + the zlib stream)."""


def length_symbol(n):
    """(symbol, extra bits, extra value) of a match length 3..258; 258 is symbol 285."""
    assert 3 <= n <= 258
    for i in range(28, -1, -1):
        if n >= _LEN_BASE[i]:
            return 257 + i, _LEN_EXTRA[i], n - _LEN_BASE[i]


def _rev(code, n):
    return int(format(code, "0%db" % n)[::-1], 2)


def _fixed_code(sym):
    """RFC 1951 3.2.6, as (value to put LSB-first, bits): Huffman codes are packed from their MSB."""
    if sym < 144:
        return _rev(0x30 + sym, 8), 8
    if sym < 256:
        return _rev(0x190 + sym - 144, 9), 9
    if sym < 280:
        return _rev(sym - 256, 7), 7
    return _rev(0xC0 + sym - 280, 8), 8


_FIXED = [_fixed_code(s) for s in range(288)]


def filter_rows(arr):
    """(filter type per row, filtered stream H x (1 + row bytes)) of an H x W x C uint8 array."""
    h, w, c = arr.shape
    rb = w * c
    x = arr.reshape(h, rb).astype(np.int32)
    a = np.zeros_like(x)
    a[:, c:] = x[:, :-c] if rb > c else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, c:] = x[:-1, :-c] if rb > c else 0
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 0xFF  # 5 x H x rb
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)  # |i8|; -128 counts 128
    types = np.argmin(cost, axis=0)  # the first minimum: ties go to the lower type
    out = np.empty((h, rb + 1), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(h)]
    return types.astype(np.uint8), out


def parse(stream):
    """Greedy parse of the filtered stream: [("lit", byte) | ("match", length)] with stream positions."""
    s = stream.tolist() if isinstance(stream, np.ndarray) else list(stream)
    n = len(s)
    # ahead[i]: how many bytes from i on equal the byte before them
    eq = np.zeros(n + 1, np.int64)
    if n > 1:
        arr = np.asarray(s, np.int64)
        eq[1:n] = arr[1:] == arr[:-1]
    ahead = np.zeros(n + 1, np.int64)
    idx = np.flatnonzero(eq[:n] == 0)  # positions that break a run
    nxt = np.searchsorted(idx, np.arange(n), side="left")
    brk = np.where(nxt < len(idx), idx[np.minimum(nxt, len(idx) - 1)], n)
    ahead[:n] = brk - np.arange(n)
    ahead = ahead.tolist()
    out = []
    i = 0
    while i < n:
        edge = (i // PIECE + 1) * PIECE
        k = min(ahead[i], 258, edge - i, n - i) if i > 0 else 0
        if k >= 3:
            out.append((i, k))
            i += k
        else:
            out.append((i, 0))
            i += 1
    return out


def deflate_fixed(stream):
    """(deflate bytes, length symbols, matches) of the stream under parse()."""
    s = np.asarray(stream, np.uint8).reshape(-1)
    toks = parse(s)
    sl = s.tolist()
    vals, lens, syms, matches = [3], [3], [], []  # BFINAL = 1, BTYPE = 01: bits 1, 1, 0
    for pos, k in toks:
        if k:
            sym, eb, ev = length_symbol(k)
            syms.append(sym)
            matches.append((pos, k))
            v, n = _FIXED[sym]
            vals.append(v)
            lens.append(n)
            if eb:
                vals.append(ev)
                lens.append(eb)
            vals.append(0)  # distance code 0 = distance 1: five bits, no extra
            lens.append(5)
        else:
            v, n = _FIXED[sl[pos]]
            vals.append(v)
            lens.append(n)
    vals.append(0)  # end of block: symbol 256, seven zero bits
    lens.append(7)
    vals, lens = np.asarray(vals, np.uint32), np.asarray(lens, np.int64)
    total = int(lens.sum())
    start = np.cumsum(lens) - lens
    which = np.repeat(np.arange(len(lens)), lens)
    bit = np.arange(total) - start[which]
    bits = ((vals[which] >> bit.astype(np.uint32)) & 1).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes(), syms, matches


def _chunk(t, body):
    return struct.pack(">I", len(body)) + t + body + struct.pack(">I", binascii.crc32(t + body) & 0xFFFFFFFF)


def encode(arr):
    """The PNG file of an H x W x C uint8 array (C = 1..4) and what went into it: a Ref."""
    arr = np.ascontiguousarray(arr, np.uint8)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    h, w, c = arr.shape
    types, rows = filter_rows(arr)
    stream = rows.reshape(-1)
    body, syms, matches = deflate_fixed(stream)
    z = b"\x78\x01" + body + struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c], 0, 0, 0)
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", z) + _chunk(b"IEND", b"")
    return Ref(data, types, syms, stream, matches, 4 + len(z))
