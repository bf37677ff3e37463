"""The JPEG re-encoder's per-image Huffman tables (context option
"jenc_optimize") restated: a function from a standard-table file of the
encoder to its optimised twin.  A plain helper module (no GPU, no fixtures).

The table rule is libjpeg's jpeg_gen_optimal_table (T.81 K.2 + K.3 with
jchuff.c's tie-breaks), written out here from DESIGN.md "JPEG re-encode", per
table over that table's symbol counts; luma DC / AC take component 0, chroma
DC / AC components 1 and 2 together.

  K.2  symbols 0..255 carry their counts, a reserved symbol 256 carries 1.
       Until one tree is left: c1 = the least nonzero count, the largest index
       winning ties; c2 = the same over the rest; c2's count goes to c1 and
       every symbol in either tree gets one more bit.
  K.3  bits[n] = symbols of size n (n <= 32); for i = 32 down to 17, while
       bits[i] > 0: j = the largest j <= i - 2 with bits[j] > 0;
       bits[i] -= 2, bits[i-1] += 1, bits[j+1] += 2, bits[j] -= 1.  Then one
       code leaves the largest nonzero length (the reserved symbol's).
  HUFFVAL  for each K.2 size in turn the symbols of that size, ascending;
       canonical codes along that order.
  A K.2 size above 32: the image keeps the standard tables (the file itself).

Everything else in the file stays: the segments in front of the DHTs, four DHT
segments (two for one component) with classes 00 10 01 11, SOS, the scan with
1-bit padding and FF 00 stuffing, EOI.
"""
import struct
from collections import namedtuple

import numpy as np

Table = namedtuple("Table", "bits vals sizes fallback")
Table.__doc__ = "bits[0..16] (BITS), vals (HUFFVAL), sizes: the K.2 sizes of symbols 0..256, fallback: a size > 32"
Twin = namedtuple("Twin", "file hist tables fallback header_len std_header_len")
Twin.__doc__ = """file: the optimised file; hist / tables: {(class, id): 256 counts / Table}; fallback: some table
met a size above 32 (file is then the input); header_len: bytes in front of the scan, std_header_len: the input's"""


def optimal_table(counts):
    cnt = [int(c) for c in counts] + [0] * (256 - len(counts)) + [1]
    assert len(cnt) == 257 and min(cnt) >= 0
    size = [0] * 257
    members = {i: [i] for i in range(257) if cnt[i]}
    while len(members) > 1:
        c1 = min(members, key=lambda i: (cnt[i], -i))
        c2 = min((i for i in members if i != c1), key=lambda i: (cnt[i], -i))
        cnt[c1] += cnt[c2]
        cnt[c2] = 0
        members[c1] += members.pop(c2)
        for s in members[c1]:
            size[s] += 1
    if max(size) > 32:
        return Table(None, None, size, True)
    bits = [0] * 33
    for s in range(257):
        if size[s]:
            bits[size[s]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = max(j for j in range(1, i - 1) if bits[j] > 0)
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    top = max(n for n in range(1, 17) if bits[n])
    bits[top] -= 1
    assert not any(bits[17:])
    vals = [s for _, s in sorted((size[s], s) for s in range(256) if size[s])]
    assert sum(bits[1:17]) == len(vals)
    return Table(bits[:17], vals, size, False)


def canonical(bits, vals):
    """{symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n]):
            out[vals[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    return out


def dht_segment(cls, t):
    body = bytes([cls]) + bytes(t.bits[1:17]) + bytes(t.vals)
    return b"\xff\xc4" + struct.pack(">H", len(body) + 2) + body


def segments(data):
    """[(marker, offset, end)] of the segments between SOI and the scan, SOS included."""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((data[i + 1], i, i + 2 + n))
        i += 2 + n
        if out[-1][0] == 0xDA:
            return out


def symbols(data):
    """The scan's symbol stream [(table key, symbol, value, value bits)] from the file's coefficients."""
    from jpeg_craft import ZIGZAG, _block_symbols
    from oracle import oracle as O
    segs = segments(data)
    sof = next(s for s in segs if s[0] == 0xC0)
    h, w = struct.unpack(">HH", data[sof[1] + 5:sof[1] + 9])
    ncomp = data[sof[1] + 9]
    nb = ((h + 7) // 8) * ((w + 7) // 8) * ncomp
    st, co = O.jpeg_coefs(data, nb + 8)
    assert st == 0 and len(co) == nb, (st, len(co), nb)
    z = np.asarray(co)[:, ZIGZAG].astype(np.int64)
    pred, seq = [0] * ncomp, []
    for b in range(nb):
        c = b % ncomp
        _block_symbols(z[b], pred[c], (0, min(c, 1)), (1, min(c, 1)), seq)
        pred[c] = int(z[b, 0])
    return ncomp, seq


def histograms(ncomp, seq):
    keys = [(0, 0), (1, 0)] + ([(0, 1), (1, 1)] if ncomp == 3 else [])
    hist = {k: [0] * 256 for k in keys}
    for key, sym, _, _ in seq:
        hist[key][sym] += 1
    return hist


def _scan(seq, codes):
    out, acc, n = bytearray(), 0, 0
    for key, sym, v, nb in seq:
        c, m = codes[key][sym]
        acc = acc << m | c
        n += m
        if nb:
            acc = acc << nb | (v if v >= 0 else v + (1 << nb) - 1)
            n += nb
        while n >= 8:
            n -= 8
            out.append(acc >> n)
            acc &= (1 << n) - 1
    if n:
        out.append(acc << (8 - n) | ((1 << (8 - n)) - 1))
    return bytes(out).replace(b"\xff", b"\xff\x00")


def optimise(data):
    """Twin of a standard-table file as the encoder writes it."""
    data = bytes(data)
    segs = segments(data)
    dhts = [s for s in segs if s[0] == 0xC4]
    ncomp, seq = symbols(data)
    hist = histograms(ncomp, seq)
    classes = [0x00, 0x10, 0x01, 0x11][:len(hist)]
    assert [data[s[1] + 4] for s in dhts] == classes  # one table per segment, in the encoder's order
    assert segs[-1][0] == 0xDA and dhts[-1][2] == segs[-1][1] and all(a[2] == b[1] for a, b in zip(dhts, dhts[1:]))
    std_len = segs[-1][2]
    tables = {(cls >> 4, cls & 15): optimal_table(hist[(cls >> 4, cls & 15)]) for cls in classes}
    if any(t.fallback for t in tables.values()):
        return Twin(data, hist, tables, True, std_len, std_len)
    head = data[:dhts[0][1]] + b"".join(dht_segment(cls, tables[(cls >> 4, cls & 15)]) for cls in classes) \
        + data[segs[-1][1]:segs[-1][2]]
    codes = {k: canonical(t.bits, t.vals) for k, t in tables.items()}
    return Twin(head + _scan(seq, codes) + b"\xff\xd9", hist, tables, False, len(head), std_len)
