"""Plain restatement of the PNG re-encoder's format under context option
"penc_dynamic" (DESIGN.md "PNG re-encode"), for tests: written from that
format's statement and RFC 1951, not from the kernel or its shared header.

Filtering and the greedy distance-1 parse are ref_penc's.  What changes is the
DEFLATE block: the token list goes out under a Huffman code built from the
image's own histogram (a dynamic block, RFC 1951 3.2.7) when that block is
strictly shorter in bits than the fixed one, and as ref_penc's fixed block
otherwise.

  * histogram f[0..285]: literals by value, matches by length symbol,
    f[256] = 1; distances are not counted
  * code lengths: package-merge, limit 15 (7 for the code-length alphabet),
    leaves ascending by (frequency, symbol), a leaf before a package of equal
    weight -- package_merge() builds the lists as lists
  * canonical codes (3.2.2), MSB first into the LSB-first stream
  * HDIST = 0: one distance code of one bit; a match's distance is the bit 0
  * the HLIT + 257 literal/length lengths and the distance length 1 run-length
    coded as one sequence, greedily (rle())
  * zlib header, Adler-32, the chunks: as ref_penc

A helper module (no fixtures).  read_block() walks either kind of block back
into tokens, so that a test can say which part of two unequal files differs.
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

import ref_penc

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

DynRef = namedtuple("DynRef", "file dyn litlen cllen hdr_bits tokens freq rle body_bits fixed_bits stream")
DynRef.__doc__ = """encode()'s result: the PNG file; whether its block is dynamic; the literal/length code lengths
(286) and the code-length code's lengths (19), as built whether or not the block was chosen; the dynamic header's
bit count; ref_penc.parse's token list [(position, match length or 0)]; the histogram; the run-length tokens
[(symbol, extra value)]; the dynamic and the fixed block's whole length in bits; the filtered stream."""


def histogram(stream, tokens):
    f = [0] * 286
    for pos, k in tokens:
        f[ref_penc.length_symbol(k)[0] if k else int(stream[pos])] += 1
    f[256] = 1
    return f


def package_merge(freq, limit):
    """Code lengths (one per entry of freq, 0 where the frequency is 0), none above limit."""
    leaves = sorted((fr, s) for s, fr in enumerate(freq) if fr > 0)
    n = len(leaves)
    lens = [0] * len(freq)
    if n == 0:
        return lens
    if n == 1:
        lens[leaves[0][1]] = 1
        return lens
    # a list of items: weights, and per item how often it contains each leaf (a row of `holds`)
    leaf_w = np.array([fr for fr, _ in leaves], np.int64)
    leaf_holds = np.eye(n, dtype=np.int64)
    weight, holds = leaf_w, leaf_holds
    for _ in range(2, limit + 1):
        m = len(weight) // 2  # an odd last item is dropped
        pkg_w = weight[0:2 * m:2] + weight[1:2 * m:2]
        pkg_holds = holds[0:2 * m:2] + holds[1:2 * m:2]
        w = np.concatenate([leaf_w, pkg_w])
        is_pkg = np.concatenate([np.zeros(n, np.int64), np.ones(m, np.int64)])
        # a stable sort by (weight, leaf before package): leaves keep their order, packages theirs
        order = np.lexsort((np.arange(n + m), is_pkg, w))
        weight, holds = w[order], np.concatenate([leaf_holds, pkg_holds])[order]
    count = holds[:2 * n - 2].sum(axis=0)
    for (_, s), c in zip(leaves, count.tolist()):
        lens[s] = c
    return lens


def canonical(lens):
    """RFC 1951 3.2.2: {symbol: (code, length)} for the lengths that are not 0."""
    count = [0] * (max(lens) + 2)
    for n in lens:
        if n:
            count[n] += 1
    code, nxt = 0, [0] * (max(lens) + 2)
    for bits in range(1, max(lens) + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def rle(seq):
    """[(symbol 0..18, extra value)] of a sequence of code lengths."""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                c = min(r, 138)
                out.append((18, c - 11))
                r -= c
            if r >= 3:
                out.append((17, r - 3))
                r = 0
            out += [(0, 0)] * r
        else:
            out.append((v, 0))
            r -= 1
            while r >= 3:
                c = min(r, 6)
                out.append((16, c - 3))
                r -= c
            out += [(v, 0)] * r
    return out


_EXTRA_BITS = {16: 2, 17: 3, 18: 7}


class _Bits:
    def __init__(self):
        self.vals, self.lens = [], []

    def put(self, v, n):
        """n bits of v, least significant first"""
        self.vals.append(v)
        self.lens.append(n)

    def code(self, c):
        """a Huffman code (value, length): from its most significant bit"""
        v, n = c
        self.put(int(format(v, "0%db" % n)[::-1], 2), n)

    def nbits(self):
        return int(sum(self.lens))

    def tobytes(self):
        vals, lens = np.asarray(self.vals, np.uint64), np.asarray(self.lens, np.int64)
        total = int(lens.sum())
        start = np.cumsum(lens) - lens
        which = np.repeat(np.arange(len(lens)), lens)
        bit = (np.arange(total) - start[which]).astype(np.uint64)
        bits = ((vals[which] >> bit) & np.uint64(1)).astype(np.uint8)
        return np.packbits(bits, bitorder="little").tobytes()


def header(litlen):
    """(bit writer holding the dynamic block's header, code-length lengths, run-length tokens, HLIT + 257)"""
    top = max(s for s in range(286) if litlen[s])
    nlit = max(257, top + 1)
    toks = rle(list(litlen[:nlit]) + [1])
    clfreq = [0] * 19
    for s, _ in toks:
        clfreq[s] += 1
    cllen = package_merge(clfreq, 7)
    clcode = canonical(cllen)
    last = max(i for i, s in enumerate(CL_ORDER) if cllen[s])
    nclen = max(4, last + 1)
    b = _Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(nlit - 257, 5)
    b.put(0, 5)
    b.put(nclen - 4, 4)
    for s in CL_ORDER[:nclen]:
        b.put(cllen[s], 3)
    for s, x in toks:
        b.code(clcode[s])
        if s >= 16:
            b.put(x, _EXTRA_BITS[s])
    return b, cllen, toks, nlit


def deflate(stream):
    """(deflate bytes, dyn, litlen, cllen, header bits, tokens, freq, rle tokens, dynamic bits, fixed bits)"""
    s = np.asarray(stream, np.uint8).reshape(-1)
    tokens = ref_penc.parse(s)
    freq = histogram(s, tokens)
    litlen = package_merge(freq, 15)
    b, cllen, toks, _ = header(litlen)
    hdr_bits = b.nbits()
    # every code turned round once (MSB first into the LSB-first stream), as _Bits.code would per token
    code = {sym: (ref_penc._rev(v, n), n) for sym, (v, n) in canonical(litlen).items()}
    fixed_bits = 3
    sl = s.tolist()
    for pos, k in tokens:
        if k:
            sym, eb, ev = ref_penc.length_symbol(k)
            b.put(*code[sym])
            if eb:
                b.put(ev, eb)
            b.put(0, 1)  # the one distance code
            fixed_bits += ref_penc._FIXED[sym][1] + eb + 5
        else:
            b.put(*code[sl[pos]])
            fixed_bits += ref_penc._FIXED[sl[pos]][1]
    b.put(*code[256])
    fixed_bits += 7
    dyn_bits = b.nbits()
    dyn = dyn_bits < fixed_bits
    body = b.tobytes() if dyn else ref_penc.deflate_fixed(s)[0]
    return body, dyn, litlen, cllen, hdr_bits, tokens, freq, toks, dyn_bits, fixed_bits


def encode(arr):
    """The PNG file of an H x W x C uint8 array (C = 1..4) with the option on, and what went into it: a DynRef."""
    arr = np.ascontiguousarray(arr, np.uint8)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    h, w, c = arr.shape
    _, rows = ref_penc.filter_rows(arr)
    stream = rows.reshape(-1)
    body, dyn, litlen, cllen, hdr_bits, tokens, freq, toks, dyn_bits, fixed_bits = deflate(stream)
    z = b"\x78\x01" + body + struct.pack(">I", zlib.adler32(stream.tobytes()) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c], 0, 0, 0)
    ch = ref_penc._chunk
    data = b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", ihdr) + ch(b"IDAT", z) + ch(b"IEND", b"")
    return DynRef(data, dyn, litlen, cllen, hdr_bits, tokens, freq, toks, dyn_bits, fixed_bits, stream)


# ------------------------------------------------------------------ a reader, for saying what differs

Block = namedtuple("Block", "dyn hlit hdist hclen cllen litlen distlen hdr_bits tokens bits")
Block.__doc__ = """What read_block() found: the block type; for a dynamic block the header fields (counts, not
field values: 257.., 1.., 4..), the three length arrays and the header's bit count; the tokens as
[(position, match length or 0)] with the literal bytes in `stream` order; the block's length in bits."""


def idat_deflate(png):
    """The raw DEFLATE bytes of a one-IDAT PNG file."""
    pos = 8
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        if png[pos + 4:pos + 8] == b"IDAT":
            return png[pos + 8 + 2:pos + 8 + n - 4]
        pos += 12 + n
    raise ValueError("no IDAT")


def _decoder(lens):
    return {(n, c): s for s, (c, n) in canonical(lens).items()}


def read_block(body):
    """One final block (fixed or dynamic) whose matches are all at distance 1 -> (Block, the bytes it holds)."""
    bits = np.unpackbits(np.frombuffer(body, np.uint8), bitorder="little").tolist()
    at = [0]

    def take(n):
        v = 0
        for i in range(n):
            v |= bits[at[0] + i] << i
        at[0] += n
        return v

    def sym(dec):
        c = n = 0
        while True:
            c = (c << 1) | bits[at[0]]
            at[0] += 1
            n += 1
            if (n, c) in dec:
                return dec[(n, c)]
            assert n < 16, "no code matches"

    assert take(1) == 1, "BFINAL"
    btype = take(2)
    assert btype in (1, 2), btype
    if btype == 1:
        litlen = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
        distlen, cllen, hlit, hdist, hclen = [5] * 30, None, 288, 30, 0
    else:
        hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
        cllen = [0] * 19
        for s in CL_ORDER[:hclen]:
            cllen[s] = take(3)
        dec, seq = _decoder(cllen), []
        while len(seq) < hlit + hdist:
            s = sym(dec)
            if s < 16:
                seq.append(s)
            elif s == 16:
                seq += [seq[-1]] * (3 + take(2))
            else:
                seq += [0] * (3 + take(3) if s == 17 else 11 + take(7))
        assert len(seq) == hlit + hdist, "a run passes the end of the lengths"
        litlen, distlen = seq[:hlit], seq[hlit:]
    hdr_bits = at[0]
    lit = _decoder(litlen)
    dist = _decoder(distlen) if sum(1 for n in distlen if n) > 1 else {(1, 0): 0}
    out, tokens = bytearray(), []
    while True:
        s = sym(lit)
        if s == 256:
            break
        if s < 256:
            tokens.append((len(out), 0))
            out.append(s)
            continue
        base, eb = ref_penc._LEN_BASE[s - 257], ref_penc._LEN_EXTRA[s - 257]
        k = base + take(eb)
        assert sym(dist) == 0, "a distance other than 1"
        tokens.append((len(out), k))
        out += bytes([out[-1]]) * k
    return Block(btype == 2, hlit, hdist, hclen, cllen, litlen, distlen, hdr_bits, tokens, at[0]), bytes(out)


def explain_difference(got, exp):
    """A sentence on where two PNG files of the same pixels part: for failure messages."""
    if got == exp:
        return "equal"
    try:
        g, gb = read_block(idat_deflate(got))
        e, eb = read_block(idat_deflate(exp))
    except Exception as err:  # the reader could not walk one of them: say so
        return f"unreadable block ({type(err).__name__}: {err})"
    if g.dyn != e.dyn:
        return f"block type: dynamic={g.dyn} against the reference's dynamic={e.dyn}"
    for name in ("hlit", "hdist", "hclen", "cllen", "litlen", "distlen", "hdr_bits", "tokens", "bits"):
        if getattr(g, name) != getattr(e, name):
            a, b = getattr(g, name), getattr(e, name)
            if isinstance(a, list) and isinstance(b, list):
                i = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
                return f"{name} differs from entry {i}: {a[i:i + 4]} against {b[i:i + 4]}"
            return f"{name}: {a} against {b}"
    if gb != eb:
        return "the blocks read alike but hold different bytes"
    return "the blocks read alike: the difference is outside the DEFLATE block (padding bits, Adler-32, chunks)"
