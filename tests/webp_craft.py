"""webp_craft.py: a bit writer that emits VP8L (lossless WebP) files from explicit
choices: the transform list in any order with given sub-images, the cache bits
and the prefix image, per code either given lengths or the simple form, and an
explicit symbol stream.  The role gif_craft.py plays for GIF.

Low level:  BitWriter, simple_code / normal_code (-> Enc), write_image
High level: vp8l(width, height, ...) -> chunk payload; forward(pixels, ...) turns
            target ARGB pixels plus a transform list into residuals and specs
Container:  chunk, riff, simple_file, extended_file
"""
import struct

import ref_webp as R


class BitWriter:
    def __init__(self):
        self.v = 0
        self.n = 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.v |= v << self.n
        self.n += n

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


# ------------------------------------------------------------ prefix codes

class Enc:
    """Canonical codes of a length list (or a single symbol that costs no bits)."""

    def __init__(self, lens):
        used = [s for s, l in enumerate(lens) if l]
        self.single = len(used) == 1
        self.codes = {}
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        nxt, c = [0] * 16, 0
        for l in range(1, 16):
            c = (c + count[l - 1]) << 1
            nxt[l] = c
        for s, l in enumerate(lens):
            if l:
                self.codes[s] = (R._rev(nxt[l], l), l)
                nxt[l] += 1

    def put(self, w, s):
        if self.single:
            return
        c = self.codes.get(s)  # (a refusal's broken code may lack the symbol or overflow its length)
        if c:
            w.put(c[0] & ((1 << c[1]) - 1), c[1])


def flat_lens(symbols, alphabet):
    """Lengths of a complete code over `symbols` (two lengths at most)."""
    symbols = sorted(set(symbols))
    lens = [0] * alphabet
    n = len(symbols)
    if n == 1:
        lens[symbols[0]] = 1
        return lens
    L = (n - 1).bit_length()
    short = (1 << L) - n
    for i, s in enumerate(symbols):
        lens[s] = L - 1 if i < short else L
    return lens


def simple_code(w, syms, alphabet=256):
    """The 1- or 2-symbol form."""
    w.put(1, 1)
    w.put(len(syms) - 1, 1)
    if syms[0] < 2:
        w.put(0, 1)
        w.put(syms[0], 1)
    else:
        w.put(1, 1)
        w.put(syms[0], 8)
    if len(syms) == 2:
        w.put(syms[1], 8)
    lens = [0] * max(alphabet, 256)
    for s in syms:
        lens[s] = 1
    return Enc(lens)


DEFAULT_CL = [4] * 16 + [0, 0, 0]  # lengths 0..15 at four bits each, no repeat codes


def normal_code(w, lens, cl_lens=None, cl_stream=None, max_symbol=None, num_cl=19):
    """The normal form.  cl_lens: the code-length code's 19 lengths; cl_stream: the
    code-length symbols as (symbol, extra) pairs (default: one per length);
    max_symbol: written when given (counts code-length symbols read)."""
    cl_lens = list(cl_lens or DEFAULT_CL)
    w.put(0, 1)
    w.put(num_cl - 4, 4)
    for i in range(num_cl):
        w.put(cl_lens[R.CODE_LENGTH_ORDER[i]], 3)
    e = Enc(cl_lens)
    if cl_stream is None:
        cl_stream = [(l, 0) for l in lens]
    if max_symbol is None:
        w.put(0, 1)
    else:
        nb = max(2, ((max_symbol - 2).bit_length() + 1) // 2 * 2)
        w.put(1, 1)
        w.put((nb - 2) // 2, 3)
        w.put(max_symbol - 2, nb)
    for s, extra in cl_stream:
        e.put(w, s)
        if s >= 16:
            w.put(extra, (2, 3, 7)[s - 16])
    return Enc(lens)


def put_code(w, spec, alphabet):
    """spec: ("simple", [syms]) | ("lens", lens, {normal_code options}) | [symbols used] (a flat code)."""
    if isinstance(spec, tuple) and spec[0] == "simple":
        return simple_code(w, spec[1], alphabet)
    if isinstance(spec, tuple) and spec[0] == "lens":
        lens = list(spec[1]) + [0] * (alphabet - len(spec[1]))
        return normal_code(w, lens, **(spec[2] if len(spec) > 2 else {}))
    syms = sorted(set(spec))
    if len(syms) <= 2 and all(s < 256 for s in syms):
        return simple_code(w, syms, alphabet)
    return normal_code(w, flat_lens(syms, alphabet))


def prefix_encode(v):
    d = v - 1
    if d < 4:
        return d, 0, 0
    hi = d.bit_length() - 1
    nb = hi - 1
    return 2 * hi + ((d >> nb) & 1), nb, d & ((1 << nb) - 1)


# ------------------------------------------------------------ an entropy-coded image

def used_symbols(ops, ngroups, meta, meta_bits, width):
    """Per group the symbols each of the five codes needs for `ops`."""
    use = [[set() for _ in range(5)] for _ in range(ngroups)]
    mw = (width + (1 << meta_bits) - 1) >> meta_bits if meta else 0
    pos = 0
    for op in ops:
        x, y = pos % width, pos // width
        u = use[meta[(y >> meta_bits) * mw + (x >> meta_bits)] if meta else 0]
        if op[0] == "px":
            p = op[1]
            u[0].add((p >> 8) & 255), u[1].add((p >> 16) & 255), u[2].add(p & 255), u[3].add(p >> 24)
            pos += 1
        elif op[0] == "copy":
            u[0].add(256 + prefix_encode(op[1])[0]), u[4].add(prefix_encode(op[2])[0])
            pos += op[1]
        else:
            u[0].add(280 + op[1])
            pos += 1
    return use


def write_image(w, width, ops, cache_bits=0, meta=None, meta_bits=0, groups=None, level0=False, cache_field=None):
    """ops: ("px", argb) | ("copy", length, plane_code) | ("cache", key).  groups: per group five code
    specs (None: flat codes over the symbols used).  cache_field: the raw 4-bit field when it is to lie."""
    if cache_bits or cache_field is not None:
        w.put(1, 1)
        w.put(cache_bits if cache_field is None else cache_field, 4)
    else:
        w.put(0, 1)
    ngroups = (max(meta) + 1) if meta else 1
    if level0:
        if meta:
            w.put(1, 1)
            w.put(meta_bits - 2, 3)
            write_image(w, (width + (1 << meta_bits) - 1) >> meta_bits, [("px", 0xFF000000 | (g << 8)) for g in meta])
        else:
            w.put(0, 1)
    use = used_symbols(ops, ngroups, meta, meta_bits, width)
    sizes = (280 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    encs = []
    for g in range(ngroups):
        specs = groups[g] if groups and groups[g] else [None] * 5
        encs.append([put_code(w, specs[k] if specs[k] is not None else (sorted(use[g][k]) or [0]), sizes[k]) for k in range(5)])
    mw = (width + (1 << meta_bits) - 1) >> meta_bits if meta else 0
    pos = 0
    for op in ops:
        x, y = pos % width, pos // width
        e = encs[meta[(y >> meta_bits) * mw + (x >> meta_bits)] if meta else 0]
        if op[0] == "px":
            p = op[1]
            e[0].put(w, (p >> 8) & 255), e[1].put(w, (p >> 16) & 255), e[2].put(w, p & 255), e[3].put(w, p >> 24)
            pos += 1
        elif op[0] == "copy":
            s, nb, ex = prefix_encode(op[1])
            e[0].put(w, 256 + s)
            w.put(ex, nb)
            s, nb, ex = prefix_encode(op[2])
            e[4].put(w, s)
            w.put(ex, nb)
            pos += op[1]
        else:
            e[0].put(w, 280 + op[1])
            pos += 1


def literals(pixels):
    return [("px", int(p)) for p in pixels]


# ------------------------------------------------------------ forward transforms

def _sub(a, b):
    return (((a | 0x00FF00FF) - (b & 0xFF00FF00)) & 0xFF00FF00) | (((a | 0xFF00FF00) - (b & 0x00FF00FF)) & 0x00FF00FF)


def forward(px, width, height, transforms):
    """px: ARGB list.  transforms, in the order they are written:
      ("predictor", bits, modes per block) ("color", bits, (g2r, g2b, r2b) per block) ("green",)
      ("index", table)   (every pixel must be in the table)
    -> (residual pixels, their width, the specs vp8l() takes)."""
    px = list(px)
    specs = []
    w = width
    for t in transforms:
        if t[0] == "predictor":
            bits, modes = t[1], t[2]
            bw = (w + (1 << bits) - 1) >> bits
            out = [0] * len(px)
            for y in range(height):
                for x in range(w):
                    i = y * w + x
                    if y == 0:
                        pr = 0xFF000000 if x == 0 else px[i - 1]
                    elif x == 0:
                        pr = px[i - w]
                    else:
                        pr = R.predict(modes[(y >> bits) * bw + (x >> bits)], px[i - 1], px[i - w], px[i - w - 1], px[i - w + 1])
                    out[i] = _sub(px[i], pr)
            px = out
            specs.append((R.T_PREDICTOR, bits, [0xFF000000 | (m << 8) for m in modes]))
        elif t[0] == "color":
            bits, ms = t[1], t[2]
            bw = (w + (1 << bits) - 1) >> bits
            out = []
            for i, p in enumerate(px):
                g2r, g2b, r2b = ms[((i // w) >> bits) * bw + ((i % w) >> bits)]
                g, r = (p >> 8) & 255, (p >> 16) & 255
                out.append((p & 0xFF00FF00) | (((r - R._delta(g2r, g)) & 255) << 16) | ((p - R._delta(g2b, g) - R._delta(r2b, r)) & 255))
            px = out
            specs.append((R.T_COLOR, bits, [0xFF000000 | (r2b << 16) | (g2b << 8) | g2r for g2r, g2b, r2b in ms]))
        elif t[0] == "green":
            px = [(p & 0xFF00FF00) | ((((p >> 16) - (p >> 8)) & 255) << 16) | ((p - (p >> 8)) & 255) for p in px]
            specs.append((R.T_GREEN,))
        else:
            table = list(t[1]) if t[1] is not None else sorted(set(px))  # None: whatever the pixels are by now
            bits = R.index_bits(len(table))
            bpp = 8 >> bits
            pw = (w + (1 << bits) - 1) >> bits
            out = [0xFF000000] * (pw * height)
            for y in range(height):
                for x in range(w):
                    out[y * pw + (x >> bits)] |= table.index(px[y * w + x]) << (8 + (x & ((1 << bits) - 1)) * bpp)
            px = out
            specs.append((R.T_INDEX, table))
            w = pw
    return px, w, specs


def vp8l(width, height, alpha=1, transforms=(), ops=None, cache_bits=0, meta=None, meta_bits=0, groups=None,
         version=0, cache_field=None, raw_index_size=None):
    """-> the VP8L chunk's payload.  transforms: specs as forward() returns them, written in order;
    ops address the image at its final (packed) width."""
    w = BitWriter()
    w.put(0x2F, 8)
    w.put(width - 1, 14)
    w.put(height - 1, 14)
    w.put(alpha, 1)
    w.put(version, 3)
    xs = width
    for t in transforms:
        w.put(1, 1)
        w.put(t[0], 2)
        if t[0] in (R.T_PREDICTOR, R.T_COLOR):
            w.put(t[1] - 2, 3)
            write_image(w, (xs + (1 << t[1]) - 1) >> t[1], literals(t[2]))
        elif t[0] == R.T_INDEX:
            table = t[1]
            w.put(len(table) - 1, 8)
            write_image(w, len(table), literals([_sub(p, table[i - 1]) if i else p for i, p in enumerate(table)]))
            bits = R.index_bits(len(table))
            xs = (xs + (1 << bits) - 1) >> bits
    w.put(0, 1)
    write_image(w, xs, ops, cache_bits, meta, meta_bits, groups, level0=True, cache_field=cache_field)
    return w.bytes()


# ------------------------------------------------------------ container

def chunk(cc, body):
    return cc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def riff(chunks):
    body = b"WEBP" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def simple_file(payload):
    return riff([chunk(b"VP8L", payload)])


def vp8x(width, height, alpha=0, anim=0, icc=0, exif=0):
    flags = (0x10 if alpha else 0) | (0x02 if anim else 0) | (0x20 if icc else 0) | (0x08 if exif else 0)
    return chunk(b"VP8X", bytes([flags, 0, 0, 0]) + (width - 1).to_bytes(3, "little") + (height - 1).to_bytes(3, "little"))


def extended_file(payload, width, height, alpha=0, before=(), after=(), **kw):
    return riff([vp8x(width, height, alpha, **kw)] + list(before) + [chunk(b"VP8L", payload)] + list(after))
