"""Named edge inputs for the JPEG and PNG re-encoders (pre_encode_images):
pixel arrays built so that the encoders' entropy-coding edges are met on
purpose, each with a property that says which edge, as a predicate over the
REFERENCE's output (oracle.jpeg_encode / tests/ref_penc.py).  The CPU test
(test_encode_edges_cpu.py) asserts the properties, so no GPU comparison made
with these inputs can pass without having met its edge.

A plain helper module (NumPy only, no GPU, no fixtures).  Every seed below was
found by a search on the CPU against the references; the properties re-check
what the search found.

  jpeg_cases() -> [(label, uint8 H x W x C, property)]     C = 1 or 3
      property(facts) with facts = a function quality -> JpegFacts of the
      reference's file of that case at that quality
  JPEG_SET_PROPERTIES: [(name, predicate over {label: facts})] for what only a
      set of cases can show (both classes of an edge are met)
  png_cases()  -> [(label, uint8 H x W x C, property)]     C = 1..4
      property(ref) with ref = ref_penc.encode(array)
  PNG_SET_PROPERTIES: [(name, predicate over {label: ref})]
"""
import struct
from collections import namedtuple

import numpy as np

JPEG_QUALITIES = (1, 50, 75, 100)

_k = np.arange(8)


def basis(u, v):
    """8x8 DCT basis function: vertical frequency u, horizontal v."""
    return np.cos((2 * _k[:, None] + 1) * u * np.pi / 16) * np.cos((2 * _k[None, :] + 1) * v * np.pi / 16)


# ------------------------------------------------------------------ facts about a baseline 4:4:4 / gray JPEG

JpegFacts = namedtuple("JpegFacts", "file ncomp coefs dc_diff ac_max ac_min zrl last_nonzero run_before_63 bits "
                                    "scan_bytes ff00 ends_stuffed rounds nblocks code16_at")
JpegFacts.__doc__ = """What a reference JPEG holds.  coefs: (nblocks, 64) zigzag order, scan order; dc_diff,
ac_max, ac_min: per component lists of the DC differences / the extreme AC values; zrl: ZRL symbols in the scan;
last_nonzero: blocks whose coefficient 63 is not zero (no EOB); run_before_63: the longest zero run in front of
such a coefficient; bits: the scan's length before padding; scan_bytes: the stuffed scan; ff00: stuffed bytes;
ends_stuffed: the file ends FF 00 FF D9; rounds: 4096-byte rounds of the unstuffed scan; code16_at: the scan bit
positions modulo 32 at which a 16-bit Huffman code begins (31: it straddles a word with one bit in it)."""

_ac_len = None


def _code_lengths():
    """Annex K code lengths {(class, id): {symbol: bits}} from the standard tables."""
    global _ac_len
    if _ac_len is None:
        from jpeg_craft import std_tables
        _ac_len = {}
        for key, (bits, vals) in std_tables().items():
            lens, i = {}, 0
            for n in range(1, 17):
                for _ in range(bits[n]):
                    lens[vals[i]] = n
                    i += 1
            _ac_len[key] = lens
    return _ac_len


def jpeg_facts(data, coefs_natural):
    """JpegFacts of an encoder's file and its coefficients as oracle.jpeg_coefs reads them back."""
    from jpeg_craft import ZIGZAG, _block_symbols
    i, ncomp = 2, 0
    while data[i + 1] != 0xDA:
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        if data[i + 1] == 0xC0:
            ncomp = data[i + 9]
        i += 2 + n
    i += 2 + struct.unpack(">H", data[i + 2:i + 4])[0]
    assert data[-2:] == b"\xff\xd9"
    scan = data[i:-2]
    z = np.asarray(coefs_natural)[:, ZIGZAG].astype(np.int64)
    nb = len(z)
    assert ncomp in (1, 3) and nb % ncomp == 0
    lens = _code_lengths()
    bits = zrl = 0
    pred = [0] * ncomp
    dc_diff = [[] for _ in range(ncomp)]
    run63, code16_at = -1, set()
    for b in range(nb):
        c = b % ncomp
        syms = []
        _block_symbols(z[b], pred[c], (0, min(c, 1)), (1, min(c, 1)), syms)
        dc_diff[c].append(int(z[b, 0]) - pred[c])
        pred[c] = int(z[b, 0])
        for key, sym, _, extra in syms:
            if lens[key][sym] == 16:
                code16_at.add(bits % 32)
            bits += lens[key][sym] + extra
            zrl += key[0] == 1 and sym == 0xF0
        if z[b, 63]:
            nz = np.flatnonzero(z[b, 1:63])
            run63 = max(run63, 62 - (int(nz[-1]) + 1 if len(nz) else 0))
    ff00 = scan.count(b"\xff\x00")
    assert scan.count(b"\xff") == ff00  # every FF of the scan is a stuffed one
    assert (bits + 7) // 8 + ff00 == len(scan), ((bits + 7) // 8, ff00, len(scan))
    ac = [z[c::ncomp, 1:] for c in range(ncomp)]
    return JpegFacts(data, ncomp, z, dc_diff, [int(a.max()) for a in ac], [int(a.min()) for a in ac], int(zrl),
                     int(np.count_nonzero(z[:, 63])), run63, bits, scan, ff00, data.endswith(b"\xff\x00\xff\xd9"),
                     ((bits + 7) // 8 + 4095) // 4096, nb, code16_at)


def category(v):
    return int(abs(int(v))).bit_length()


# ------------------------------------------------------------------ JPEG cases

def _tile(blocks, reps=1):
    """8x8 blocks (a list of rows of blocks) as one image; C = 1 or 3 follows from the blocks."""
    return np.concatenate([np.concatenate(row * reps, axis=1) for row in blocks], axis=0)


def _gray(b):
    return np.asarray(b, np.uint8)[:, :, None]


def _red_cyan(mask):
    """RGB block: red where mask, cyan elsewhere (luma moves little, Cr swings fully)."""
    out = np.empty((8, 8, 3), np.uint8)
    out[mask] = (255, 0, 0)
    out[~mask] = (0, 255, 255)
    return out


def _noise(seed, h, w, c, binary=False):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2, (h, w, c)) * 255 if binary else rng.integers(0, 256, (h, w, c))
    return v.astype(np.uint8)


def _low_noise(seed, h, w, c):
    return (128 + np.random.default_rng(seed).integers(-4, 5, (h, w, c))).astype(np.uint8)


# seeds of 8x8 gray uniform noise whose quality-100 file ends FF 00 FF D9 (searched; the property re-checks)
STUFFED_END_SEEDS = (2, 10, 20)
# seed of 8x8 gray uniform noise whose quality-100 scan is a whole number of bytes (no padding)
WHOLE_BYTES_SEED = 11

NOISE_DIMS = (1, 7, 8, 9, 15, 17)


def _true(_f):
    return True


def jpeg_cases():
    cases = []

    # 1. sign-of-basis blocks: one AC coefficient of +-1020 (category 10) at quality 100
    def big_ac(comp):
        def prop(f):
            q = f(100)
            return q.ac_max[comp] >= 512 and q.ac_min[comp] <= -512
        return prop

    for u, v in ((4, 4), (0, 4), (4, 0)):
        pos = basis(u, v) > 0
        a, b = np.where(pos, 0, 255), np.where(pos, 255, 0)
        flat = np.full((8, 8), 128)
        # both polarities, each twice in a row (DC difference 0) and against a flat block
        cases.append((f"basis{u}{v}_gray", _gray(_tile([[a, a, b, b, flat], [b, flat, a, b, a]])), big_ac(0)))
        ra, rb, rf = _red_cyan(pos), _red_cyan(~pos), np.full((8, 8, 3), 128, np.uint8)
        cases.append((f"basis{u}{v}_redcyan", _tile([[ra, ra, rb, rb, rf], [rb, rf, ra, rb, ra]]), big_ac(2)))
        wa, wb = np.repeat(_gray(a), 3, axis=2), np.repeat(_gray(b), 3, axis=2)
        cases.append((f"basis{u}{v}_rgb", _tile([[wa, wb, wb], [wb, wa, wa]]), big_ac(0)))

    # 2. DC differences of +-2040 (category 11); flat images: EOB-only blocks
    def big_dc(f):
        d = f(100).dc_diff[0]
        return max(d) == 2040 and min(d) == -2040 and 0 in d[1:]
    lo, hi = np.zeros((8, 8)), np.full((8, 8), 255)
    cases.append(("dc_alternate_gray", _gray(_tile([[lo, hi, lo, hi, hi, lo, lo], [hi, lo, hi, lo, lo, hi, hi]])),
                  big_dc))
    lo3, hi3 = np.zeros((8, 8, 3), np.uint8), np.full((8, 8, 3), 255, np.uint8)
    cases.append(("dc_alternate_rgb", _tile([[lo3, hi3, lo3, hi3, hi3, lo3], [hi3, lo3, lo3, hi3, lo3, hi3]]),
                  big_dc))

    def eob_only(f):
        return all(not f(q).coefs[:, 1:].any() and not any(any(d[1:]) for d in f(q).dc_diff)
                   for q in JPEG_QUALITIES)
    for v in (0, 255, 128):
        for c in (1, 3):
            cases.append((f"flat{v}_c{c}", np.full((17, 25, c), v, np.uint8), eob_only))

    # 3. coefficient 63 non-zero behind a zero run >= 48: three ZRLs and no EOB
    def zrl3(qualities):
        def prop(f):
            return all(f(q).last_nonzero > 0 and f(q).run_before_63 >= 48 and f(q).zrl >= 3 for q in qualities)
        return prop
    b77 = basis(7, 7)
    soft = 128 + np.rint(16 * b77)
    hard = 128 + np.rint(127 * b77)
    flat = np.full((8, 8), 128)
    cases.append(("b77_amp16_gray", _gray(_tile([[soft, soft, flat, soft]])), zrl3((100,))))
    cases.append(("b77_amp16_rgb", np.repeat(_gray(_tile([[soft, flat], [soft, soft]])), 3, axis=2), zrl3((100,))))
    cases.append(("b77_amp127_gray", _gray(_tile([[hard, flat, hard, hard]])), zrl3((75,))))
    cases.append(("b77_amp127_rgb", np.repeat(_gray(_tile([[hard, hard], [flat, hard]])), 3, axis=2), zrl3((75,))))

    # 4. noise on every edge-replication shape
    n = 0
    for h in NOISE_DIMS:
        for w in NOISE_DIMS:
            cases.append((f"noise_{h}x{w}", _noise(1000 + n, h, w, (1, 3)[n % 2], binary=n % 4 >= 2), _true))
            n += 1
    cases.append(("noise_1x40", _noise(1100, 1, 40, 3), _true))
    cases.append(("noise_40x1", _noise(1101, 40, 1, 1, binary=True), _true))

    # 4 / 5. 64 x 64: many stuffing rounds, many FF 00 pairs
    def many_ff(f):
        q = f(100)
        return q.ff00 > 100 and q.rounds > 1
    cases.append(("noise_64x64_binary_gray", _noise(1200, 64, 64, 1, binary=True), many_ff))
    cases.append(("noise_64x64_binary_rgb", _noise(1201, 64, 64, 3, binary=True), many_ff))
    cases.append(("noise_64x64_uniform_rgb", _noise(1202, 64, 64, 3), lambda f: f(100).rounds > 1))

    # 5. one stuffing round; the last byte: stuffed after padding, and not padded at all
    def one_round_stuffed_end(f):
        q = f(100)
        return q.rounds == 1 and q.ends_stuffed and q.bits % 8 != 0
    for s in STUFFED_END_SEEDS:
        cases.append((f"noise_8x8_stuffed_end_{s}", _noise(s, 8, 8, 1), one_round_stuffed_end))
    cases.append((f"noise_8x8_whole_bytes_{WHOLE_BYTES_SEED}", _noise(WHOLE_BYTES_SEED, 8, 8, 1),
                  lambda f: f(100).rounds == 1 and f(100).bits % 8 == 0))

    # 6. block counts around the scan's 1024 slices (per = ceil(nblocks / 1024))
    def blocks(n, per, multiple):
        def prop(f):
            q = f(100)
            return q.nblocks == n and (n + 1023) // 1024 == per and (n % per == 0) == multiple
        return prop
    cases.append(("blocks_1023", _low_noise(1300, 248, 264, 1), blocks(1023, 1, True)))
    cases.append(("blocks_1024", _low_noise(1301, 256, 256, 1), blocks(1024, 1, True)))
    cases.append(("blocks_1025", _low_noise(1302, 200, 328, 1), blocks(1025, 2, False)))
    cases.append(("blocks_3075_rgb", _low_noise(1303, 200, 328, 3), blocks(3075, 4, False)))
    return cases


def _some(pred):
    return lambda facts: any(pred(f) for f in facts.values())


# over {label: facts at quality 100}
JPEG_SET_PROPERTIES = [
    ("AC category 10, both signs, in luma", _some(lambda f: f.ac_max[0] >= 512 and f.ac_min[0] <= -512)),
    ("AC category 10, both signs, in chroma", _some(lambda f: f.ncomp == 3 and f.ac_max[2] >= 512
                                                     and f.ac_min[2] <= -512)),
    ("DC difference +2040 and -2040", _some(lambda f: max(f.dc_diff[0]) == 2040 and min(f.dc_diff[0]) == -2040)),
    ("three ZRLs in one block, no EOB", _some(lambda f: f.last_nonzero > 0 and f.run_before_63 >= 48)),
    ("a 16-bit code that begins on the last bit of a word", _some(lambda f: 31 in f.code16_at)),
    ("a scan of whole bytes", _some(lambda f: f.bits % 8 == 0)),
    ("a padded scan", _some(lambda f: f.bits % 8 != 0)),
    ("two files end FF 00 FF D9", lambda facts: sum(f.ends_stuffed for f in facts.values()) >= 2),
    ("one stuffing round and several", lambda facts: {1} < {f.rounds for f in facts.values()}),
    ("more than 100 stuffed bytes", _some(lambda f: f.ff00 > 100)),
    ("nblocks 1023, 1024, 1025 and one above 2048 that is no multiple of per",
     lambda facts: {1023, 1024, 1025} <= {f.nblocks for f in facts.values()}
     and any(f.nblocks > 2048 and f.nblocks % ((f.nblocks + 1023) // 1024) for f in facts.values())),
]


# ------------------------------------------------------------------ PNG cases

# match lengths asked for on purpose: the edges of the length symbols' ranges and of 258
RUN_LENGTHS = (2, 3, 4, 10, 11, 12, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258, 259, 260, 261, 516, 517)
# ... and the first and last length of every symbol 257..285, so that each is emitted
_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258)
SYMBOL_LENGTHS = tuple(sorted((set(_LEN_BASE) | {b - 1 for b in _LEN_BASE[1:]}) - set(RUN_LENGTHS)))

# (seed, height, width) of gray noise whose IDAT has the named number of CRC'd bytes (searched)
CRC_CASES = {
    "crc_lt1024": (0, 8, 110),  # 953
    "crc_1024": (3, 8, 119),
    "crc_1025": (0, 8, 119),
    "crc_multiple": (8, 32, 125),  # 4265 = 853 * 5
    "crc_multiple_plus1": (3, 32, 125),  # 4266
}


def crc_class(cn):
    """Which edges of the sliced CRC a count of CRC'd bytes meets."""
    per = (cn + 1023) // 1024
    out = set()
    if cn < 1024:
        out.add("lt1024")
    if cn == 1024:
        out.add("1024")
    if cn == 1025:
        out.add("1025")
    if cn > 4096 and cn % per == 0:
        out.add("multiple")
    if cn > 4097 and (cn - 1) % per == 0 and (cn - 1 + 1023) // 1024 == per:
        out.add("multiple_plus1")
    return out


def _png_noise(seed, h, w, c, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, c)).astype(np.uint8)


def _filter_class(kind, seed, h, w, c):
    rng = np.random.default_rng(seed)
    y, x = np.arange(h)[:, None, None], np.arange(w)[None, :, None]
    if kind == "noise":
        v = rng.integers(0, 256, (h, w, c))
    elif kind == "hramp":  # a horizontal ramp, every row at its own offset: Sub
        v = 3 * x + rng.integers(0, 256, (h, 1, c)) + np.zeros((1, 1, c), int)
    elif kind == "vramp":  # a vertical ramp over a random first row: Up
        v = rng.integers(0, 256, (1, w, c)) + 5 * y
    elif kind == "paeth":  # left half: a function of y alone (Sub is exact); right half: of x alone (Up is
        # exact); only Paeth follows both.  +-1 noise on top
        v = np.where(x < w // 2, rng.integers(0, 256, (h, 1, c)), rng.integers(0, 256, (1, w, c)))
        v = v + rng.integers(-1, 2, (h, w, c))
    elif kind == "avg":
        v = rng.integers(0, 3, (h, w, c))
    else:
        v = np.zeros((h, w, c), int)
    return (v & 0xFF).astype(np.uint8)


def _picks(ftype, rows_after_first=True):
    def prop(ref):
        f = ref.filters[1:] if rows_after_first else ref.filters
        return ftype in f
    return prop


def _run_image(r):
    """Two equal gray rows: a marker, then r zero pixels.  Row 0 keeps filter None (literal marker, a literal
    zero, a match of r - 1); row 1 takes Up: its filter byte 2, a literal zero, then a match of r."""
    row = np.zeros(r + 1, np.uint8)
    row[0] = 1
    return np.stack([row, row])[:, :, None]


def _has_length(r):
    want = [258] * (r // 258) + ([r % 258] if r % 258 >= 3 else [])

    def prop(ref):
        n = len(ref.stream)
        row1 = [k for pos, k in ref.matches if pos >= n // 2]
        # the 1 KiB edge may cut a match of row 1 in two; where it does not, the lengths are exactly these
        return ref.filters.tolist() == [0, 2] and (row1 == want or (n > 1024 and sum(row1) >= sum(want) - 2))
    return prop


def _marker_image(p):
    """Gray, 41 stream bytes per row, zero but for one pixel: the filtered stream is zero except a 1 at p - 2,
    so a run of bytes equal to the byte before starts at stream position p."""
    a = np.zeros((30, 40, 1), np.uint8)
    y, x = divmod(p - 2, 41)
    assert x >= 1
    a[y, x - 1] = 1
    return a


def _run_starts_at(p):
    def prop(ref):
        s = ref.stream
        return (not ref.filters.any() and s[p] == s[p - 1] and s[p - 1] != s[p - 2]
                and not s[p:1100].any() and len(s) > 1100)
    return prop


def png_cases():
    cases = []
    # 1. filter classes, every channel count
    target = {"noise": None, "hramp": 1, "vramp": 2, "paeth": 4, "avg": 3, "flat": 0}
    for kind, ft in target.items():
        for c in (1, 2, 3, 4):
            prop = _true if ft is None else _picks(ft)
            cases.append((f"filt_{kind}_c{c}", _filter_class(kind, 2000 + c, 37, 40, c), prop))
    # rows narrower than, equal to and just wider than a wave's 64 lanes
    for w, c in ((1, 1), (1, 3), (3, 1), (21, 3), (63, 1), (16, 4), (32, 2), (65, 1), (43, 3)):
        for kind in ("noise", "paeth", "avg"):
            cases.append((f"narrow_{kind}_{w}x{c}", _filter_class(kind, 2100 + w, 9, w, c), _true))
    cases.append(("one_row", _filter_class("noise", 2200, 1, 50, 3), _true))
    cases.append(("one_row_ramp", _filter_class("hramp", 2201, 1, 50, 4), lambda r: r.filters[0] == 1))
    cases.append(("one_column", _filter_class("noise", 2202, 50, 1, 2), _true))

    # 2. match lengths
    for r in RUN_LENGTHS + SYMBOL_LENGTHS:
        cases.append((f"run_{r}", _run_image(r), _has_length(r)))
    # a match at stream byte 1: the filter byte 0 of a flat zero image is followed by zeros
    cases.append(("flat_zero", np.zeros((5, 7, 1), np.uint8),
                  lambda ref: ref.matches[0] == (1, 39) and not ref.stream.any()))

    # 3. piece edges: the filtered stream's length around 1 KiB and 2 KiB
    def stream_len(n):
        return lambda ref: len(ref.stream) == n
    for n, (h, w, c) in ((1023, (33, 10, 3)), (1024, (32, 31, 1)), (1024, (4, 85, 3)), (1025, (25, 10, 4)),
                         (1025, (25, 20, 2)), (2048, (8, 85, 3)), (2049, (3, 341, 2))):  # 2049 = 3 x 683: no narrower shape
        assert h * (w * c + 1) == n
        cases.append((f"piece_{n}_noise_{h}x{w}x{c}", _png_noise(2300 + h, h, w, c), stream_len(n)))
        cases.append((f"piece_{n}_flat_{h}x{w}x{c}", np.full((h, w, c), 200, np.uint8), stream_len(n)))
    for p in (1021, 1022, 1023, 1024):
        cases.append((f"run_from_{p}", _marker_image(p), _run_starts_at(p)))

    # 4. CRC slices
    for name, (seed, h, w) in CRC_CASES.items():
        cls = name[4:]
        cases.append((name, _png_noise(seed, h, w, 1), lambda ref, cls=cls: cls in crc_class(ref.cn)))

    # 5. expansion (every literal >= 144 costs 9 bits) and large Adler-32 sums
    def grows(ref):
        return len(ref.file) > len(ref.stream) and not ref.matches
    cases.append(("expand_rgb", _png_noise(2500, 64, 64, 3, 144, 256), grows))
    cases.append(("expand_gray_odd", _png_noise(2501, 33, 31, 1, 144, 256), grows))
    cases.append(("adler_rgba_300", _png_noise(2502, 300, 300, 4), lambda ref: len(ref.stream) == 300 * 1201))
    return cases


def _all_filters(refs):
    later = set().union(*[set(r.filters[1:].tolist()) for r in refs.values()])
    first = {int(r.filters[0]) for r in refs.values()}
    return later == {0, 1, 2, 3, 4} and {0, 1} <= first


PNG_SET_PROPERTIES = [
    ("all five filters after row 0; None and Sub on row 0", _all_filters),
    ("every length symbol 257..285", lambda refs: set().union(*[set(r.len_syms) for r in refs.values()])
     == set(range(257, 286))),
    ("every length edge", lambda refs: {3, 4, 10, 11, 12, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258}
     <= {k for r in refs.values() for _, k in r.matches}),
    ("stream lengths 1023, 1024, 1025, 2048, 2049", lambda refs: {1023, 1024, 1025, 2048, 2049}
     <= {len(r.stream) for r in refs.values()}),
    ("a match cut at a piece edge and one that begins on it",
     lambda refs: any((pos + k) % 1024 == 0 and r.stream[pos + k] == r.stream[pos + k - 1]
                      for r in refs.values() for pos, k in r.matches if pos + k < len(r.stream))
     and any(pos % 1024 == 0 for r in refs.values() for pos, k in r.matches)),
    ("every CRC slice class", lambda refs: {"lt1024", "1024", "1025", "multiple", "multiple_plus1"}
     <= set().union(*[crc_class(r.cn) for r in refs.values()])),
    ("a file longer than its pixels", lambda refs: any(len(r.file) > r.stream.size for r in refs.values())),
]


# ------------------------------------------------------------------ the references, computed once per process

_jpeg_refs, _png_refs = {}, {}


def jpeg_ref(label, arr, quality):
    """JpegFacts of oracle.jpeg_encode(arr, quality), kept per (label, quality)."""
    key = (label, quality)
    if key not in _jpeg_refs:
        from oracle import oracle as O
        data = O.jpeg_encode(arr, quality)
        h, w, c = arr.shape
        nb = ((h + 7) // 8) * ((w + 7) // 8) * (1 if c == 1 else 3)
        st, co = O.jpeg_coefs(data, nb + 8)
        assert st == 0 and len(co) == nb, (label, st, len(co), nb)
        _jpeg_refs[key] = jpeg_facts(data, co)
    return _jpeg_refs[key]


def png_ref(label, arr):
    """ref_penc.encode(arr), kept per label."""
    if label not in _png_refs:
        import ref_penc
        _png_refs[label] = ref_penc.encode(arr)
    return _png_refs[label]


def png_input(arr):
    """A PNG file of the array for the library to decode: unfiltered rows, zlib level 1."""
    from datago_amd.synth import encode_png
    h, w, c = arr.shape
    return encode_png(np.ascontiguousarray(arr).reshape(h, w * c), w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c], c,
                      np.random.default_rng(0), level=1, filters="none")


def png_independent_checks(data, arr):
    """Readers that share nothing with the encoder under test: chunk layout and CRCs, zlib (with its Adler-32),
    PIL and the oracle's decoder must all give back `arr`.  Returns the inflated (filtered) stream."""
    import binascii
    import io
    import zlib

    from PIL import Image

    from oracle import oracle as O
    h, w, c = arr.shape
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, types = 8, b"", []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        t, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert binascii.crc32(t + body) & 0xFFFFFFFF == crc, t
        types.append(t)
        if t == b"IDAT":
            idat += body
        pos += 12 + n
    assert types == [b"IHDR", b"IDAT", b"IEND"] and pos == len(data)
    filt = zlib.decompress(idat)
    assert len(filt) == h * (w * c + 1)
    st, dec = O.png_decode(data)
    assert st == 0 and dec.shape == arr.shape and np.array_equal(dec, arr)
    im = Image.open(io.BytesIO(data))
    assert im.size == (w, h) and im.mode == {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[c]
    assert np.array_equal(np.asarray(im).reshape(arr.shape), arr)
    return filt
