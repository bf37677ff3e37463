"""A small TIFF writer and the files the TIFF tests share: either byte order, strips or tiles, any segment phase,
an LZW and a PackBits encoder.  Pillow writes one strip for small images and cannot be asked for tiles, odd
offsets or a table that fills without a clear; every file made here is still read back by Pillow in the tests."""
import struct

import numpy as np


def lzw(data, clear=True, end=True):
    """TIFF LZW: MSB-first codes, clear 256, end 257, the width grows one code early.  clear=False never clears
    (the table fills and stays full); end=False leaves the end code out."""
    out, acc, nacc = bytearray(), 0, 0
    tab, dn, first, s = {}, 258, True, None  # dn: the decoder's entries when it reads the next code

    def put(c):
        nonlocal acc, nacc, dn, first
        w = min(12, (dn + 1).bit_length())
        acc, nacc = (acc << w) | c, nacc + w
        while nacc >= 8:
            out.append((acc >> (nacc - 8)) & 255)
            nacc -= 8
        dn, first = (258, True) if c == 256 else (dn, False) if first else (min(dn + 1, 4096), False)

    put(256)
    for b in bytes(data):
        if s is None or (s, b) in tab:
            s = b if s is None else tab[(s, b)]
            continue
        put(s)
        if len(tab) < 4096 - 258:
            tab[(s, b)] = 258 + len(tab)
        s = b
        if clear and len(tab) >= 4094 - 258:
            put(256)
            tab = {}
    for c in ([] if s is None else [s]) + ([257] if end else []):
        put(c)
    return bytes(out) + (bytes([(acc << (8 - nacc)) & 255]) if nacc else b"")


def packbits(data):
    """Greedy PackBits: repeats of 3 or more, literals of up to 128."""
    d, out, i, lit = bytes(data), bytearray(), 0, bytearray()
    while i <= len(d):
        j = i
        while j < len(d) and j - i < 128 and d[j] == d[i]:
            j += 1
        if j - i >= 3 or i == len(d):  # a repeat (or the end) closes the literals gathered so far
            for k in range(0, len(lit), 128):
                out += bytes([len(lit[k:k + 128]) - 1]) + lit[k:k + 128]
            lit = bytearray()
        if j - i >= 3:
            out += bytes([257 - (j - i), d[i]])
        else:
            lit += d[i:j]
        i = max(j, i + 1)
    return bytes(out)


def tiff(arr, comp=1, pred=1, rps=None, tile=None, be=False, photo=None, phase=0, pack=None, rowwise=False, tags=()):
    """arr: H x W or H x W x C uint8.  tile=(tw, th) or strips of rps rows.  pack: segment bytes -> coded bytes
    (default by comp); rowwise packs every row on its own.  tags: (tag, type, values or None) replaced or dropped."""
    a = np.asarray(arr, np.uint8)
    a = a[:, :, None] if a.ndim == 2 else a
    H, W, C = a.shape
    e = ">" if be else "<"
    pack = pack or {1: bytes, 5: lzw, 32773: packbits}[comp]
    if tile:
        tw, th = tile
        p = np.zeros((-(-H // th) * th, -(-W // tw) * tw, C), np.uint8)
        p[:H, :W] = a
        segs = [p[y:y + th, x:x + tw].copy() for y in range(0, p.shape[0], th) for x in range(0, p.shape[1], tw)]
    else:
        rps = rps or H
        segs = [a[y:y + rps].copy() for y in range(0, H, rps)]
    body, offs, lens = bytearray(b"\0" * phase), [], []
    for s in segs:
        if pred == 2:
            s[:, 1:] -= s[:, :-1].copy()
        c = b"".join(pack(r.tobytes()) for r in s) if rowwise else pack(s.tobytes())
        offs, lens, body = offs + [8 + len(body)], lens + [len(c)], body + c
    body += b"\0" * (len(body) & 1)
    ent = {256: (4, [W]), 257: (4, [H]), 258: (3, [8] * C), 259: (3, [comp]), 277: (3, [C]), 284: (3, [1]),
           262: (3, [(1 if C < 3 else 2) if photo is None else photo]), 317: (3, [pred]), 338: (3, [2] if C in (2, 4) else None)}
    ent.update({322: (4, [tile[0]]), 323: (4, [tile[1]]), 324: (4, offs), 325: (4, lens)} if tile else
               {278: (4, [rps]), 273: (4, offs), 279: (4, lens)})
    ent.update({t: (ty, v) for t, ty, v in tags})
    ifd, extra, base = bytearray(), bytearray(), 8 + len(body)
    ent = {t: (ty, list(v)) for t, (ty, v) in sorted(ent.items()) if v is not None}
    for t, (ty, v) in ent.items():
        raw = struct.pack(e + {1: "B", 3: "H", 4: "I"}[ty] * len(v), *v)
        if len(raw) > 4:
            raw, extra = struct.pack(e + "I", base + len(extra)), extra + raw + b"\0" * (len(raw) & 1)
        ifd += struct.pack(e + "HHI", t, ty, len(v)) + raw.ljust(4, b"\0")
    head = (b"MM" if be else b"II") + struct.pack(e + "HI", 42, base + len(extra))
    return head + bytes(body) + bytes(extra) + struct.pack(e + "H", len(ent)) + bytes(ifd) + b"\0\0\0\0"


def noise(h, w, c, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)
    return a[:, :, 0] if c == 1 else a


def cases():
    """(label, file, pixels) of every crafted file that decodes; 97 x 70 unless the label says otherwise."""
    n3, n4, out = noise(70, 97, 3, 1), noise(70, 97, 4, 3), []

    def add(label, arr, **kw):
        out.append((label, tiff(arr, **kw), np.asarray(arr)))
    add("lzw one strip", n3, comp=5)
    # (libtiff refuses a table that stays full for 1024 codes, so the stream that never clears comes in strips of
    # 16 rows: each fills its table and goes on with it full for some 700 codes)
    add("lzw never clears", n3, comp=5, rps=16, pack=lambda d: lzw(d, clear=False))
    add("lzw flat", np.full((70, 97, 3), 7, np.uint8), comp=5)
    big = noise(150, 151, 3, 8)  # one strip of 67,950 bytes: over what k_tiff_lzw keeps in LDS
    big[40:90] = 5
    add("lzw pred big strip 151x150", big, comp=5, pred=2)
    add("lzw no end code", n3, comp=5, rps=7, pack=lambda d: lzw(d, end=False))
    for rps in (1, 7, 70):
        add("lzw pred rps %d" % rps, n3, comp=5, pred=2, rps=rps)
    for ph in range(4):
        add("lzw phase %d" % ph, n3, comp=5, rps=7, phase=ph)
    # a chosen PackBits stream: literals of 1, 127 and 128, repeats of 2, 3 and 128, the no-op header 128 twice, a
    # literal across the first 64-header step; 579 bytes = 193 x 3
    r127, r128, r60 = bytes(range(127)), bytes(range(100, 228)), bytes(range(60))
    stream = b"\x00a\xffb\x7e" + r127 + b"\xfec\x80\x7f" + r128 + b"\x81d\x80\xffe\x3b" + r60 + b"\x81f"
    data = b"abb" + r127 + b"ccc" + r128 + b"d" * 128 + b"ee" + r60 + b"f" * 128
    add("packbits chosen runs 193x3", np.frombuffer(data, np.uint8).reshape(3, 193), comp=32773, pack=lambda d: stream)
    mix = n3.copy()
    mix[10:40, 20:90] = 9
    add("packbits rows apart", mix, comp=32773, rowwise=True, rps=9)
    add("packbits across rows", mix, comp=32773, rps=9)
    for w in (1, 63, 64, 65, 129, 257):
        for c in (1, 2, 3, 4):
            add("pred %dx3x%d" % (w, c), noise(3, w, c, 10 * w + c), comp=5, pred=2)
    for tile in ((16, 16), (32, 48)):
        add("tiles %dx%d raw" % tile, n3, tile=tile)
        add("tiles %dx%d lzw pred" % tile, n3, tile=tile, comp=5, pred=2)
    add("MM lzw pred", n3, be=True, comp=5, pred=2, rps=7)
    add("MM raw gray", n3[:, :, 0], be=True)
    out.append(("WhiteIsZero", tiff(n3[:, :, 0], photo=0, comp=5), 255 - n3[:, :, 0]))
    add("La8 packbits", n4[:, :, :2], comp=32773)
    add("Rgba8 lzw pred tiles", n4, comp=5, pred=2, tile=(32, 32))
    add("Rgba8 without ExtraSamples", n4, comp=5, tags=[(338, 3, None)])
    return out


def refusals():
    """(label, file, corrupt) of every form the library refuses: DG_ERR_CORRUPT if corrupt, else DG_ERR_UNSUPPORTED.
    A label that starts with "stream" is refused by a kernel, the others by the header walk."""
    n3, n4 = noise(8, 20, 3, 5), noise(8, 20, 4, 6)
    g, whole = n3[:, :, 0], tiff(n3)
    out = [("BigTIFF", whole[:2] + b"\x2b" + whole[3:], False)]
    for label, arr, kw in [
            ("16-bit", n3, dict(tags=[(258, 3, [16] * 3)])), ("32-bit", n3, dict(tags=[(258, 3, [32] * 3)])),
            ("1-bit", g, dict(tags=[(258, 3, [1])])), ("2-bit", g, dict(tags=[(258, 3, [2])])), ("4-bit", g, dict(tags=[(258, 3, [4])])),
            ("float", n3, dict(tags=[(339, 3, [3] * 3)])), ("palette", g, dict(photo=3)), ("mask", g, dict(photo=4)),
            ("CMYK", n4, dict(photo=5)), ("YCbCr", n3, dict(photo=6)), ("CIELab", n3, dict(photo=8)),
            ("planar 2", n3, dict(tags=[(284, 3, [2])])), ("FillOrder 2", n3, dict(tags=[(266, 3, [2])])),
            ("predictor 3", n3, dict(comp=5, pred=3)), ("predictor 2 uncompressed", n3, dict(tags=[(317, 3, [2])])),
            ("associated alpha", n4, dict(tags=[(338, 3, [1])])), ("unspecified extra", n4, dict(tags=[(338, 3, [0])])),
            ("gray + extra without the tag", n4[:, :, :2], dict(tags=[(338, 3, None)])), ("tile 24x24", n3, dict(tile=(24, 24))),
            ("old-style LZW", n3, dict(comp=5, pack=lambda d: b"\0\1" + lzw(d))),
            ("stream: LZW table stays full", noise(70, 97, 3, 1), dict(comp=5, pack=lambda d: lzw(d, clear=False)))]:
        out.append((label, tiff(arr, **kw), False))
    out += [("compression %d" % c, tiff(n3, tags=[(259, 3, [c])]), False) for c in (2, 3, 4, 6, 7, 8, 32946, 34712)]
    return out + [
        ("IFD past the file", whole[:-20], True), ("IFD offset past the file", whole[:4] + b"\xff\xff\xff\x7f" + whole[8:], True),
        ("segment offset past the file", tiff(n3, tags=[(273, 4, [1 << 30])]), True),
        ("segment count past the file", tiff(n3, tags=[(279, 4, [1 << 20])]), True),
        ("truncated segment", tiff(n3, tags=[(279, 4, [n3.size - 1])]), True),
        ("segment table too short", tiff(n3, rps=4, tags=[(273, 4, [8]), (279, 4, [240])]), True),
        ("stream: short LZW", tiff(n3, comp=5, pack=lambda d: lzw(d)[:100]), True),
        ("stream: short PackBits", tiff(n3, comp=32773, pack=lambda d: packbits(d)[:100]), True)]
