"""The crafted BMP files that the tests of context option "bmp" share
(test_bmp_cpu.py, test_gpu_bmp.py): pixel cases for every uncompressed form,
RLE cases that reach every edge of the step logic, and the refusals with the
status and text each must give.

pixel_cases() and rle_cases() give (label, bytes, pillow, reason): pillow False
marks a file Pillow decodes wrongly (reason says which of its two quirks), which
is compared against ref_bmp alone.  refusals() gives (label, bytes, status,
text)."""
import numpy as np

import bmp_craft as G
import ref_bmp as R

WIDTHS = [1, 2, 3, 5, 7, 8, 9, 31, 33]
RLE_WIDTHS = [1, 2, 9, 64, 65, 131]
QUIRK_PARITY = "Pillow pads an absolute run by the parity of the file position; bfOffBits is odd here"
QUIRK_ODD4 = "Pillow reads n // 2 bytes for an RLE4 absolute run of odd n"


def noise(h, w, ncol, seed):
    return np.random.default_rng(seed).integers(0, ncol, (h, w)).astype(np.uint8)


def photo(h, w, ncol, seed):
    """Smooth ramps plus a little noise: short runs and literal stretches mixed."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = (x * 3 + y * 5) // 7 + rng.integers(0, 2, (h, w)) * rng.integers(0, 2, (h, w))
    return (v % ncol).astype(np.uint8)


def rgb(h, w, seed, c=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c)).astype(np.uint8)


def _form(form, w, h, seed, top_down=False, **kw):
    """One uncompressed file of a named form."""
    if form in ("1", "4", "8"):
        bits = int(form)
        n = kw.pop("npal", 1 << bits)
        return G.bmp(w, h, bits, noise(h, w, n, seed), pal=G.palette(n, seed + 1), top_down=top_down, **kw)
    if form == "24":
        return G.bmp(w, h, 24, rgb(h, w, seed), top_down=top_down, **kw)
    if form == "32":
        return G.bmp(w, h, 32, rgb(h, w, seed, 4), top_down=top_down, **kw)
    if form == "bf24":
        return G.bmp(w, h, 24, rgb(h, w, seed), compression=G.BITFIELDS, masks=(0xFF0000, 0xFF00, 0xFF),
                     top_down=top_down, **kw)
    kind, k = form.split(":")  # "bf32:k" under a V4 header, "bf32h40:k" under a 40-byte one (three masks, no alpha)
    kw.setdefault("header", 40 if kind == "bf32h40" else 108)
    m = G.MASKS32[int(k)]
    return G.bmp(w, h, 32, rgb(h, w, seed, 4), compression=G.BITFIELDS, masks=m[:3] if kw["header"] == 40 else m,
                 top_down=top_down, **kw)


def pixel_cases():
    out = []

    def add(label, data, pillow=True, reason=""):
        out.append((label, data, pillow, reason))
    seed = 100
    for form in ["1", "4", "8", "24", "32"]:
        for w in WIDTHS:
            for td in (False, True):
                seed += 1
                add("%s-bit %dx3 %s" % (form, w, "top-down" if td else "bottom-up"), _form(form, w, 3, seed, td))
    forms = ["bf24"] + ["bf32:%d" % k for k in range(7)] + ["bf32h40:%d" % k for k in range(3)]
    for fi, form in enumerate(forms):
        for wi, w in enumerate(WIDTHS):
            seed += 1
            td = (fi + wi) % 2 == 1
            add("%s %dx3 %s" % (form, w, "top-down" if td else "bottom-up"), _form(form, w, 3, seed, td))
    for form in ["1", "4", "8", "24", "32", "bf32:5", "bf32:3"]:
        seed += 1
        add("%s 131x67" % form, _form(form, 131, 67, seed))
        add("%s 300x200 top-down" % form, _form(form, 300, 200, seed + 50, True))
    for form in ["1", "4", "8", "24"]:
        seed += 1
        add("core header %s-bit 33x5" % form, _form(form, 33, 5, seed, header=12))
    for form in ["8", "24", "bf32:5", "bf32:0"]:
        seed += 1
        add("V5 header %s 31x4" % form, _form(form, 31, 4, seed, header=124))
    add("V4 header 4-bit 9x4", _form("4", 9, 4, 180, header=108))
    for form, gap in [("24", 10), ("8", 6), ("1", 2), ("24", 1), ("8", 3), ("4", 1), ("32", 1), ("bf32:4", 3)]:
        seed += 1
        add("%s 9x5 gap %d before the pixels" % (form, gap), _form(form, 9, 5, seed, gap=gap))
    # colour tables shorter than the depth allows, indices below their length
    add("8-bit 16 entries", _form("8", 33, 7, 190, npal=16))
    add("8-bit 2 entries", _form("8", 33, 7, 191, npal=2))
    add("8-bit 100 entries", _form("8", 33, 7, 192, npal=100))
    add("4-bit 2 entries", _form("4", 33, 7, 193, npal=2))
    add("4-bit 11 entries top-down", _form("4", 31, 6, 194, True, npal=11))
    add("1-bit 1 entry", _form("1", 33, 7, 195, npal=1))
    # ... and a table longer than the largest index in use
    add("8-bit 256 entries, indices below 5", G.bmp(9, 4, 8, noise(4, 9, 5, 196), pal=G.palette(256, 197)))
    # a colour table on a 24-bit file is skipped (bfOffBits)
    add("24-bit with a colour table", G.bmp(9, 4, 24, rgb(4, 9, 198), pal=G.palette(7, 199)))
    add("trailing bytes", _form("24", 9, 4, 200, tail=b"trailing bytes"))
    return out


def _rle(w, h, idx, rle4, cmds=None, ncol=None, **kw):
    ncol = ncol or (16 if rle4 else 256)
    data = G.rle_bytes(cmds, rle4)
    return G.bmp(w, h, 4 if rle4 else 8, data=data, compression=G.RLE4 if rle4 else G.RLE8,
                 pal=G.palette(ncol, w * 7 + h), **kw)


def rle_cases():
    out = []

    def add(label, data, pillow=True, reason=""):
        out.append((label, data, pillow, reason))
    seed = 300
    for rle4 in (False, True):
        name = "RLE4" if rle4 else "RLE8"
        ncol = 16 if rle4 else 256
        for w in RLE_WIDTHS:
            seed += 1
            ph, nz = photo(3, w, ncol, seed), noise(3, w, ncol, seed)
            add("%s %dx3 runs" % (name, w), _rle(w, 3, ph, rle4, G.rle_commands(ph, rle4, "runs")))
            add("%s %dx3 runs of 1" % (name, w), _rle(w, 3, nz, rle4, G.rle_commands(nz, rle4, "runs", run_len=1)))
            add("%s %dx3 absolute even" % (name, w),
                _rle(w, 3, nz, rle4, G.rle_commands(nz, rle4, "abs", abs_len=8, odd_abs=False)))
            add("%s %dx3 absolute 254" % (name, w),
                _rle(w, 3, nz, rle4, G.rle_commands(nz, rle4, "abs", abs_len=254, odd_abs=False)))
            add("%s %dx3 mixed" % (name, w), _rle(w, 3, ph, rle4, G.rle_commands(ph, rle4, "mixed", odd_abs=not rle4)))
            if not rle4:
                add("RLE8 %dx3 absolute odd" % w, _rle(w, 3, nz, rle4, G.rle_commands(nz, rle4, "abs", abs_len=7)))
                add("RLE8 %dx3 absolute 255" % w, _rle(w, 3, nz, rle4, G.rle_commands(nz, rle4, "abs", abs_len=255)))
        for w in (9, 131):  # odd absolute runs of RLE4: the format's ceil(n / 2) bytes
            nz = noise(3, w, 16, seed + w) if rle4 else None
            if rle4:
                add("RLE4 %dx3 absolute odd" % w, _rle(w, 3, nz, True, G.rle_commands(nz, True, "abs", abs_len=7)),
                    False, QUIRK_ODD4)
        # a 255-pixel run and a 255-pixel (RLE4: 254-pixel) absolute block in one row
        nz = noise(2, 510, ncol, seed + 1)
        na = 254 if rle4 else 255
        cm = []
        for r in (1, 0):
            cm.append(("run", 255, 0x3C))
            cm.append(("abs", [int(v) for v in nz[r, 255:255 + na]]))
            cm += [("run", 1, int(v) * (17 if rle4 else 1)) for v in nz[r, 255 + na:]]
            cm.append(("eol",))
        add("%s 510x2 run 255 and absolute %d" % (name, na), _rle(510, 2, nz, rle4, cm + [("eob",)]))
        # an absolute block whose data bytes look like commands
        if rle4:
            row = [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 2, 3, 3, 0, 0]
        else:
            row = [0, 0, 0, 1, 0, 2, 5, 5, 0, 0, 0, 1, 0, 2, 1, 1]
        ix = np.array([row, row[::-1], row], np.uint8)
        cm = []
        for r in (2, 1, 0):
            cm += [("abs", list(ix[r])), ("eol",)]
        add("%s absolute data that looks like commands" % name, _rle(16, 3, ix, rle4, cm + [("eob",)]))
        # how the stream ends
        ph = photo(4, 65, ncol, seed + 2)
        kw = dict(odd_abs=not rle4)
        add("%s end-of-bitmap straight after the last pixel" % name,
            _rle(65, 4, ph, rle4, G.rle_commands(ph, rle4, "mixed", last_eol=False, **kw)))
        add("%s no end-of-bitmap" % name, _rle(65, 4, ph, rle4, G.rle_commands(ph, rle4, "mixed", eob=False, **kw)))
        add("%s data ends with the last pixel" % name,
            _rle(65, 4, ph, rle4, G.rle_commands(ph, rle4, "mixed", last_eol=False, eob=False, **kw)))
        add("%s trailing bytes after end-of-bitmap" % name,
            _rle(65, 4, ph, rle4, G.rle_commands(ph, rle4, "mixed", **kw) + [("raw", b"\x07\x09\x00\x02\x01\x01\x00")]))
        add("%s gap before the stream" % name, _rle(65, 4, ph, rle4, G.rle_commands(ph, rle4, "mixed", **kw), gap=6))
        add("%s odd bfOffBits, runs only" % name, _rle(65, 4, ph, rle4, G.rle_commands(ph, rle4, "runs"), gap=1))
        add("%s short colour table" % name,
            _rle(33, 4, ph[:, :33] % 5, rle4, G.rle_commands(ph[:, :33] % 5, rle4, "mixed", **kw), ncol=5))
        big = photo(200, 300, ncol, seed + 3)
        add("%s 300x200 photo" % name, _rle(300, 200, big, rle4, G.rle_commands(big, rle4, "mixed", **kw)))
        add("%s 131x67 noise" % name, _rle(131, 67, noise(67, 131, ncol, seed + 4), rle4,
                                          G.rle_commands(noise(67, 131, ncol, seed + 4), rle4, "mixed", **kw)))
    nz = noise(3, 33, 256, 390)
    add("RLE8 odd bfOffBits, absolute odd", _rle(33, 3, nz, False, G.rle_commands(nz, False, "abs", abs_len=7), gap=1),
        False, QUIRK_PARITY)
    return out


def refusals():
    out = []
    U, Cc = R.UNSUPPORTED, R.CORRUPT
    px16 = np.random.default_rng(401).integers(0, 65536, (3, 5))
    out.append(("16-bit 555", G.bmp(5, 3, 16, px16), U, "BMP: 16 bits per pixel"))
    out.append(("16-bit 565 masks", G.bmp(5, 3, 16, px16, compression=G.BITFIELDS, masks=(0xF800, 0x7E0, 0x1F), pos=()),
                U, "BMP: 16 bits per pixel"))
    out.append(("32-bit BI_RGB under V4", G.bmp(5, 3, 32, rgb(3, 5, 402, 4), header=108), U,
                "BMP: 32-bit BI_RGB under a V4 / V5 header"))
    out.append(("32-bit BI_RGB under V5", G.bmp(5, 3, 32, rgb(3, 5, 402, 4), header=124), U,
                "BMP: 32-bit BI_RGB under a V4 / V5 header"))
    raw32 = G.pack_rows(rgb(3, 5, 403, 4), 32)
    out.append(("10-10-10 masks", G.bmp(5, 3, 32, data=raw32, compression=G.BITFIELDS, header=108,
                                        masks=(0x3FF00000, 0xFFC00, 0x3FF, 0)), U,
                "BMP: bit masks outside the supported sets"))
    out.append(("all-zero masks", G.bmp(5, 3, 32, data=raw32, compression=G.BITFIELDS, header=108, masks=(0, 0, 0, 0)),
                U, "BMP: bit masks outside the supported sets"))
    out.append(("24-bit masks in RGB order", G.bmp(5, 3, 24, rgb(3, 5, 404), compression=G.BITFIELDS,
                                                  masks=(0xFF, 0xFF00, 0xFF0000)), U,
                "BMP: bit masks outside the supported sets"))
    out.append(("2 bits per pixel", G.bmp(5, 3, 2, noise(3, 5, 4, 405), pal=G.palette(4, 1)), U, "BMP: 2 bits per pixel"))
    for hs in (52, 56, 64):
        out.append(("header size %d" % hs, G.bmp(5, 3, 24, rgb(3, 5, 406), header=hs), U,
                    "BMP: OS/2 2.x, V2 or V3 info header"))
    for comp, nm in [(4, "BI_JPEG"), (5, "BI_PNG"), (6, "BI_ALPHABITFIELDS"), (11, "compression 11")]:
        out.append((nm, G.bmp(5, 3, 24, rgb(3, 5, 407), compression=comp), U, "BMP: unsupported compression"))
    ph = photo(3, 9, 16, 408)
    out.append(("top-down RLE8", G.bmp(9, 3, 8, data=G.rle_bytes(G.rle_commands(ph, False)), compression=G.RLE8,
                                       pal=G.palette(256, 2), top_down=True), U, "BMP: top-down RLE"))
    out.append(("RLE8 on 4 bits", G.bmp(9, 3, 4, data=G.rle_bytes(G.rle_commands(ph, False)), compression=G.RLE8,
                                        pal=G.palette(16, 2)), U, "BMP: RLE or bit-field compression on a mismatched depth"))
    out.append(("RLE4 on 8 bits", G.bmp(9, 3, 8, data=G.rle_bytes(G.rle_commands(ph, True), True), compression=G.RLE4,
                                        pal=G.palette(256, 2)), U, "BMP: RLE or bit-field compression on a mismatched depth"))
    out.append(("planes 2", G.bmp(5, 3, 24, rgb(3, 5, 409), planes=2), U, "BMP: planes not 1"))
    out.append(("biClrUsed 300 on 8 bits", G.bmp(5, 3, 8, noise(3, 5, 256, 410), pal=G.palette(300, 3)), U,
                "BMP: colour table larger than the depth allows"))
    out.append(("biClrUsed 3 on 1 bit", G.bmp(5, 3, 1, noise(3, 5, 2, 411), pal=G.palette(3, 3)), U,
                "BMP: colour table larger than the depth allows"))
    out.append(("negative width", G.bmp(-5, 3, 24, data=b"\0" * 48), U, "BMP: negative width"))
    out.append(("3 bits per pixel", G.bmp(5, 3, 3, data=b"\0" * 12, pal=G.palette(8, 4)), U, "BMP: unsupported bits per pixel"))
    out.append(("32 bits under a core header", G.bmp(5, 3, 32, data=b"\0" * 60, header=12), U,
                "BMP: unsupported bits per pixel"))
    out.append(("zero width", G.bmp(0, 3, 24, data=b""), U, "BMP: zero dimension"))
    out.append(("zero height", G.bmp(5, 0, 24, data=b""), U, "BMP: zero dimension"))
    out.append(("over 512 MiB", G.bmp(20000, 10000, 24, data=b"\0" * 64), U, "BMP: image over image's allocation limit"))
    # ---- stream irregularities: found while decoding
    for rle4 in (False, True):
        nm = "RLE4" if rle4 else "RLE8"
        v = 0x12

        def f(cmds, w=8, h=3, ncol=None, _r=rle4):
            return G.bmp(w, h, 4 if _r else 8, data=G.rle_bytes(cmds, _r), compression=G.RLE4 if _r else G.RLE8,
                         pal=G.palette(ncol or (16 if _r else 256), 6))
        full = [("run", 8, v), ("eol",)]
        out.append((nm + " run passes the row's end", f([("run", 5, v), ("run", 4, v), ("eol",)] + full * 2 + [("eob",)]),
                    U, R.WHY_ROW))
        out.append((nm + " absolute block passes the row's end",
                    f(full + [("run", 4, v), ("abs", [1, 2, 3, 4, 5, 6])] + full + [("eob",)]), U, R.WHY_ROW))
        out.append((nm + " row not closed", f([("run", 8, v), ("run", 8, v), ("eol",)] + full + [("eob",)]), U, R.WHY_ROW))
        out.append((nm + " delta", f(full + [("run", 2, v), ("delta", 3, 0), ("run", 3, v), ("eol",)] + full + [("eob",)]),
                    U, R.WHY_DELTA))
        out.append((nm + " early end-of-line", f(full + [("run", 5, v), ("eol",), ("run", 8, v), ("eol",), ("eob",)]),
                    U, R.WHY_DELTA))
        out.append((nm + " two ends-of-line", f(full + [("eol",)] + full + [("eob",)]), U, R.WHY_DELTA))
        out.append((nm + " end-of-line first", f([("eol",)] + full * 3 + [("eob",)]), U, R.WHY_DELTA))
        out.append((nm + " early end-of-bitmap", f(full * 2 + [("run", 3, v), ("eob",)]), U, R.WHY_DELTA))
        out.append((nm + " data ends early", f(full * 2 + [("run", 3, v)]), U, R.WHY_SHORT))
        cut = G.rle_bytes(full * 2 + [("abs", [1, 2, 3, 4, 5, 6, 7, 8])], rle4)[:-2]
        out.append((nm + " data ends inside an absolute block",
                    G.bmp(8, 3, 4 if rle4 else 8, data=cut, compression=G.RLE4 if rle4 else G.RLE8,
                          pal=G.palette(16 if rle4 else 256, 6)), U, R.WHY_SHORT))
        big = photo(40, 131, 16, 420)
        cm = G.rle_commands(big, rle4, "mixed", odd_abs=not rle4)
        k = len(cm) * 2 // 3
        while cm[k][0] != "run":
            k += 1
        far = cm[:k] + [("run", 200, cm[k][2])] + cm[k + 1:]
        out.append((nm + " run passes the row's end far into the stream", f(far, 131, 40), U, R.WHY_ROW))
        out.append((nm + " index past the colour table",
                    f([("run", 8, 0x11), ("eol",), ("abs", [1, 1, 1, 5, 1, 1, 1, 1]), ("eol",)] + [("run", 8, 0x11)], ncol=5),
                    U, R.WHY_PALETTE))
    for bits in (1, 4, 8):
        ix = np.zeros((3, 9), np.uint8)
        ix[1, 8] = 1 if bits == 1 else 7
        out.append(("%d-bit index past the colour table" % bits,
                    G.bmp(9, 3, bits, ix, pal=G.palette(1 if bits == 1 else 7, 7)), U, R.WHY_PALETTE))
    # ---- structurally broken
    good24 = G.bmp(9, 3, 24, rgb(3, 9, 430))
    good8 = G.bmp(9, 3, 8, noise(3, 9, 256, 431), pal=G.palette(256, 8))
    bf40 = G.bmp(9, 3, 32, rgb(3, 9, 432, 4), compression=G.BITFIELDS, masks=G.MASKS32[0][:3])
    out.append(("ends inside the file header", good24[:10], Cc, "BMP: truncated file header"))
    out.append(("ends inside the info header", good24[:30], Cc, "BMP: truncated info header"))
    out.append(("ends inside the masks", bf40[:14 + 40 + 7], Cc, "BMP: truncated bit masks"))
    out.append(("ends inside the colour table", good8[:14 + 40 + 500], Cc, "BMP: truncated colour table"))
    out.append(("bfOffBits inside the headers", G.bmp(9, 3, 24, rgb(3, 9, 430), off_bits=30), Cc,
                "BMP: pixel data offset inside the headers or past the file"))
    out.append(("bfOffBits inside the colour table", G.bmp(9, 3, 8, noise(3, 9, 256, 431), pal=G.palette(256, 8), off_bits=54),
                Cc, "BMP: pixel data offset inside the headers or past the file"))
    out.append(("bfOffBits past the file", G.bmp(9, 3, 24, rgb(3, 9, 430), off_bits=4000), Cc,
                "BMP: pixel data offset inside the headers or past the file"))
    out.append(("pixel array cut short", good24[:-1], Cc, "BMP: pixel data truncated"))
    out.append(("8-bit pixel array cut short", good8[:-13], Cc, "BMP: pixel data truncated"))
    out.append(("info header size 48", G.bmp(9, 3, 24, rgb(3, 9, 430), header=48), Cc, "BMP: unknown info header size"))
    return out
