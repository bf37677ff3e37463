"""A Windows bitmap writer with every knob the tests of context option "bmp"
need: header size, depth, compression, bit masks, top-down rows, colour table
length, slack before the pixels, explicit RLE command lists, truncation (slice
the result)."""
import struct

import numpy as np

RGB, RLE8, RLE4, BITFIELDS = 0, 1, 2, 3

# Pillow's byte-aligned 32-bit mask sets (BmpImagePlugin.py, SUPPORTED[32]) without the all-zero one: R, G, B, A
MASKS32 = [(0xFF0000, 0xFF00, 0xFF, 0x0), (0xFF000000, 0xFF0000, 0xFF00, 0x0), (0xFF000000, 0xFF00, 0xFF, 0x0),
           (0xFF000000, 0xFF0000, 0xFF00, 0xFF), (0xFF, 0xFF00, 0xFF0000, 0xFF000000),
           (0xFF0000, 0xFF00, 0xFF, 0xFF000000), (0xFF000000, 0xFF00, 0xFF, 0xFF0000)]


def palette(n, seed):
    """n RGB entries, no two alike and never a gray ramp (Pillow would report mode L / 1 for one)."""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    pal[:, 0] = (np.arange(n) * 37 + 11) % 256
    pal[0] = (200, 30, 90)
    return pal


def stride(w, bits):
    return ((w * bits + 31) // 32) * 4


def mask_pos(m):
    """Byte of a byte-aligned mask inside the pixel (None for 0)."""
    return None if m == 0 else {0xFF: 0, 0xFF00: 1, 0xFF0000: 2, 0xFF000000: 3}[m]


def pack_rows(pix, bits, top_down=False, pos=(2, 1, 0, 3)):
    """The pixel array of an uncompressed file.  pix: h x w indices (1 / 4 / 8 bits), h x w x 3 RGB (24) or
    h x w x 4 RGBA (32, pos = byte of R, G, B, A inside a pixel; None drops the channel), top row first."""
    pix = np.asarray(pix)
    h, w = pix.shape[:2]
    rows = np.zeros((h, stride(w, bits)), np.uint8)
    if bits == 8:
        rows[:, :w] = pix
    elif bits == 4:
        p = np.zeros((h, (w + 1) // 2 * 2), np.uint8)
        p[:, :w] = pix
        rows[:, :p.shape[1] // 2] = (p[:, 0::2] << 4) | p[:, 1::2]
    elif bits == 1:
        p = np.zeros((h, (w + 7) // 8 * 8), np.uint8)
        p[:, :w] = pix
        rows[:, :p.shape[1] // 8] = np.packbits(p, axis=1)
    elif bits == 2:
        p = np.zeros((h, (w + 3) // 4 * 4), np.uint8)
        p[:, :w] = pix
        rows[:, :p.shape[1] // 4] = (p[:, 0::4] << 6) | (p[:, 1::4] << 4) | (p[:, 2::4] << 2) | p[:, 3::4]
    elif bits == 24:
        rows[:, :3 * w] = pix[..., ::-1].reshape(h, 3 * w)
    elif bits == 32:
        q = np.full((h, w, 4), 0x5A, np.uint8)  # what no mask covers is not zero
        for c in range(4):
            if pos[c] is not None:
                q[..., pos[c]] = pix[..., c]
        rows[:, :4 * w] = q.reshape(h, 4 * w)
    elif bits == 16:
        rows[:, :2 * w] = np.asarray(pix, np.uint16).astype("<u2").view(np.uint8).reshape(h, 2 * w)
    else:
        raise ValueError(bits)
    if not top_down:
        rows = rows[::-1]
    return rows.tobytes()


def rle_bytes(cmds, rle4=False):
    """An RLE8 / RLE4 stream from explicit commands: ("run", n, v) (v: the value byte; RLE4: two nibbles),
    ("abs", [indices]), ("eol",), ("eob",), ("delta", dx, dy), ("raw", bytes).  An absolute block is padded
    to a 16-bit boundary relative to the start of the stream."""
    out = bytearray()
    for c in cmds:
        if c[0] == "run":
            out += bytes([c[1], c[2]])
        elif c[0] == "abs":
            idx = list(c[1])
            out += bytes([0, len(idx)])
            if rle4:
                idx = idx + [0] * (len(idx) % 2)
                out += bytes((idx[i] << 4) | idx[i + 1] for i in range(0, len(idx), 2))
            else:
                out += bytes(idx)
            if len(out) % 2:
                out.append(0)
        elif c[0] == "eol":
            out += b"\x00\x00"
        elif c[0] == "eob":
            out += b"\x00\x01"
        elif c[0] == "delta":
            out += bytes([0, 2, c[1], c[2]])
        elif c[0] == "raw":
            out += bytes(c[1])
        else:
            raise ValueError(c)
    return bytes(out)


def _run_value(vals, rle4):
    """The value byte of a run over vals (RLE4: alternating high / low nibble), None when it is no run."""
    if not rle4:
        return int(vals[0]) if all(v == vals[0] for v in vals) else None
    a, b = int(vals[0]), int(vals[1]) if len(vals) > 1 else int(vals[0])
    ok = all(int(v) == (a if t % 2 == 0 else b) for t, v in enumerate(vals))
    return (a << 4) | b if ok else None


def rle_commands(idx, rle4=False, mode="mixed", abs_len=255, run_len=255, last_eol=True, eob=True, odd_abs=True):
    """Commands that write idx (h x w, top row first) bottom-up, every row closed by end-of-line.
    mode "runs": encoded runs only; "abs": absolute blocks of abs_len (what is left under 3 pixels as runs
    of 1); "mixed": runs of 3 and more as runs, the rest absolute.  odd_abs False: no absolute block of odd
    length (the pixel left over becomes a run of 1)."""
    idx = np.asarray(idx)
    h, w = idx.shape
    cmds = []
    for r in range(h - 1, -1, -1):
        row = [int(v) for v in idx[r]]
        x = 0
        lit = []

        def flush():
            k = 0
            while len(lit) - k >= 3:
                n = min(abs_len, len(lit) - k)
                if rle4 and n % 2 and n < len(lit) - k:
                    n -= 1  # an odd block only at the end of a stretch (keeps nibble pairs whole)
                if not odd_abs and n % 2:
                    n -= 1
                if n < 3:
                    break
                cmds.append(("abs", lit[k:k + n]))
                k += n
            for v in lit[k:]:
                cmds.append(("run", 1, (v << 4) | v if rle4 else v))
            lit.clear()

        while x < w:
            n = 1
            if mode != "abs":
                while x + n < w and n < run_len and _run_value(row[x:x + n + 1], rle4) is not None:
                    n += 1
            if mode == "runs" or (mode == "mixed" and n >= 3):
                flush()
                cmds.append(("run", n, _run_value(row[x:x + n], rle4)))
                x += n
            else:
                lit.append(row[x])
                x += 1
        flush()
        if r > 0 or last_eol:
            cmds.append(("eol",))
    if eob:
        cmds.append(("eob",))
    return cmds


def bmp(w, h, bits, pix=None, *, header=40, compression=RGB, masks=None, top_down=False, pal=None, clr_used=None,
        gap=0, data=None, planes=1, pos=None, tail=b"", off_bits=None, size_image=None):
    """A BMP file.  pix as pack_rows takes it (pos defaults to the masks' bytes or B, G, R, X); data replaces
    the pixel array (an RLE stream, or anything); pal: n x 3 RGB entries written as the colour table
    (clr_used defaults to its length when that is not 2^bits, else 0); gap: bytes between the tables and the
    pixels; off_bits overrides bfOffBits."""
    if masks is not None and pos is None and data is None:
        pos = tuple(mask_pos(m) for m in (tuple(masks) + (0,))[:4])
    if data is None:
        data = pack_rows(pix, bits, top_down, pos if pos is not None else (2, 1, 0, None))
    if pal is not None and clr_used is None:
        clr_used = 0 if len(pal) == (1 << bits) else len(pal)
    clr_used = clr_used or 0
    hh = -h if top_down else h
    if header == 12:
        info = struct.pack("<IHHHH", 12, w, h, planes, bits)
    else:
        info = struct.pack("<IiiHHIIiiII", header, w, hh, planes, bits, compression,
                           len(data) if size_image is None else size_image, 2835, 2835, clr_used, 0)
        m = tuple(masks) if masks is not None else (0, 0, 0)
        if header >= 52:
            info += struct.pack("<III", *m[:3])
        if header >= 56:
            info += struct.pack("<I", m[3] if len(m) > 3 else 0)
        if header >= 108:
            info += b"BGRs" + bytes(48)
        if header >= 124:
            info += struct.pack("<IIII", 4, 0, 0, 0)
        info += bytes(header - len(info))
        if header == 40 and compression == BITFIELDS:
            info += struct.pack("<III", *m[:3])
    table = b""
    if pal is not None:
        pal = np.asarray(pal, np.uint8)
        entry = np.zeros((len(pal), 3 if header == 12 else 4), np.uint8)
        entry[:, :3] = pal[:, ::-1]
        table = entry.tobytes()
    off = 14 + len(info) + len(table) + gap
    body = info + table + bytes([0xA5]) * gap + data + tail
    return b"BM" + struct.pack("<IHHI", 14 + len(body), 0, 0, off if off_bits is None else off_bits) + body
