"""CPU restatement of the BMP decode behind context option "bmp": the header
walk of host/bmp_header.cpp and the pixels of k_bmp_rle / k_bmp_expand, with
the same statuses and texts.

What decodes is what image 0.25's BmpDecoder (restated from its published
source; the crate is not pinned by any test) and Pillow turn into the same
bytes; test_bmp_cpu.py pins this file to Pillow on every decodable case but
two Pillow quirks: Pillow pads an absolute run by the parity of the file
position (the format, and this file, pad relative to the start of the pixel
data) and reads n // 2 bytes for an RLE4 absolute run of odd n (the format
says ceil(n / 2))."""
import struct
from types import SimpleNamespace

import numpy as np

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
RGB, RLE8, RLE4, BITFIELDS = 0, 1, 2, 3

WHY_ROW = "BMP: RLE run or absolute block passes its row's end"
WHY_DELTA = "BMP: RLE delta, early end-of-line or end-of-bitmap leaves pixels unwritten"
WHY_SHORT = "BMP: RLE data ends before the bitmap is complete"
WHY_PALETTE = "BMP: pixel index past the colour table"
STREAM_TEXTS = (WHY_ROW, WHY_DELTA, WHY_SHORT, WHY_PALETTE)

MASKS32 = [(0xFF0000, 0xFF00, 0xFF, 0x0), (0xFF000000, 0xFF0000, 0xFF00, 0x0), (0xFF000000, 0xFF00, 0xFF, 0x0),
           (0xFF000000, 0xFF0000, 0xFF00, 0xFF), (0xFF, 0xFF00, 0xFF0000, 0xFF000000),
           (0xFF0000, 0xFF00, 0xFF, 0xFF000000), (0xFF000000, 0xFF00, 0xFF, 0xFF0000)]
_POS = {0xFF: 0, 0xFF00: 1, 0xFF0000: 2, 0xFF000000: 3, 0: -1}


def parse(d):
    """(status, why, header) as parse_bmp_header gives them."""
    n = len(d)
    h = SimpleNamespace(header_size=0, width=0, height=0, top_down=0, bits=0, compression=0, stride=0, data_off=0,
                        data_len=0, out_c=0, pos=[0, 0, 0, 0], npal=0, pal=np.zeros((256, 4), np.uint8))

    def fail(st, why):
        return st, why, h
    if d[:2] != b"BM":
        return fail(CORRUPT, "not a BMP")
    if n < 14:
        return fail(CORRUPT, "BMP: truncated file header")
    if n < 18:
        return fail(CORRUPT, "BMP: truncated info header")
    off, size = struct.unpack_from("<I", d, 10)[0], struct.unpack_from("<I", d, 14)[0]
    if size in (52, 56, 64):
        return fail(UNSUPPORTED, "BMP: OS/2 2.x, V2 or V3 info header")
    if size not in (12, 40, 108, 124):
        return fail(CORRUPT, "BMP: unknown info header size")
    if n < 14 + size:
        return fail(CORRUPT, "BMP: truncated info header")
    h.header_size = size
    comp = clr = 0
    if size == 12:
        w, ht, planes, bits = struct.unpack_from("<HHHH", d, 18)
    else:
        w, ht, planes, bits, comp = struct.unpack_from("<iiHHI", d, 18)
        clr = struct.unpack_from("<I", d, 46)[0]
    h.top_down = int(ht < 0)
    ht = abs(ht)
    if planes != 1:
        return fail(UNSUPPORTED, "BMP: planes not 1")
    if w < 0:
        return fail(UNSUPPORTED, "BMP: negative width")
    if w == 0 or ht == 0:
        return fail(UNSUPPORTED, "BMP: zero dimension")
    h.width, h.height = w, ht
    if bits == 16:
        return fail(UNSUPPORTED, "BMP: 16 bits per pixel")
    if bits == 2:
        return fail(UNSUPPORTED, "BMP: 2 bits per pixel")
    if bits not in (1, 4, 8, 24) and not (bits == 32 and size != 12):
        return fail(UNSUPPORTED, "BMP: unsupported bits per pixel")
    h.bits = bits
    if comp > BITFIELDS:
        return fail(UNSUPPORTED, "BMP: unsupported compression")
    h.compression = comp
    if (comp == RLE8 and bits != 8) or (comp == RLE4 and bits != 4) or (comp == BITFIELDS and bits < 24):
        return fail(UNSUPPORTED, "BMP: RLE or bit-field compression on a mismatched depth")
    if comp in (RLE8, RLE4) and h.top_down:
        return fail(UNSUPPORTED, "BMP: top-down RLE")
    if comp == RGB and bits == 32 and size != 40:
        return fail(UNSUPPORTED, "BMP: 32-bit BI_RGB under a V4 / V5 header")
    if bits <= 8 and clr > (1 << bits):
        return fail(UNSUPPORTED, "BMP: colour table larger than the depth allows")
    h.out_c = 3
    pos = 14 + size
    if bits >= 24:
        h.pos = [2, 1, 0, -1]
        if comp == BITFIELDS:
            if size == 40:
                if n < pos + 12:
                    return fail(CORRUPT, "BMP: truncated bit masks")
                m = struct.unpack_from("<III", d, pos) + (0,)
                pos += 12
            else:
                m = struct.unpack_from("<IIII", d, 14 + 40)
            if bits == 24:
                if m[:3] != (0xFF0000, 0xFF00, 0xFF):
                    return fail(UNSUPPORTED, "BMP: bit masks outside the supported sets")
            else:
                if tuple(m) not in MASKS32:
                    return fail(UNSUPPORTED, "BMP: bit masks outside the supported sets")
                h.pos = [_POS[x] for x in m]
                if h.pos[3] >= 0:
                    h.out_c = 4
    else:
        entry = 3 if size == 12 else 4
        h.npal = clr if clr else 1 << bits
        if n < pos + entry * h.npal:
            return fail(CORRUPT, "BMP: truncated colour table")
        t = np.frombuffer(d, np.uint8, entry * h.npal, pos).reshape(h.npal, entry)
        h.pal[:h.npal, :3] = t[:, 2::-1]
        h.pal[:h.npal, 3] = 255
        pos += entry * h.npal
    if h.width * h.height * h.out_c > (512 << 20):
        return fail(UNSUPPORTED, "BMP: image over image's allocation limit")
    if off < pos or off > n:
        return fail(CORRUPT, "BMP: pixel data offset inside the headers or past the file")
    h.data_off = off
    h.stride = ((h.width * bits + 31) // 32) * 4
    if comp in (RLE8, RLE4):
        h.data_len = n - off
    else:
        h.data_len = h.stride * h.height
        if off + h.data_len > n:
            return fail(CORRUPT, "BMP: pixel data truncated")
    return OK, "", h


def rle_indices(s, w, h, rle4):
    """(why, index plane in stream row order) of an RLE8 / RLE4 stream; why "" when it decodes."""
    npix = w * h
    out = np.zeros(npix, np.uint8)
    o = pos = 0
    prev_eol = False
    while o < npix:
        if pos + 2 > len(s):
            return WHY_SHORT, out
        a, b = s[pos], s[pos + 1]
        pos += 2
        r = o % w
        if a or b >= 3:
            q = a or b
            if (r == 0 and o and not prev_eol) or r + q > w:
                return WHY_ROW, out
            if a:
                v = [b] if not rle4 else [b >> 4, b & 15]
                out[o:o + q] = [v[t % len(v)] for t in range(q)]
            else:
                nb = (q + 1) // 2 if rle4 else q
                nb_pad = (nb + 1) & ~1
                if pos + nb_pad > len(s):
                    return WHY_SHORT, out
                raw = np.frombuffer(s, np.uint8, nb, pos)
                if rle4:
                    raw = np.stack([raw >> 4, raw & 15], 1).reshape(-1)
                out[o:o + q] = raw[:q]
                pos += nb_pad
            o += q
            prev_eol = False
        elif b == 0:
            if r or not o or prev_eol:
                return WHY_DELTA, out
            prev_eol = True
        else:  # an end-of-bitmap before the last pixel, or a delta
            return WHY_DELTA, out
    return "", out


def decode(d):
    """(status, why, pixels h x w x 3 or 4 uint8 top row first, header)."""
    st, why, h = parse(d)
    if st != OK:
        return st, why, None, h
    W, H = h.width, h.height
    body = bytes(d[h.data_off:h.data_off + h.data_len])
    if h.compression in (RLE8, RLE4):
        why, plane = rle_indices(body, W, H, h.compression == RLE4)
        if why:
            return UNSUPPORTED, why, None, h
        idx = plane.reshape(H, W)[::-1]
    else:
        rows = np.frombuffer(body, np.uint8).reshape(H, h.stride)
        if not h.top_down:
            rows = rows[::-1]
        if h.bits == 8:
            idx = rows[:, :W]
        elif h.bits == 4:
            idx = np.stack([rows >> 4, rows & 15], 2).reshape(H, -1)[:, :W]
        elif h.bits == 1:
            idx = np.unpackbits(rows, axis=1)[:, :W]
        else:
            px = rows[:, :W * h.bits // 8].reshape(H, W, h.bits // 8)
            chans = [px[..., p] for p in h.pos[:3]]
            if h.out_c == 4:
                chans.append(px[..., h.pos[3]])
            return OK, "", np.ascontiguousarray(np.stack(chans, 2)), h
    if (idx >= h.npal).any():
        return UNSUPPORTED, WHY_PALETTE, None, h
    return OK, "", np.ascontiguousarray(h.pal[idx][..., :3]), h
