"""A GIF writer with full control, for the tests of context option "gif":
version, global / local colour tables of 2..256 entries, Graphic Control and
other extensions, the frame rectangle, interlace, the LZW minimum code size,
the sub-block lengths, and an LZW encoder whose clear behaviour is chosen
(clear when the table is full, deferred clear, a clear every n codes, no
leading clear, no end code).  Code lists can also be packed as they are, so
irregular streams are spelled out code by code."""
import struct

import numpy as np

MAX_CODES = 4096


def code_width(nf, mcs):
    """Bits of a code read while the decoder's table holds nf entries."""
    return min(12, max(mcs + 1, int(nf).bit_length()))


def pack_codes(codes, mcs):
    """LSB-first packing with the widths a decoder reading these codes would use."""
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    nf, prev, acc, nbits, out = clear + 2, False, 0, 0, bytearray()
    ended = False
    for c in codes:
        w = code_width(nf, mcs)
        acc |= (int(c) & ((1 << w) - 1)) << nbits
        nbits += w
        while nbits >= 8:
            out.append(acc & 255)
            acc >>= 8
            nbits -= 8
        if ended:
            continue
        if c == clear:
            nf, prev = clear + 2, False
        elif c == eoi:
            ended = True
        else:
            if prev and nf < MAX_CODES:
                nf += 1
            prev = True
    if nbits:
        out.append(acc & 255)
    return bytes(out)


def lzw_codes(indices, mcs, full="clear", clear_every=0, initial_clear=True, eoi=True):
    """The code list of an LZW encoder over `indices` (all < 2 ** mcs).

    full: "clear" = a clear code when the table is full, "defer" = no more
    entries, the table stays in use.  clear_every = n: a clear after every n
    data codes."""
    clear, end = 1 << mcs, (1 << mcs) + 1
    codes = [clear] if initial_clear else []
    table, nxt, since = {}, clear + 2, 0
    idx = [int(v) for v in np.asarray(indices).reshape(-1)]
    if not idx:
        return codes + ([end] if eoi else [])
    w = idx[0]
    for k in idx[1:]:
        key = (w, k)
        if key in table:
            w = table[key]
            continue
        codes.append(w)
        since += 1
        if nxt < MAX_CODES:
            table[key] = nxt
            nxt += 1
        reset = clear_every and since >= clear_every
        if nxt >= MAX_CODES and full == "clear":
            reset = True
        if reset:
            codes.append(clear)
            table, nxt, since = {}, clear + 2, 0
        w = k
    codes.append(w)
    if eoi:
        codes.append(end)
    return codes


def lzw(indices, mcs, **kw):
    return pack_codes(lzw_codes(indices, mcs, **kw), mcs)


def sub_blocks(data, lengths=255):
    """The sub-block chain of `data`: lengths = one size, or a list cycled through."""
    ls = [lengths] if isinstance(lengths, int) else list(lengths)
    out, pos, i = bytearray(), 0, 0
    while pos < len(data):
        n = min(ls[i % len(ls)], len(data) - pos)
        out.append(n)
        out += data[pos:pos + n]
        pos += n
        i += 1
    out.append(0)
    return bytes(out)


def _table(colours):
    """(size field, bytes) of a colour table padded with black to a power of two."""
    n = max(2, len(colours))
    bits = max(1, (n - 1).bit_length())
    raw = bytearray()
    for c in colours:
        raw += bytes(int(v) & 255 for v in c)
    raw += bytes(3 * ((1 << bits) - len(colours)))
    return bits - 1, bytes(raw)


def palette(n, seed=1):
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(n)]


def interlace_rows(fh):
    return list(range(0, fh, 8)) + list(range(4, fh, 8)) + list(range(2, fh, 4)) + list(range(1, fh, 2))


def gce(transparent=None, disposal=0, delay=0):
    packed = (disposal << 2) | (1 if transparent is not None else 0)
    return b"\x21\xF9\x04" + struct.pack("<BHB", packed, delay, 0 if transparent is None else transparent) + b"\x00"


def comment(text=b"made by gif_craft"):
    return b"\x21\xFE" + sub_blocks(text, 7)


def netscape(loops=0):
    return b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loops) + b"\x00"


def plain_text():
    return b"\x21\x01\x0C" + struct.pack("<HHHHBBBB", 0, 0, 8, 8, 8, 8, 1, 0) + sub_blocks(b"hello", 3)


def unknown_ext():
    return b"\x21\x77" + sub_blocks(b"\x01\x02\x03\x04\x05", 2)


def frame_block(indices, mcs, left=0, top=0, lct=None, interlace=False, sub=255, data=None, **lzw_kw):
    """Image descriptor + local table + min code size + sub-blocks of one frame.

    indices: fh x fw array in display order (reordered here when interlaced);
    data: the LZW bytes to use instead of encoding `indices`."""
    idx = np.asarray(indices)
    fh, fw = idx.shape
    if interlace:
        idx = idx[interlace_rows(fh)]
    packed, tab = (0x40 if interlace else 0), b""
    if lct is not None:
        bits, tab = _table(lct)
        packed |= 0x80 | bits
    if data is None:
        data = lzw(idx, mcs, **lzw_kw)
    return b"\x2C" + struct.pack("<HHHHB", left, top, fw, fh, packed) + tab + bytes([mcs]) + sub_blocks(data, sub)


def gif(width, height, indices, mcs, gct=None, lct=None, version=b"89a", left=0, top=0, interlace=False,
        before=(), sub=255, data=None, trailer=True, tail=b"", more=b"", bg=0, **lzw_kw):
    """A whole file: header, screen descriptor, global table, the blocks in
    `before`, the first frame, `more` (further blocks, e.g. a second frame),
    the trailer and `tail`."""
    packed, tab = 0, b""
    if gct is not None:
        bits, tab = _table(gct)
        packed = 0x80 | (bits << 4) | bits
    out = b"GIF" + version + struct.pack("<HHBBB", width, height, packed, bg, 0) + tab
    for b in before:
        out += b
    out += frame_block(indices, mcs, left, top, lct, interlace, sub, data, **lzw_kw)
    out += more
    if trailer:
        out += b"\x3B"
    return out + tail
