"""The GIF decode of context option "gif" restated on the CPU: what image
0.25's GifDecoder (gif 0.13 + weezl) returns for load_from_memory -- the first
frame composited on the logical screen as Rgba8 -- with the library's status
rules: structural breaks are CORRUPT, stream irregularities UNSUPPORTED.  The
crates are not available offline, so this is a restatement; test_gif_cpu.py
pins it to Pillow wherever the two agree (indices, palette, transparency,
interlace, frame placement inside the frame's rectangle).

The LZW decoder here is the classic prefix-chain one, on purpose not the
(position, length) scheme of dg_gif.h."""
import numpy as np

OK, UNSUPPORTED, CORRUPT = 0, 1, 2

WHY_CODE = "GIF: LZW code above the next free code"
WHY_SHORT = "GIF: image data ends before the frame is complete"
WHY_PALETTE = "GIF: pixel index past the colour table"


class Parsed:
    pass


def parse(data):
    """-> (status, why, Parsed).  Mirrors host/gif_header.cpp."""
    d, n = bytes(data), len(data)
    h = Parsed()
    h.runs = []
    if n < 6 or d[:6] not in (b"GIF87a", b"GIF89a"):
        return CORRUPT, "not a GIF", h
    h.version = 87 if d[4:5] == b"7" else 89
    if n < 13:
        return CORRUPT, "GIF: truncated logical screen descriptor", h
    h.width, h.height = d[6] | d[7] << 8, d[8] | d[9] << 8
    unsup = None
    if h.width == 0 or h.height == 0:
        unsup = "GIF: zero logical screen dimension"
    pos, table = 13, None
    h.has_global = h.has_local = 0
    if d[10] & 0x80:
        nt = 2 << (d[10] & 7)
        if pos + 3 * nt > n:
            return CORRUPT, "GIF: truncated global colour table", h
        table = d[pos:pos + 3 * nt]
        pos += 3 * nt
        h.has_global = 1
    h.transparent = -1
    while True:
        if pos >= n:
            return CORRUPT, "GIF: no image descriptor", h
        b = d[pos]
        pos += 1
        if b == 0x3B:
            return CORRUPT, "GIF: no image descriptor", h
        if b == 0x2C:
            break
        if b != 0x21:
            return CORRUPT, "GIF: unknown block", h
        if pos >= n:
            return CORRUPT, "GIF: truncated extension", h
        label = d[pos]
        pos += 1
        first = True
        while True:
            if pos >= n:
                return CORRUPT, "GIF: truncated extension", h
            ln = d[pos]
            pos += 1
            if not ln:
                break
            if pos + ln > n:
                return CORRUPT, "GIF: truncated extension", h
            if label == 0xF9 and first and ln >= 4:
                h.transparent = d[pos + 3] if d[pos] & 1 else -1
            first = False
            pos += ln
    if pos + 9 > n:
        return CORRUPT, "GIF: truncated image descriptor", h
    h.left, h.top = d[pos] | d[pos + 1] << 8, d[pos + 2] | d[pos + 3] << 8
    h.fw, h.fh = d[pos + 4] | d[pos + 5] << 8, d[pos + 6] | d[pos + 7] << 8
    packed = d[pos + 8]
    pos += 9
    h.interlace = 1 if packed & 0x40 else 0
    if unsup is None and (h.fw == 0 or h.fh == 0):
        unsup = "GIF: zero frame dimension"
    if packed & 0x80:
        nt = 2 << (packed & 7)
        if pos + 3 * nt > n:
            return CORRUPT, "GIF: truncated local colour table", h
        table = d[pos:pos + 3 * nt]
        pos += 3 * nt
        h.has_local = 1
    if pos >= n:
        return CORRUPT, "GIF: truncated image data", h
    h.min_code_size = d[pos]
    pos += 1
    if unsup is None and not 2 <= h.min_code_size <= 8:
        unsup = "GIF: LZW minimum code size outside 2..8"
    h.data_off = pos
    chunks = []
    while True:
        if pos >= n:
            return CORRUPT, "GIF: truncated sub-block chain", h
        ln = d[pos]
        if not ln:
            break
        if pos + 1 + ln > n:
            return CORRUPT, "GIF: truncated sub-block chain", h
        if h.runs and h.runs[-1][1] == ln:
            h.runs[-1][2] += 1
        else:
            h.runs.append([pos, ln, 1])
        chunks.append(d[pos + 1:pos + 1 + ln])
        pos += 1 + ln
    h.codes = b"".join(chunks)
    h.nbytes = len(h.codes)
    r = h.runs
    h.closed = (not r or (len(r) == 1 and (r[0][1] == 255 or r[0][2] == 1)) or
                (len(r) == 2 and r[0][1] == 255 and r[1][2] == 1))
    if table is None:
        return CORRUPT, "GIF: no colour table", h
    h.npal = len(table) // 3
    pal = np.zeros((256, 4), np.uint8)
    pal[:h.npal, :3] = np.frombuffer(table, np.uint8).reshape(-1, 3)
    pal[:h.npal, 3] = 255
    if h.transparent >= 0:
        pal[h.transparent, 3] = 0
    h.pal = pal
    if unsup is None and h.width * h.height * 4 > (512 << 20):
        unsup = "GIF: screen over image's allocation limit"
    if unsup:
        return UNSUPPORTED, unsup, h
    return OK, "", h


def lzw_decode(codes, mcs, npix):
    """-> (status, why, indices).  Classic prefix-chain LZW, LSB first."""
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    prefix, suffix, length = [0] * 4096, [0] * 4096, [0] * 4096
    for i in range(clear):
        suffix[i], length[i] = i, 1
    out = bytearray()
    nbits = len(codes) * 8
    big = int.from_bytes(codes, "little")
    pos, nf, w, prev = 0, clear + 2, mcs + 1, -1
    while len(out) < npix:
        if pos + w > nbits:
            return UNSUPPORTED, WHY_SHORT, None
        c = (big >> pos) & ((1 << w) - 1)
        pos += w
        if c == clear:
            nf, w, prev = clear + 2, mcs + 1, -1
            continue
        if c == eoi:
            return UNSUPPORTED, WHY_SHORT, None
        if c > nf or (c == nf and prev < 0):
            return UNSUPPORTED, WHY_CODE, None
        if c < nf and (c < clear or c >= clear + 2):
            s = bytearray(length[c])
            k = c
            for i in range(length[c] - 1, -1, -1):
                s[i] = suffix[k]
                k = prefix[k]
        else:  # KwKwK (c == nf; with a full table nf == 4096 is never a code)
            s = bytearray(length[prev] + 1)
            k = prev
            for i in range(length[prev] - 1, -1, -1):
                s[i] = suffix[k]
                k = prefix[k]
            s[-1] = s[0]
        if prev >= 0 and nf < 4096:
            prefix[nf], suffix[nf], length[nf] = prev, s[0], length[prev] + 1
            nf += 1
            if nf == (1 << w) and w < 12:
                w += 1
        out += s
        prev = c
    return OK, "", np.frombuffer(bytes(out[:npix]), np.uint8)


def decode(data):
    """-> (status, why, rgba H x W x 4 or None, info)."""
    st, why, h = parse(data)
    if st != OK:
        return st, why, None, h
    st, why, idx = lzw_decode(h.codes, h.min_code_size, h.fw * h.fh)
    if st != OK:
        return st, why, None, h
    plane = idx.reshape(h.fh, h.fw)
    if h.interlace:
        rows = (list(range(0, h.fh, 8)) + list(range(4, h.fh, 8)) + list(range(2, h.fh, 4)) +
                list(range(1, h.fh, 2)))
        nat = np.empty_like(plane)
        nat[rows] = plane
        plane = nat
    h.indices = plane
    out = np.zeros((h.height, h.width, 4), np.uint8)
    vh = max(0, min(h.fh, h.height - h.top))
    vw = max(0, min(h.fw, h.width - h.left))
    vis = plane[:vh, :vw]
    if vis.size and int(vis.max()) >= h.npal:
        return UNSUPPORTED, WHY_PALETTE, None, h
    out[h.top:h.top + vh, h.left:h.left + vw] = h.pal[vis]
    return OK, "", out, h
