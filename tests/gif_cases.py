"""The crafted GIF files that the tests of context option "gif" share
(test_gif_cpu.py, test_gpu_gif.py): stream cases that reach every edge of the
LZW decode, frame cases for the placement on the screen, and the refusals
with the status and text each must give."""
import numpy as np

import gif_craft as G
import ref_gif as R


def noise(h, w, ncol, seed):
    return np.random.default_rng(seed).integers(0, ncol, (h, w)).astype(np.uint8)


def photo(h, w, ncol, seed):
    """Smooth ramps plus a little noise: long and short strings mixed."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = (x * 3 + y * 5) // 7 + rng.integers(0, 2, (h, w))
    return (v % ncol).astype(np.uint8)


def _simple(w, h, idx, mcs, ncol, seed=1, **kw):
    return G.gif(w, h, idx, mcs, gct=G.palette(ncol, seed), **kw)


def stream_cases():
    out = []
    for w, h in [(1, 1), (1, 7), (7, 1), (37, 29), (131, 67)]:
        out.append(("photo %dx%d" % (w, h), _simple(w, h, photo(h, w, 8, w + h), 3, 8)))
    out.append(("noise 128x64 full clears", _simple(128, 64, noise(64, 128, 256, 2), 8, 256)))
    out.append(("noise 128x96 deferred", _simple(128, 96, noise(96, 128, 256, 3), 8, 256, full="defer")))
    out.append(("flat 300x200", _simple(300, 200, np.full((200, 300), 5, np.uint8), 3, 8)))
    out.append(("flat 300x200 deferred mcs2", _simple(300, 200, np.zeros((200, 300), np.uint8), 2, 4, full="defer")))
    out.append(("clear every 7", _simple(61, 23, photo(23, 61, 32, 4), 5, 32, clear_every=7)))
    out.append(("clear every 1", _simple(9, 5, photo(5, 9, 8, 5), 3, 8, clear_every=1)))
    out.append(("no leading clear", _simple(37, 29, photo(29, 37, 8, 6), 3, 8, initial_clear=False)))
    out.append(("no end code", _simple(37, 29, photo(29, 37, 8, 7), 3, 8, eoi=False)))
    for mcs, ncol in [(2, 4), (3, 8), (5, 32), (8, 256)]:
        out.append(("mcs %d noise" % mcs, _simple(45, 31, noise(31, 45, ncol, mcs), mcs, ncol)))
        out.append(("mcs %d photo" % mcs, _simple(90, 50, photo(50, 90, ncol, mcs), mcs, ncol)))
    out.append(("2 colours", _simple(33, 17, noise(17, 33, 2, 8), 2, 2)))
    idx = photo(29, 37, 8, 9)
    data = G.lzw(idx, 3) + bytes(range(1, 40))
    out.append(("garbage after the end code", _simple(37, 29, idx, 3, 8, data=data)))
    data = G.pack_codes(G.lzw_codes(idx, 3, eoi=False) + [8 + 6, 9 + 200, 3], 3)
    out.append(("codes past the last pixel", _simple(37, 29, idx, 3, 8, data=data)))
    second = G.gce() + G.frame_block(noise(29, 37, 8, 10), 3)
    out.append(("second frame", _simple(37, 29, idx, 3, 8, more=second, tail=b"trailing bytes")))
    big = noise(80, 120, 256, 11)
    out.append(("sub-blocks 255", _simple(120, 80, big, 8, 256, sub=255)))
    out.append(("sub-blocks 1", _simple(37, 29, idx, 3, 8, sub=1)))
    out.append(("sub-blocks mixed", _simple(120, 80, big, 8, 256, sub=[3, 1, 7, 2, 255, 5, 254])))
    out.append(("sub-blocks 255 then 254s", _simple(120, 80, big, 8, 256, sub=[255, 254])))
    out.append(("sub-blocks 100", _simple(120, 80, big, 8, 256, sub=100)))
    return out


def frame_cases():
    out = []
    pal = G.palette(8, 21)
    for fh in (1, 2, 3, 4, 5, 8, 9, 67):
        out.append(("interlaced h%d" % fh, G.gif(19, fh, photo(fh, 19, 8, fh), 3, gct=pal, interlace=True)))
    idx = photo(11, 13, 8, 22)
    out.append(("offset inside", G.gif(30, 20, idx, 3, gct=pal, left=5, top=4)))
    out.append(("offset inside interlaced", G.gif(30, 20, idx, 3, gct=pal, left=5, top=4, interlace=True)))
    out.append(("full width, top offset", G.gif(13, 20, idx, 3, gct=pal, left=0, top=6)))
    out.append(("past right and bottom", G.gif(16, 12, idx, 3, gct=pal, left=9, top=7)))
    out.append(("past right and bottom interlaced", G.gif(16, 12, idx, 3, gct=pal, left=9, top=7, interlace=True)))
    out.append(("wholly outside", G.gif(8, 8, idx, 3, gct=pal, left=8, top=2)))
    out.append(("local over global", G.gif(13, 11, idx, 3, gct=pal, lct=G.palette(8, 23))))
    out.append(("local only", G.gif(13, 11, idx, 3, lct=G.palette(8, 24))))
    out.append(("transparent index", G.gif(13, 11, idx, 3, gct=pal, before=[G.gce(transparent=2)])))
    out.append(("transparent index, sub-frame", G.gif(20, 16, idx, 3, gct=pal, left=3, top=2,
                                                      before=[G.gce(transparent=0)])))
    out.append(("two GCEs: the last counts", G.gif(13, 11, idx, 3, gct=pal,
                                                   before=[G.gce(transparent=1), G.gce(transparent=4)])))
    out.append(("transparent index past the table", G.gif(13, 11, idx, 3, gct=pal, before=[G.gce(transparent=200)])))
    out.append(("GIF87a", G.gif(13, 11, idx, 3, gct=pal, version=b"87a")))
    out.append(("extensions", G.gif(13, 11, idx, 3, gct=pal, before=[G.comment(), G.netscape(), G.plain_text(),
                                                                      G.unknown_ext(), G.gce(transparent=3)])))
    out.append(("no trailer", G.gif(13, 11, idx, 3, gct=pal, trailer=False)))
    return out


def refusals():
    """(label, bytes, status, text)."""
    pal = G.palette(8, 31)
    idx = photo(9, 11, 8, 32)
    good_codes = G.lzw_codes(idx, 3)
    out = []

    def add(label, data, st, text):
        out.append((label, data, st, text))

    codes = good_codes[:5] + [15] + good_codes[5:]  # 13 entries by then: two above the next free code
    add("code above next free", G.gif(11, 9, idx, 3, gct=pal, data=G.pack_codes(codes, 3)), R.UNSUPPORTED, R.WHY_CODE)
    codes = [8, 1, 2, 8, 10] + good_codes[1:]  # the next free code straight after a clear
    add("next free after a clear", G.gif(11, 9, idx, 3, gct=pal, data=G.pack_codes(codes, 3)), R.UNSUPPORTED, R.WHY_CODE)
    add("next free as the first code", G.gif(11, 9, idx, 3, gct=pal, data=G.pack_codes([10, 1, 2], 3)),
        R.UNSUPPORTED, R.WHY_CODE)
    add("data runs out", G.gif(11, 9, idx, 3, gct=pal, data=G.lzw(idx, 3)[:20]), R.UNSUPPORTED, R.WHY_SHORT)
    add("early end code", G.gif(11, 9, idx, 3, gct=pal, data=G.pack_codes(good_codes[:9] + [9], 3)),
        R.UNSUPPORTED, R.WHY_SHORT)
    add("no data", G.gif(11, 9, idx, 3, gct=pal, data=b""), R.UNSUPPORTED, R.WHY_SHORT)
    add("index past the table", G.gif(11, 9, idx, 3, gct=pal[:4]), R.UNSUPPORTED, R.WHY_PALETTE)
    for mcs in (0, 1, 9, 12):
        add("min code size %d" % mcs, G.gif(11, 9, idx, 3, gct=pal).replace(b"\x03" + G.sub_blocks(G.lzw(idx, 3)),
                                                                           bytes([mcs]) + G.sub_blocks(G.lzw(idx, 3))),
            R.UNSUPPORTED, "GIF: LZW minimum code size outside 2..8")
    add("zero screen", G.gif(0, 9, idx, 3, gct=pal), R.UNSUPPORTED, "GIF: zero logical screen dimension")
    add("zero frame", G.gif(11, 9, np.zeros((0, 11), np.uint8), 3, gct=pal, data=G.lzw(idx, 3)), R.UNSUPPORTED,
        "GIF: zero frame dimension")
    add("screen over the limit", G.gif(20000, 20000, idx, 3, gct=pal), R.UNSUPPORTED,
        "GIF: screen over image's allocation limit")
    whole = G.gif(11, 9, idx, 3, gct=pal, before=[G.comment()])
    add("ends in the header", whole[:9], R.CORRUPT, "GIF: truncated logical screen descriptor")
    add("ends in the global table", whole[:20], R.CORRUPT, "GIF: truncated global colour table")
    add("ends in an extension", whole[:13 + 24 + 5], R.CORRUPT, "GIF: truncated extension")
    add("ends in the chain", whole[:-6], R.CORRUPT, "GIF: truncated sub-block chain")
    add("no descriptor before the trailer", whole[:13 + 24] + G.comment() + b"\x3B", R.CORRUPT, "GIF: no image descriptor")
    add("no descriptor before the end", whole[:13 + 24] + G.comment(), R.CORRUPT, "GIF: no image descriptor")
    add("no colour table", G.gif(11, 9, idx, 3), R.CORRUPT, "GIF: no colour table")
    add("unknown block", whole[:13 + 24] + b"\x55" + whole[13 + 24:], R.CORRUPT, "GIF: unknown block")
    lct = G.gif(11, 9, idx, 3, lct=pal)
    add("ends in the local table", lct[:13 + 10 + 7], R.CORRUPT, "GIF: truncated local colour table")
    return out
