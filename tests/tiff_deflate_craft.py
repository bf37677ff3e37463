"""The Deflate TIFFs the tiff_deflate tests share (tiff_craft.tiff with comp=8 and a zlib closure as the packer)."""
import zlib

import numpy as np

import tiff_craft as T


def z(level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, every=0, **kw):
    """Segment bytes -> zlib stream; every > 0: a Z_FULL_FLUSH after each `every` bytes."""
    def pack(d):
        c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy, **kw)
        parts = [c.compress(d[i:i + every]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(d), every)] if every else [c.compress(d)]
        return b"".join(parts) + c.flush()
    return pack


def mix():
    a = T.noise(70, 97, 3, 1)
    a[10:40, 20:90] = 9
    return a


def cases():
    """(group, label, file, pixels) of every crafted file that decodes; 97 x 70 RGB unless the label says otherwise."""
    m, n4, out = mix(), T.noise(70, 97, 4, 3), []

    def add(group, label, arr, pack=z(), **kw):
        out.append((group, label, T.tiff(arr, pack=pack, **dict(dict(comp=8), **kw)), np.asarray(arr)))
    geo = np.minimum(np.random.default_rng(5).geometric(0.5, 20370) - 1, 40).astype(np.uint8).reshape(70, 97, 3)
    flat, ramp = np.full((70, 97, 3), 7, np.uint8), (np.arange(20370) % 251).astype(np.uint8).reshape(70, 97, 3)
    add("blocks", "stored", m, z(0))
    add("blocks", "fixed", m, z(6, zlib.Z_FIXED))
    add("blocks", "level 9", m, z(9))
    add("blocks", "huffman only", m, z(6, zlib.Z_HUFFMAN_ONLY))
    add("blocks", "full flush every 100", m, z(6, every=100))
    add("blocks", "compression 32946", m, comp=32946)
    add("blocks", "wbits 9", m, z(6, wbits=9))
    add("blocks", "geometric", geo)
    add("blocks", "geometric huffman only", geo, z(6, zlib.Z_HUFFMAN_ONLY))
    add("blocks", "geometric full flush every 3000", geo, z(6, every=3000))  # dynamic headers anywhere in the source window
    add("matches", "flat rle", flat, z(6, zlib.Z_RLE))
    add("matches", "flat level 9", flat, z(9))
    add("matches", "ramp 251", ramp, z(9))
    add("matches", "mix", m)
    for rps in (1, 7, 70):
        add("layout", "pred rps %d" % rps, m, pred=2, rps=rps)
    add("layout", "tiles 32x48 pred", m, pred=2, tile=(32, 48))
    add("layout", "Rgba8 tiles 32x32 pred", n4, pred=2, tile=(32, 32))
    add("layout", "MM gray rps 7", m[:, :, 0], be=True, rps=7)
    for ph in range(4):
        add("layout", "phase %d" % ph, m, rps=7, phase=ph)
    big = T.noise(150, 151, 3, 8)  # one strip of 67,950 bytes: over what k_tiff_inflate keeps in LDS
    big[40:90] = 5
    add("layout", "pred big strip 151x150", big, pred=2)
    add("layout", "missing trailer", m, lambda d: z()(d)[:-4])
    add("layout", "extra output", m, lambda d: z()(d + b"more" * 50))
    return out


def refusals():
    """(label, file) of the streams the kernel refuses, as Pillow does."""
    good = z()(mix().tobytes())
    fdict = zlib.compressobj(6, zlib.DEFLATED, 15, 9, 0, b"a preset dictionary")
    streams = [("wrong Adler-32", good[:-1] + bytes([good[-1] ^ 1])), ("cut at 100 bytes", good[:100]),
               ("raw deflate", z(wbits=-15)(mix().tobytes())), ("FDICT", fdict.compress(mix().tobytes()) + fdict.flush()),
               ("block type 3", b"\x78\x9c\x07" + b"\0" * 8), ("bad NLEN", b"\x78\x9c\x01\x05\x00\x00\x00abcde"),
               # a fixed block: length code 257 (0000001), distance code 0: distance 1 with no byte before it
               ("distance before the first byte", b"\x78\x9c\x03\x02" + b"\0" * 8)]
    return [(label, T.tiff(mix(), comp=8, pack=lambda d, s=s: s)) for label, s in streams]
