"""16-bit TIFFs for the tiff16 tests: a thin wrapper over tiff_craft.tiff, which writes the samples' bytes as an 8-bit
gray image of twice the width and takes the tags that say what they are.  Pillow reads the gray files back exactly."""
import zlib

import numpy as np

import tiff_craft as T


def tiff16(label, arr, be=False, pred=1, tile=None, tags=(), **kw):
    """arr: H x W [x C] uint16 -> (label, file, arr).  Predictor 2 runs on whole samples modulo 65536, per segment
    row: from a tile's left edge anew.  kw (comp, rps, phase, pack) and tags go to tiff_craft.tiff."""
    a = np.asarray(arr, np.uint16)
    s = (a[:, :, None] if a.ndim == 2 else a).copy()
    H, W, C = s.shape
    if pred == 2:
        first = s[:, ::tile[0] if tile else W].copy()
        s[:, 1:] -= s[:, :-1].copy()
        s[:, ::tile[0] if tile else W] = first
    raw = s.astype(">u2" if be else "<u2").view(np.uint8).reshape(H, W * 2 * C)
    over = [(256, 4, [W]), (258, 3, [16] * C), (277, 3, [C]), (262, 3, [1 if C < 3 else 2]), (317, 3, [pred]),
            (338, 3, [2] if C in (2, 4) else None)] + ([(322, 4, [tile[0]])] if tile else [])
    return label, T.tiff(raw, be=be, tile=(tile[0] * 2 * C, tile[1]) if tile else None, tags=over + list(tags), **kw), a


def noise16(h, w, c, seed):
    """Full-range samples; row 1 alternates 0x00FF and 0x0001, whose byte-wise sums differ from the sample-wise ones."""
    a = np.random.default_rng(seed).integers(0, 65536, (h, w, c), dtype=np.uint16)
    a[1].reshape(-1)[:] = np.resize(np.array([0x00FF, 0x0001], np.uint16), w * c)
    return a[:, :, 0] if c == 1 else a


def forms():
    """(label, file, pixels) of the 97 x 70 forms; the Deflate one needs option tiff_deflate."""
    g, la, n3, n4 = (noise16(70, 97, c, 40 + c) for c in (1, 2, 3, 4))
    out = [tiff16("raw phase %d" % ph, (g, n3, la, n4)[ph], be=ph & 1 == 1, phase=ph) for ph in range(4)]
    out += [tiff16("packbits", n3, comp=32773, rps=9), tiff16("MM packbits gray", g, be=True, comp=32773)]
    out += [tiff16("lzw rps %d" % rps, n3, comp=5, pred=2, rps=rps, be=rps == 7) for rps in (1, 7, 70)]
    for tile in ((16, 16), (32, 48)):
        out += [tiff16("tiles %dx%d raw" % tile, n3, tile=tile, be=True, phase=1),
                tiff16("tiles %dx%d lzw pred" % tile, n4, tile=tile, comp=5, pred=2),
                tiff16("tiles %dx%d lzw pred gray" % tile, g, tile=tile, comp=5, pred=2, be=True)]
    out.append(tiff16("Rgba16 without ExtraSamples", n4, comp=5, tags=[(338, 3, None)]))
    out.append(tiff16("deflate pred", la, comp=8, pred=2, rps=16, pack=zlib.compress))
    return out


def refusals():
    """(label, file, corrupt) of what stays refused with the option on; "stream" files are refused by a kernel."""
    g, n3, n4 = noise16(8, 20, 1, 5), noise16(8, 20, 3, 6), noise16(8, 20, 4, 7)
    return [tiff16(label, arr, **kw)[:2] + (corrupt,) for label, arr, kw, corrupt in [
        ("16-bit WhiteIsZero", g, dict(tags=[(262, 3, [0])]), False), ("SampleFormat 2", n3, dict(tags=[(339, 3, [2] * 3)]), False),
        ("SampleFormat 3", n3, dict(tags=[(339, 3, [3] * 3)]), False), ("BitsPerSample 16 16 8", n3, dict(tags=[(258, 3, [16, 16, 8])]), False),
        ("predictor 2 uncompressed", n3, dict(tags=[(317, 3, [2])]), False), ("associated alpha", n4, dict(tags=[(338, 3, [1])]), False),
        ("one byte short", n3, dict(tags=[(279, 4, [2 * n3.size - 1])]), True),
        ("stream: short LZW", noise16(70, 97, 3, 8), dict(comp=5, pack=lambda d: T.lzw(d)[:100]), True)]]
