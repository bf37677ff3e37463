"""The bitmaps the bilevel TIFF tests share, each the smallest that reaches one thing k_tiff_g4 can get wrong, and the
two ways a file is made of one: written by Pillow (libtiff), or crafted by tiff_craft around strips Pillow coded."""
import io

import numpy as np
from PIL import Image

import tiff_craft as T

COMP = {"raw": (None, 1), "packbits": ("packbits", 32773), "lzw": ("tiff_lzw", 5), "deflate": ("tiff_adobe_deflate", 8),
        "g4": ("group4", 4)}


def cases():
    """(label, H x W array of 0 / 1 with 1 = white, rows per strip or None for one strip)."""
    rng, out = np.random.default_rng(4), []
    for k, w in enumerate((1, 7, 8, 9, 31, 33, 63, 64, 65, 2049)):  # noise: horizontal mode on nearly every edge
        out.append(("noise %d" % w, rng.integers(0, 2, (5, w)), (None, 1, 3)[k % 3]))
    out += [("height 1", rng.integers(0, 2, (1, 50)), None), ("height 2", rng.integers(0, 2, (2, 50)), 1),
            ("white", np.ones((6, 40), int), 3), ("black", np.zeros((6, 40), int), None)]
    row = rng.integers(0, 2, (1, 300))  # some 150 changing elements: a V0 run over more than one step
    out.append(("equal rows", np.repeat(row, 4, 0), None))
    sparse = np.ones((3, 4500), int)  # V0 runs that look past 2,048 pixels for their next changing element
    sparse[:, 5:4000] = 0
    sparse[:, 4010:4490] = 0
    out += [("sparse equal rows", sparse, None), ("stripes", np.tile(np.arange(70) % 2, (3, 1)), None)]
    y, x = np.mgrid[0:12, 0:80]
    for s in (1, 2, 3, 4):  # VR / VL 1 .. 3, and the fall to horizontal mode at 4
        out += [("edge +%d" % s, (x > 10 + s * y).astype(int), None), ("edge -%d" % s, (x > 70 - s * y).astype(int), 3)]
    dots = np.ones((7, 60), int)  # a dot under white and white under a dot: pass mode
    dots[::2, 5::9] = 0
    out.append(("dots", dots, None))
    for n in (63, 64, 65, 1728, 1792, 2559, 2560, 5300):  # terminating, make-up, shared make-up codes, one repeated
        a = np.ones((2, 2 * n + 1), int)
        a[0, n:2 * n] = 0
        a[1, :n] = 0
        a[1, 2 * n:] = 0
        out.append(("runs %d" % n, a, None))
    page = np.ones((65, 40), int)
    y, x = np.mgrid[0:65, 0:40]
    for cy, cx, r in rng.integers(3, 37, (14, 3)):
        page[(y - 2 * cy + 5) ** 2 + (x - cx) ** 2 < (r / 4) ** 2] = 0
    return out + [("page", page, 16)]


def written(arr, comp, rps=None):
    """The file Pillow writes of a 0 / 1 array with compression COMP[comp], in strips of rps rows."""
    b, kw = io.BytesIO(), {}
    if COMP[comp][0]:
        kw["compression"] = COMP[comp][0]
    if rps:
        kw["tiffinfo"] = {278: rps}
    Image.fromarray(np.asarray(arr, np.uint8) * 255).convert("1").save(b, "TIFF", **kw)
    return b.getvalue()


def g4_strip(bits):
    """The Group 4 stream Pillow codes for rows of bits (1 = a black run's pixels, as T.6 has them)."""
    bits = np.asarray(bits, np.uint8)
    data = written(bits, "g4")
    im = Image.open(io.BytesIO(data))
    assert im.tag_v2[262] == 1 and len(im.tag_v2[273]) == 1  # BlackIsZero: Pillow codes its white pixels as the 1 bits
    return data[im.tag_v2[273][0]:im.tag_v2[273][0] + im.tag_v2[279][0]]


def crafted(arr, g4, photo=1, be=False, tile=None, **kw):
    """A 1-bit file of tiff_craft: arr is 0 / 1 with 1 = the stored bit.  tile = (width, height) in pixels."""
    arr = np.asarray(arr, np.uint8)
    H, W = arr.shape
    tags = [(256, 4, [W]), (258, 3, [1])] + ([(322, 4, [tile[0]])] if tile else []) + list(kw.pop("tags", []))
    sw = tile[0] if tile else W  # a segment's pixels per row: its packed rows are ceil(sw / 8) bytes
    if tile:  # tiff_craft cuts its tiles from whole bytes
        arr = np.pad(arr, ((0, 0), (0, -W % tile[0])))
    pack = (lambda d: g4_strip(np.unpackbits(np.frombuffer(d, np.uint8).reshape(-1, (sw + 7) // 8), axis=1)[:, :sw])) if g4 else None
    return T.tiff(np.packbits(arr, axis=1), comp=4 if g4 else 1, photo=photo, be=be, tile=(tile[0] // 8, tile[1]) if tile else None,
                  pack=kw.pop("pack", pack), tags=tags, **kw)
