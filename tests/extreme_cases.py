"""Content at the ends of the pixel range, for the stages whose arithmetic
depends on pixel value: YCbCr -> RGB (both decode semantics), chroma
upsampling, the clamps after the IDCT and after each resize pass, the packed
i16 pairs and the i8 matrix-core split of the H passes, the alpha programs.

JPEGs are built from chosen coefficients (tests/jpeg_craft.py), so a flat block
decodes to exactly the value asked for; pixel arrays go through synth.pil_png
or jpeg_craft.from_pixels.  Everything is seeded.  A plain helper module shared
by the CPU tests (test_extremes_cpu.py) and the GPU tests
(test_gpu_extremes.py).
"""
import numpy as np

import jpeg_craft as J

V = [0, 1, 16, 127, 128, 129, 240, 254, 255]  # the lattice: both ends, their neighbours, the centre, studio range
TILE = 27                                     # MCUs per tile side: 27 * 27 = 9 ** 3 triples
Q = 8                                         # every quantiser: DC (v - 128) dequantises to a flat block of v
SAMPLINGS = {"444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}
AC_NATURAL = (1, 8, 7, 56, 63)                # lowest and highest frequency of each axis, and of both
_NAT_TO_ZZ = {int(n): z for z, n in enumerate(J.ZIGZAG)}
KINDS = ("checker", "vstripes", "hstripes", "impulse", "inv_impulse")


def _qtabs():
    return [np.full(64, Q)] * 2


def lattice_size(samp, tiles, crop=False):
    """(width, height) of ycc_lattice(samp, tiles, ..., crop)."""
    w, h = TILE * tiles * 8 * samp[0][0], TILE * tiles * 8 * samp[0][1]
    return (w - 5, h - 3) if crop else (w, h)


def lattice_coefs(samp, tiles, ac, seed):
    """Per component the zigzag coefficients [bh, bw, 64] of the lattice: in
    each of the tiles x tiles tiles, MCU k of that tile's own seeded
    permutation of 0..728 holds (Y, Cb, Cr) = V[digits of k in base 9] as the
    DC of every block of the MCU; with `ac`, every block also holds one
    coefficient in [-127, 127] at a seeded one of AC_NATURAL."""
    rng = np.random.default_rng(seed)
    n = TILE * tiles
    k = np.empty((n, n), np.int64)
    for ty in range(tiles):
        for tx in range(tiles):
            k[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = rng.permutation(TILE * TILE).reshape(TILE, TILE)
    val = np.asarray(V)
    per_mcu = [val[k // 81], val[(k // 9) % 9], val[k % 9]]
    out = []
    for (hs, vs), v in zip(samp, per_mcu):
        z = np.zeros((n * vs, n * hs, 64), np.int64)
        z[:, :, 0] = np.repeat(np.repeat(v, vs, axis=0), hs, axis=1) - 128
        if ac:
            pos = np.asarray([_NAT_TO_ZZ[p] for p in AC_NATURAL])[rng.integers(0, len(AC_NATURAL), z.shape[:2])]
            amp = rng.integers(-127, 128, z.shape[:2])
            np.put_along_axis(z, pos[:, :, None], amp[:, :, None], axis=2)
        out.append(z)
    return out


def ycc_lattice(samp, tiles=1, ac=False, crop=False, seed=0):
    """The lattice as a baseline JPEG (module docstring, lattice_coefs).
    crop: the declared size is 5 pixels narrower and 3 shorter than the MCU
    grid, so the MCU-padded last columns and rows hold lattice values too."""
    w, h = lattice_size(samp, tiles, crop)
    return J.from_coefs(lattice_coefs(samp, tiles, ac, seed), samp, w, h, _qtabs())


PAIR_PLANES = {"cbcr": (1, 2, 0), "ycb": (0, 1, 2), "ycr": (0, 2, 1)}  # (by column, by row, seeded)
PAIRS_SIDE = 2048


def pairs_values(which, seed=0):
    """[Y, Cb, Cr] per block, each [256, 256]: two planes run over 0..255 by
    block column and by block row (all 65,536 pairs), the third is seeded."""
    col, row, free = PAIR_PLANES[which]
    v = [None] * 3
    v[col] = np.tile(np.arange(256), (256, 1))
    v[row] = v[col].T.copy()
    v[free] = np.random.default_rng(seed).integers(0, 256, (256, 256))
    return v


def ycc_pairs(which, seed=0):
    """A 2048 x 2048 4:4:4 DC-only JPEG of 256 x 256 flat blocks (pairs_values)."""
    comps = []
    for v in pairs_values(which, seed):
        z = np.zeros((256, 256, 64), np.int64)
        z[:, :, 0] = v - 128
        comps.append(z)
    return J.from_coefs(comps, SAMPLINGS["444"], PAIRS_SIDE, PAIRS_SIDE, _qtabs())


def plane_of(comps, ci):
    """Component `ci` of a lattice alone, as a 1-component JPEG of the same
    coefficients: what a decoder makes of it is the plane the colour file
    holds before upsampling and colour conversion."""
    z = np.asarray(comps[ci])
    return J.from_coefs([z], [(1, 1)], z.shape[1] * 8, z.shape[0] * 8, _qtabs())


# Contrast PNG sources for a 224/16 context: (w, h, square); square is about
# 4 x the downscale factor.  H scale, taps (ksize) and what the size is for:
#   211 x 213   -> 224 x 224  0.94   7  upscale; integral y crop (224 x 226, top 1)
#   427 x 213   -> 304 x 160  1.33   9  <= 16 taps; x.5 crop (321 x 160, left 8.5)
#   432 x 432   -> 224 x 224  1.93  13  <= 16 taps, no crop
#   859 x 861   -> 224 x 224  3.83  25  <= 32 taps; y.5 crop (224 x 225)
#   1296 x 1296 -> 224 x 224  5.79  37  more taps than any fixed class: weights from memory
#   1920 x 1000 -> 304 x 160  6.25  39  the same, 1.9 MP, x.5 crop (307 x 160, left 1.5)
# From a scale of about 4.5 the H pass's source segment no longer fits the band
# kernels' LDS, so the last two also run the direct H kernel.
PNG_SIZES = [(211, 213, 1), (427, 213, 5), (432, 432, 8), (859, 861, 15), (1296, 1296, 23), (1920, 1000, 25)]
PNG_CHANNELS = (1, 2, 3, 4)  # L, LA, RGB, RGBA


def png_cases():
    """[(label, kind, w, h, channels, square, seed)]: every size for every
    channel count, the kinds in rotation so that each channel count sees all."""
    out = []
    for ci, ch in enumerate(PNG_CHANNELS):
        for si, (w, h, sq) in enumerate(PNG_SIZES):
            kind = KINDS[(si + ci) % len(KINDS)]
            out.append(("%s_%dx%d_c%d" % (kind, w, h, ch), kind, w, h, ch, sq, 100 * ci + si))
    return out


# Contrast sources for the JPEG path at 512/16 (from_pixels at quality 100):
# (label, kind, w, h, channels, square, sampling).  The squares are multiples
# of the MCU, so every block is flat and the planes hold exactly 0 and 255.
JPEG_CASES = [("gray_4000x3000", "checker", 4000, 3000, 1, 32, [(1, 1)]),
              ("444_4000x3000", "vstripes", 4000, 3000, 3, 32, SAMPLINGS["444"]),
              ("420_6400x4000", "checker", 6400, 4000, 3, 64, SAMPLINGS["420"])]


def _cells(kind, w, h, square):
    """Boolean [h, w]: where the pattern is high."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "checker":
        return ((x // square + y // square) & 1) == 1
    if kind == "vstripes":
        return ((x // square) & 1) == 1
    if kind == "hstripes":
        return ((y // square) & 1) == 1
    if kind in ("impulse", "inv_impulse"):
        # isolated pixels further apart than the filter's support (3 x the
        # downscale factor each side when square is about 4 x the factor); an
        # odd pitch, so the pixels fall on every phase of the output grid
        pitch = max(7, 2 * square + 1)
        hit = (x % pitch == pitch // 2) & (y % pitch == pitch // 2)
        return hit if kind == "impulse" else ~hit
    raise ValueError(kind)


def contrast(kind, w, h, channels=1, square=1, seed=0, noisy=False):
    """uint8 [h, w] (channels 1) or [h, w, channels] of 0 / 255 content (KINDS).
    Colour channel 1 is the inverse of channel 0 and channel 2 is channel 0
    moved half a square, so no two channels agree.  noisy: each low sample is
    drawn from 0..3 and each high one from 252..255 (an ordinary zlib stream
    when the array is written as a PNG).  With 2 or 4 channels the last is
    alpha: its own checkerboard over {0, 1, 128, 255}, half a square out of
    phase with the colour."""
    rng = np.random.default_rng(seed)
    nc = channels - (channels in (2, 4))
    hi = _cells(kind, w, h, square)
    step = (square + 1) // 2
    planes = [hi, ~hi, np.roll(hi, step, axis=1)][:nc]
    out = []
    for p in planes:
        v = np.where(p, 255, 0)
        if noisy:
            v = np.where(p, 255 - rng.integers(0, 4, (h, w)), rng.integers(0, 4, (h, w)))
        out.append(v)
    if channels in (2, 4):
        y, x = np.mgrid[0:h, 0:w]
        out.append(np.asarray([0, 1, 128, 255])[((x + step) // square + 2 * ((y + step) // square)) % 4])
    arr = np.stack(out, axis=2).astype(np.uint8)
    return arr[:, :, 0] if channels == 1 else arr
