"""The references on the content of tests/extreme_cases.py, and that content's
power to tell a wrong kernel from a right one (no GPU).

The oracle in libjpeg mode is pinned to PIL on every file; on the flat-block
files both colour conversions are pinned to integer restatements written
here; each wrong restatement (a constant off by a little, a clamp side
missing, a division for an arithmetic shift) must differ from the oracle on
at least one pixel, or the content could not catch that mistake in a kernel;
the planes reach 0 and 255, the colour sums leave 0..255 on both sides, and
the half-rate chroma planes hold 0 next to 255 along both axes; the resize
reference stays within its bound of Pillow on the contrast images and keeps
both ends of the range in its output."""
import io

import numpy as np
import pytest
from PIL import Image

import extreme_cases as X
from oracle import buckets as B
from oracle import oracle as O

FIR_VS_PILLOW_TOL = 3  # test_oracle_resize.py: fast_image_resize's i16 weights against Pillow's 22-bit ones
SEMS = [O.SEM_LIBJPEG, O.SEM_ZUNE]
SEM_IDS = ["libjpeg", "zune"]
LATTICES = [(s, ac, crop) for s in X.SAMPLINGS for ac in (False, True) for crop in (False, True)]
FLAT = ["lattice", "lattice_crop", "cbcr", "ycb", "ycr"]


def _decode(data, sem=O.SEM_LIBJPEG):
    with O.semantics(sem):
        st, dec = O.jpeg_decode(data)
    assert st == 0
    return dec


def _pil(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.fixture(scope="module")
def lattices():
    return {k: X.ycc_lattice(X.SAMPLINGS[k[0]], 1, k[1], k[2], seed=7) for k in LATTICES}


@pytest.fixture(scope="module")
def flat():
    """{name: (bytes, [Y, Cb, Cr] per block, (w, h))}: the files made of flat
    blocks, whose pixels are known without a decoder."""
    out = {}
    for name, crop in (("lattice", False), ("lattice_crop", True)):
        vals = [z[:, :, 0] + 128 for z in X.lattice_coefs(X.SAMPLINGS["444"], 1, False, 7)]
        out[name] = (X.ycc_lattice(X.SAMPLINGS["444"], 1, False, crop, seed=7), vals,
                     X.lattice_size(X.SAMPLINGS["444"], 1, crop))
    for which in X.PAIR_PLANES:
        out[which] = (X.ycc_pairs(which, seed=3), X.pairs_values(which, seed=3), (X.PAIRS_SIDE, X.PAIRS_SIDE))
    return out


@pytest.fixture(scope="module")
def flat_decoded(flat):
    """{(name, sem): the oracle's pixel per block [bh, bw, 3]}, after checking
    that every block of the oracle's image is flat."""
    out = {}
    for name, (data, vals, (w, h)) in flat.items():
        for sem in SEMS:
            dec = _decode(data, sem)
            assert dec.shape == (h, w, 3)
            blocks = dec[::8, ::8]
            assert np.array_equal(np.kron(blocks, np.ones((8, 8, 1), np.uint8))[:h, :w], dec), (name, sem)
            out[(name, sem)] = blocks.astype(np.int64)
    return out


# ------------------------------------------------------------- restatements
def _shr(x, n):
    return x >> n


def _tdiv(x, n):
    """x / 2**n rounded toward zero: what a division gives where the code means an arithmetic shift."""
    return np.where(x >= 0, x >> n, -((-x) >> n))


def zune_sums(y, cb, cr, k=(45, 11, 23, 113), sh=(_shr, _shr, _shr)):
    """zune-jpeg's scalar ycbcr_to_rgb before its clamp."""
    cb, cr = cb - 128, cr - 128
    return [y + sh[0](k[0] * cr, 5), y - sh[1](k[1] * cb + k[2] * cr, 5), y + sh[2](k[3] * cb, 6)]


def libjpeg_sums(y, cb, cr, k=(91881, 116130, 46802, 22554), sh=(_shr, _shr, _shr)):
    """libjpeg's jdcolor.c tables (SCALEBITS 16, ONE_HALF 32768) before the range limit."""
    cb, cr = cb - 128, cr - 128
    return [y + sh[0](k[0] * cr + 32768, 16), y + sh[1](-k[3] * cb - k[2] * cr + 32768, 16),
            y + sh[2](k[1] * cb + 32768, 16)]


SUMS = {O.SEM_LIBJPEG: libjpeg_sums, O.SEM_ZUNE: zune_sums}


def finish(sums, no_low=None, no_high=None):
    """Clamp to 0..255; channel no_low / no_high lacks that side of the clamp
    and wraps to uint8 there instead."""
    out = []
    for c, v in enumerate(sums):
        lo = v & 255 if c == no_low else 0
        hi = v & 255 if c == no_high else 255
        out.append(np.where(v < 0, lo, np.where(v > 255, hi, v)))
    return np.stack(out, axis=2)


def _mutations():
    """[(id, semantics, kwargs of the sums, kwargs of finish)]"""
    out = []
    for sem, name, consts, step in ((O.SEM_ZUNE, "zune", (45, 11, 23, 113), 1),
                                    (O.SEM_LIBJPEG, "libjpeg", (91881, 116130, 46802, 22554), 64)):
        for i, c in enumerate(consts):
            for d in (-step, step):
                k = list(consts)
                k[i] = c + d
                out.append(("%s_const_%d%+d" % (name, c, d), sem, {"k": tuple(k)}, {}))
        for ch in range(3):
            out.append(("%s_no_low_clamp_%s" % (name, "rgb"[ch]), sem, {}, {"no_low": ch}))
            out.append(("%s_no_high_clamp_%s" % (name, "rgb"[ch]), sem, {}, {"no_high": ch}))
            sh = [_shr] * 3
            sh[ch] = _tdiv
            out.append(("%s_division_%s" % (name, "rgb"[ch]), sem, {"sh": tuple(sh)}, {}))
    return out


MUTATIONS = _mutations()


# ------------------------------------------------------------------- tests
def test_libjpeg_mode_equals_pil_on_every_file(lattices, flat):
    files = [(k, d) for k, d in lattices.items()] + [(k, v[0]) for k, v in flat.items()]
    for label, data in files:
        assert np.array_equal(_decode(data), _pil(data)), label


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_colour_conversion_equals_its_restatement_on_flat_blocks(flat, flat_decoded, sem):
    for name, (_, vals, _) in flat.items():
        want = finish(SUMS[sem](*vals))
        got = flat_decoded[(name, sem)]
        bad = np.argwhere(want != got)
        assert bad.size == 0, (name, bad[0].tolist(), [int(v[bad[0][0], bad[0][1]]) for v in vals])


def test_the_two_semantics_differ_on_this_content(lattices):
    for key, data in lattices.items():
        assert int((_decode(data, O.SEM_LIBJPEG) != _decode(data, O.SEM_ZUNE)).any(axis=2).sum()) > 1000, key


@pytest.mark.parametrize("mutation", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_wrong_colour_conversion_changes_a_pixel(flat, flat_decoded, mutation):
    _, sem, sums_kw, finish_kw = mutation
    changed = 0
    for name, (_, vals, _) in flat.items():
        changed += int((finish(SUMS[sem](*vals, **sums_kw), **finish_kw) != flat_decoded[(name, sem)]).sum())
    assert changed > 0


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_colour_sums_leave_the_range_on_both_sides(flat, sem):
    for name, (_, vals, _) in flat.items():
        for ch, v in zip("rgb", SUMS[sem](*vals)):
            assert v.min() < 0 and v.max() > 255, (name, ch, int(v.min()), int(v.max()))


@pytest.fixture(scope="module")
def planes():
    """{(sampling, ac, component, sem): the oracle's decode of that plane alone}"""
    out = {}
    for s, samp in X.SAMPLINGS.items():
        for ac in (False, True):
            comps = X.lattice_coefs(samp, 1, ac, 7)
            for ci in range(3):
                data = X.plane_of(comps, ci)
                for sem in SEMS:
                    out[(s, ac, ci, sem)] = _decode(data, sem)[:, :, 0]
    return out


def test_every_plane_with_ac_reaches_both_ends(planes):
    for (s, ac, ci, sem), p in planes.items():
        if ac:
            assert p.min() == 0 and p.max() == 255, (s, ci, sem)


def _adjacent_extremes(p, axis):
    a, b = (p[:, :-1], p[:, 1:]) if axis == 1 else (p[:-1], p[1:])
    return bool((((a == 0) & (b == 255)) | ((a == 255) & (b == 0))).any())


def test_half_rate_chroma_holds_0_next_to_255(planes):
    for (s, ac, ci, sem), p in planes.items():
        if s != "444" and ci > 0:
            assert _adjacent_extremes(p, 1), (s, ac, ci, sem, "horizontal")
            assert _adjacent_extremes(p, 0), (s, ac, ci, sem, "vertical")


def _resize_cases():
    out = [(label, kind, w, h, ch, sq, seed, True, (224, 16, 0.5, 2.0))
           for label, kind, w, h, ch, sq, seed in X.png_cases() if ch in (1, 3)]
    out += [(label, kind, w, h, ch, sq, 0, False, (512, 16, 0.5, 2.0)) for label, kind, w, h, ch, sq, _ in X.JPEG_CASES]
    return out


RESIZE_CASES = _resize_cases()


@pytest.mark.parametrize("case", RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_fir_resize_of_contrast_images(case):
    """MODE_FIR (what the GPU computes) against MODE_PILLOW (pinned to PIL by
    test_oracle_resize.py) on L and RGB; PIL does not premultiply, so the
    alpha cases have no such reference."""
    label, kind, w, h, ch, sq, seed, noisy, cfg = case
    src = X.contrast(kind, w, h, ch, sq, seed, noisy=noisy)
    tw, th = B.ARAwareTransform(*cfg).target_size(w, h)
    fir = O.crop_and_resize(src, tw, th, O.MODE_FIR)
    pil = O.crop_and_resize(src, tw, th, O.MODE_PILLOW)
    d = np.abs(fir.astype(int) - pil.astype(int))
    assert d.max() <= FIR_VS_PILLOW_TOL, int(d.max())
    if kind in ("checker", "vstripes", "hstripes"):
        for c in range(fir.shape[2]):
            assert fir[:, :, c].min() == 0 and fir[:, :, c].max() == 255, (c, int(fir[:, :, c].min()),
                                                                          int(fir[:, :, c].max()))
