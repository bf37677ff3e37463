"""The crafted coefficient streams (tests/coef_patterns.py) are what they
claim to be, and can catch a wrong part mask: the oracle reads back exactly
the coefficients written, and zeroing any single stored part of a
mask_sweep block changes that block's decoded pixels in both semantics -- so
a decoder that drops a stored part cannot pass test_gpu_coef_patterns.py."""
import numpy as np
import pytest

import coef_patterns as P
import jpeg_craft as J
from oracle import oracle as O


def _decode(data, sem):
    with O.semantics(sem):
        st, dec = O.jpeg_decode(data)
    assert st == 0
    return dec


@pytest.mark.parametrize("geo", list(P.GEOS))
def test_streams_hold_the_coefficients_written(geo):
    for comps, q in ((P.sweep_coefs(geo), P.Q_SWEEP), (P.dense_coefs(geo), P.Q_DENSE), (P.zero_coefs(geo), 16)):
        st, co = O.jpeg_coefs(P.build(comps, geo, q, restart=5))
        assert st == 0
        samp = P.GEOS[geo]
        want = [z for mcu in J._mcus([np.asarray(c) for c in comps], samp) for _, z in mcu]
        nat = np.zeros((len(want), 64), np.int64)
        nat[:, J.ZIGZAG] = np.array(want)
        assert np.array_equal(co, nat)
    masks = P.sweep_masks(geo)
    assert sorted(masks[0].reshape(-1).tolist()) == list(range(256))
    for m, z in zip(masks, P.sweep_coefs(geo)):  # the nonzero parts of a block are exactly its mask's
        got = sum(((z.reshape(*m.shape, 8, 8) != 0).any(axis=3)[:, :, p].astype(int) << p) for p in range(8))
        assert np.array_equal(got, m)


def test_eob_sweep_positions():
    z = P.eob_coefs()[0].reshape(64, 64)
    for k in range(64):
        assert int(np.flatnonzero(z[k]).max()) == k
        if k >= 18:
            assert not z[k, 2:k].any()


@pytest.mark.parametrize("sem", [0, 1], ids=["libjpeg", "zune"])
@pytest.mark.parametrize("geo", list(P.GEOS))
def test_every_stored_part_of_mask_sweep_matters(geo, sem):
    base = _decode(P.build(P.sweep_coefs(geo), geo, P.Q_SWEEP), sem).astype(int)
    masks = P.sweep_masks(geo)
    insensitive = 0
    for p in range(8):
        for ci in range(len(masks)):
            comps = P.sweep_coefs(geo)
            comps[ci] = P.sweep_coefs(geo, drop_part=p)[ci]
            diff = (_decode(P.build(comps, geo, P.Q_SWEEP), sem).astype(int) != base).any(axis=2)
            s = 8 if ci == 0 else 16  # pixels a block of this component covers
            changed = diff.reshape(P.H // s, s, P.W // s, s).any(axis=(1, 3))
            has = ((masks[ci] >> p) & 1).astype(bool)
            insensitive += int((has & ~changed).sum())
            if ci == 0:  # (chroma upsampling may spread a chroma block into its neighbours' pixels)
                assert not (changed & ~has).any()
    assert insensitive == 0
