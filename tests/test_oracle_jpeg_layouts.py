"""Sampling layouts the header accepts beyond PIL's three (tests/jpeg_craft.py
LAYOUTS): the oracle in libjpeg mode is pinned bit for bit against PIL
(libjpeg-turbo) on every accepted one, so the GPU tests of these layouts
(test_gpu_layouts.py) have a reference independent of this project; and
dg_probe reports each layout as the header parser classifies it."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_craft as J
from oracle import oracle as O

SIZES = [(3, 5), (37, 29), (131, 67)]
RESTARTS = [0, 1, 3]


def pil_decode(data, ncomp):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im.convert("RGB")) if ncomp == 3 else np.asarray(im.convert("L"))[:, :, None]


@pytest.mark.parametrize("rst", RESTARTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", J.OK_LAYOUTS)
def test_oracle_equals_pil(name, size, rst):
    data = J.layout_jpeg(name, *size, seed=size[0] + rst, restart=rst, tables="optimal" if rst == 3 else "std")
    st, dec = O.jpeg_decode(data)
    assert st == O.OJ_OK
    ref = pil_decode(data, len(J.LAYOUTS[name][0]))
    assert dec.shape == ref.shape
    assert np.array_equal(dec, ref), int((dec != ref).sum())


def test_rgb_component_ids_equal_pil():
    """No APPn marker, component ids 'R', 'G', 'B': untransformed RGB."""
    px = np.random.default_rng(4).integers(0, 256, (29, 37, 3)).astype(np.uint8)
    for samp in ([(1, 1)] * 3, [(2, 1)] * 3):
        data = J.from_pixels(px, samp, 90, header="rgb", restart=2)
        st, dec = O.jpeg_decode(data)
        assert st == O.OJ_OK and np.array_equal(dec, pil_decode(data, 3))


@pytest.mark.parametrize("name", [k for k, v in J.LAYOUTS.items() if v[2] == J.UNSUPPORTED])
def test_oracle_refuses_unsupported_ratio(name):
    for size in SIZES:
        st, dec = O.jpeg_decode(J.layout_jpeg(name, *size))
        assert st == O.OJ_UNSUPPORTED and dec is None


@pytest.fixture(scope="module")
def lib():
    import os
    from datago_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from datago_amd import build
        build.build()
    _lib.load()
    return _lib


@pytest.mark.parametrize("name", list(J.LAYOUTS))
def test_probe_status(lib, name):
    """dg_probe: DG_OK and gpu_supported for the accepted layouts, with the
    frame's size, component count and factors; DG_ERR_CORRUPT for more than
    10 blocks per MCU; a valid file outside the GPU path (the UNSUPPORTED
    rows) is, as dg_probe documents and test_abi_cpu pins for CMYK, DG_OK with
    gpu_supported 0 -- DG_ERR_UNSUPPORTED is then the decode's status
    (test_gpu_layouts.py)."""
    samp, _, want = J.LAYOUTS[name]
    for w, h in SIZES:
        st, info = lib.probe(J.layout_jpeg(name, w, h, restart=3))
        if want == J.CORRUPT:
            assert st == lib.DG_ERR_CORRUPT and info.gpu_supported == 0
            continue
        assert st == lib.DG_OK and info.format == lib.DG_FMT_JPEG
        assert info.gpu_supported == (1 if want == J.OK else 0)
        assert (info.width, info.height, info.components) == (w, h, len(samp))
        assert [(info.h_samp[c], info.v_samp[c]) for c in range(len(samp))] == samp
        assert info.restart_interval == 3 and info.progressive == 0
