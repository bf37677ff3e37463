"""Sampling layouts the header accepts but PIL never writes (tests/jpeg_craft.py
LAYOUTS: 4:4:4 as (2,1)x3, 4:2:2 as (4,1),(2,1),(2,1), one chroma plane at
half rate and the other not, subsampled luma, Adobe RGB, gray with factors),
bit-exact against the oracle in both decode semantics and, in libjpeg mode,
against PIL (test_oracle_jpeg_layouts.py pins the oracle to it): the general
block index of k_idct_t, chroma records on one plane only, a record plane for
luma, the generic colour path of k_color and of the fused band kernels."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_craft as J
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEMS = [0, 1]
SEM_IDS = ["libjpeg", "zune"]
CFG = (224, 16, 0.5, 2.0)
RESIZE_LAYOUTS = [n for n in J.OK_LAYOUTS if len(J.LAYOUTS[n][0]) == 3] + ["gray_22"]
BIG_LAYOUTS = ["444_h2", "mixed_cb_full"]


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (resize, decode semantics), made once per module."""
    cache = {}

    def get(resize, sem):
        if (resize, sem) not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if resize else {}
            cache[(resize, sem)] = _lib().Context(0, decode_semantics=sem, **kw)
        return cache[(resize, sem)]
    yield get
    for c in cache.values():
        c.close()


def _oracle_decoded(data, sem):
    with O.semantics(sem):
        st, dec = O.jpeg_decode(data)
    assert st == 0
    return dec


def _oracle_resized(data, tw, th, sem=0):
    return O.crop_and_resize(_oracle_decoded(data, sem), tw, th, O.MODE_FIR)


def _pil(data):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im.convert("RGB")) if im.mode != "L" else np.asarray(im)[:, :, None]


@pytest.fixture(scope="module")
def decode_files():
    """[(label, expected status, bytes)]: every layout at three sizes and
    three restart intervals, and two ordinary PIL 4:2:0 files among them."""
    out = []
    for name, (_, _, want) in J.LAYOUTS.items():
        for w, h in ((3, 5), (37, 29), (131, 67)):
            for rst in (0, 1, 3):
                out.append(("%s %dx%d r%d" % (name, w, h, rst), want,
                            J.layout_jpeg(name, w, h, seed=w + rst, quality=(50, 90, 100)[rst % 3], restart=rst,
                                          tables="optimal" if rst == 1 else "std")))
    out.insert(40, ("pil420 a", 0, synth.make_jpeg(5, 203, 117, 85, "4:2:0")))
    out.insert(120, ("pil420 b", 0, synth.make_jpeg(6, 64, 48, 92, "4:2:0", restart_marker_rows=1)))
    return out


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_decode_only_every_layout_in_one_batch(ctxs, decode_files, sem):
    ctx = ctxs(False, sem)
    res = ctx.decode_batch([d for _, _, d in decode_files])
    for (label, want, data), (st, arr, meta) in zip(decode_files, res):
        assert st == want, (label, st)
        if want != J.OK:
            assert arr is None
            continue
        ref = _oracle_decoded(data, sem)
        assert arr.shape == ref.shape, label
        assert np.array_equal(arr, ref), (label, int((arr != ref).sum()))
        if sem == 0:
            assert np.array_equal(arr, _pil(data)), label
    assert ctx.stat("write_mismatch") == 0


def _bucket_sized_source():
    """A source size that is its own bucket (the copy path: no resize pass)."""
    t = B.ARAwareTransform(*CFG)
    for _, key in t.aspect_ratios:
        w, h = t.aspect_ratio_to_size[key]
        if w != h and t.target_size(w, h) == (w, h):
            return w, h
    raise AssertionError("no bucket maps to itself")


@pytest.fixture(scope="module")
def resize_files():
    """[(label, bytes)]: an upscale (8-tap class), the 16- and 32-tap
    classes; for two layouts also the any-tap kernel and the copy path."""
    out = []
    for name in RESIZE_LAYOUTS:
        sizes = [(150, 110), (420, 300), (900, 640)]
        if name in BIG_LAYOUTS:
            sizes += [(1500, 1000), _bucket_sized_source()]
        for k, (w, h) in enumerate(sizes):
            out.append(("%s %dx%d" % (name, w, h),
                        J.layout_jpeg(name, w, h, seed=20 + k, quality=60 if w * h > 200000 else 85,
                                      restart=(0, 7, 0, 50, 3)[k])))
    return out


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_crop_resize_every_layout(ctxs, resize_files, sem):
    ctx = ctxs(True, sem)
    t = B.ARAwareTransform(*CFG)
    res = ctx.decode_batch([d for _, d in resize_files])
    for (label, data), (st, arr, meta) in zip(resize_files, res):
        assert st == 0, (label, st)
        w, h = O.jpeg_info(data)[1:3]
        tw, th = t.target_size(w, h)
        assert (meta.width, meta.height) == (tw, th), label
        ref = _oracle_resized(data, tw, th, sem)
        assert arr.shape[:2] == ref.shape[:2], label
        assert np.array_equal(arr.reshape(ref.shape), ref), (label, int((arr.reshape(ref.shape) != ref).sum()))
    assert ctx.stat("write_mismatch") == 0


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
@pytest.mark.parametrize("option,value,default,resize", [("chroma_rec", 0, 1, False), ("h_planar", 0, 1, True),
                                                         ("idct_thread", 0, 1, False), ("sub_bits", 64, 0, False)])
def test_options_leave_layouts_exact(ctxs, option, value, default, resize, sem):
    datas = [J.layout_jpeg(n, 131, 67, seed=31, quality=90, restart=r)
             for n in ("mixed_cb_full", "422_wide") for r in (0, 3)]
    ctx = ctxs(resize, sem)
    base = ctx.decode_batch(datas)
    ctx.set_option(option, value)
    try:
        res = ctx.decode_batch(datas)
    finally:
        ctx.set_option(option, default)
    t = B.ARAwareTransform(*CFG)
    for d, (st0, a0, _), (st, arr, _) in zip(datas, base, res):
        assert st0 == 0 and st == 0
        ref = _oracle_resized(d, *t.target_size(131, 67), sem) if resize else _oracle_decoded(d, sem)
        assert np.array_equal(arr.reshape(ref.shape), ref)
        assert np.array_equal(a0, arr)
