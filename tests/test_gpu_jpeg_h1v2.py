"""Colour JPEGs with a component at the full horizontal and half the vertical
rate (4:4:0 and four mixed layouts) behind context option "jpeg_h1v2":
bit-exact in both decode semantics against tests/ref_jpeg_h1v2.py (pinned
against Pillow in test_jpeg_h1v2_cpu.py; the oracle refuses these files) and,
decode-only in libjpeg mode, against Pillow itself.  Covers the generic
upsampling (k_color, the generic band fill, k_resize_hv, k_resize_hm), the
4:4:0 fill classes of k_resize_hb / k_resize_hbp in every tap class, the
progressive path and the other outputs."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_craft as J
import ref_jpeg_h1v2 as R
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEMS = [0, 1]
SEM_IDS = ["libjpeg", "zune"]
CFG = (224, 16, 0.5, 2.0)
SIZES = [(1, 1), (2, 33), (3, 5), (5, 2), (9, 17), (37, 29), (131, 67)]
RESTARTS = [0, 1, 3]
OLD_WHY = "chroma sampling other than 4:4:4/4:2:2/4:2:0"


def _lib():
    from datago_amd import _lib as L
    return L


class Case:
    """A crafted file with its coefficients; reference pixels per semantics, computed once."""

    def __init__(self, name, w, h, seed, quality=75, restart=0, tables="std", progressive=False):
        self.label = "%s %dx%d r%d%s" % (name, w, h, restart, " prog" if progressive else "")
        self.samp, self.w, self.h = R.H1V2_LAYOUTS[name], w, h
        self.comps, self.qtabs, self.tq = R.craft(self.samp, w, h, seed=seed, quality=quality)
        if progressive:
            self.data = R.progressive(self.comps, self.samp, w, h, self.qtabs, self.tq)
            self.comps = R.visible_coefs(self.comps, self.samp, w, h)
        else:
            self.data = R.baseline(self.comps, self.samp, w, h, self.qtabs, self.tq, restart=restart, tables=tables)
        self._ref = {}

    def ref(self, sem):
        if sem not in self._ref:
            self._ref[sem] = R.decode(self.comps, self.samp, self.w, self.h, self.qtabs, self.tq, sem)
        return self._ref[sem]


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (resize, decode semantics, jpeg_h1v2), made once per module."""
    cache = {}

    def get(resize, sem, h1v2=True, **extra):
        key = (resize, sem, h1v2, tuple(sorted(extra.items())))
        if key not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if resize else {}
            cache[key] = _lib().Context(0, decode_semantics=sem, **kw, **extra)
            if h1v2:
                cache[key].set_option("jpeg_h1v2", 1)
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


def _pil(data):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im.convert("RGB")) if im.mode != "L" else np.asarray(im)[:, :, None]


def _same(arr, ref, label):
    assert arr.shape[:2] == ref.shape[:2], label
    got = arr.reshape(ref.shape)
    assert np.array_equal(got, ref), (label, int((got != ref).sum()))


def test_option_off_refuses_with_the_old_text(ctxs):
    L = _lib()
    ctx = ctxs(False, 0, h1v2=False)
    cases = [Case(name, 37, 29, seed=3) for name in R.H1V2_LAYOUTS] + [Case("440", 9, 17, seed=4, progressive=True)]
    for c, (st, arr, _) in zip(cases, ctx.decode_batch([c.data for c in cases])):
        assert st == L.DG_ERR_UNSUPPORTED and arr is None, c.label
        assert ctx.output_size(c.data)[0] == L.DG_ERR_UNSUPPORTED, c.label
        assert OLD_WHY in L.last_error(), (c.label, L.last_error())
        st, info = L.probe(c.data)  # dg_probe describes the default options
        assert info.gpu_supported == 0, c.label


def test_option_values():
    L = _lib()
    ctx = L.Context(0)
    data = Case("440", 37, 29, seed=3).data
    ctx.set_option("jpeg_h1v2", 1)
    assert ctx.output_size(data) == (L.DG_OK, 37 * 29 * 3)
    ctx.set_option("jpeg_h1v2", 0)
    assert ctx.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("jpeg_h1v2", bad)
        assert e.value.status == L.DG_ERR_INVALID and "jpeg_h1v2" in L.last_error()
    ctx.close()


@pytest.fixture(scope="module")
def decode_cases():
    return [Case(name, w, h, seed=w + rst, quality=(50, 90, 100)[rst % 3], restart=rst,
                 tables="optimal" if rst == 1 else "std")
            for name in R.H1V2_LAYOUTS for w, h in SIZES for rst in RESTARTS]


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_decode_only_in_one_batch(ctxs, decode_cases, sem):
    ordinary = {40: synth.make_jpeg(5, 203, 117, 85, "4:2:0"),
                80: synth.make_jpeg(6, 64, 48, 92, "4:2:0", restart_marker_rows=1),
                100: synth.make_jpeg(7, 70, 53, 90, gray=True)}
    files = [c.data for c in decode_cases]
    for k in sorted(ordinary):
        files.insert(k, ordinary[k])
    ctx = ctxs(False, sem)
    res = ctx.decode_batch(files)
    plain = ctxs(False, sem, h1v2=False).decode_batch([ordinary[k] for k in sorted(ordinary)])
    for k, (st0, a0, _) in zip(sorted(ordinary), plain):
        assert st0 == 0 and res[k][0] == 0
        assert np.array_equal(res[k][1], a0)
    cases = iter(decode_cases)
    for k, (st, arr, meta) in enumerate(res):
        if k in ordinary:
            continue
        c = next(cases)
        assert st == 0, (c.label, st, _lib().last_error())
        assert arr.shape == (c.h, c.w, 3), c.label
        _same(arr, c.ref(sem), c.label)
        if sem == 0:
            assert np.array_equal(arr, _pil(c.data)), c.label
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
def resize_cases():
    """An upscale (8-tap class), the 16- and 32-tap classes, the any-tap kernel
    and the copy path, for 4:4:0 (the fill classes) and a mixed layout (the
    generic fill); a portrait 4:4:0, the shape a rotated camera file has."""
    out = []
    for name in ("440", "420_cb_h2v1"):
        sizes = [(150, 110), (420, 300), (900, 640), (1500, 1000), _bucket_sized_source()]
        for k, (w, h) in enumerate(sizes):
            out.append(Case(name, w, h, seed=20 + k, quality=60 if w * h > 200000 else 85, restart=(0, 7, 0, 50, 3)[k]))
    out.append(Case("440", 300, 420, seed=30, quality=85))
    return out


def _resized_ref(c, sem):
    tw, th = B.ARAwareTransform(*CFG).target_size(c.w, c.h)
    return (tw, th), O.crop_and_resize(c.ref(sem), tw, th, O.MODE_FIR)


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_crop_and_resize(ctxs, resize_cases, sem):
    ctx = ctxs(True, sem)
    res = ctx.decode_batch([c.data for c in resize_cases])
    for c, (st, arr, meta) in zip(resize_cases, res):
        assert st == 0, (c.label, st, _lib().last_error())
        (tw, th), ref = _resized_ref(c, sem)
        assert (meta.width, meta.height) == (tw, th), c.label
        _same(arr, ref, c.label)
    assert ctx.stat("write_mismatch") == 0


@pytest.fixture(scope="module")
def sweep_cases():
    return [Case("440", 131, 67, seed=31, quality=90, restart=3), Case("440", 420, 300, seed=32, quality=85)]


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
@pytest.mark.parametrize("option,value,default", [("h_planar", 0, 1), ("h_prefetch", 0, 1), ("idct_thread", 0, 1),
                                                  ("v_tile", 0, 4), ("band_dec", 1, 0), ("h_mfma", 1, 0),
                                                  ("hv_fused", 1, 0), ("idct_fused", 1, 0)])
def test_options_leave_440_exact(ctxs, sweep_cases, option, value, default, sem):
    ctx = ctxs(True, sem)
    datas = [c.data for c in sweep_cases]
    base = ctx.decode_batch(datas)
    ctx.set_option(option, value)
    try:
        res = ctx.decode_batch(datas)
    finally:
        ctx.set_option(option, default)
    for c, (st0, a0, _), (st, arr, _) in zip(sweep_cases, base, res):
        assert st0 == 0 and st == 0, (c.label, st0, st)
        _same(arr, _resized_ref(c, sem)[1], c.label)
        assert np.array_equal(a0, arr), c.label


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_progressive(ctxs, sem):
    small, big = Case("440", 9, 17, seed=9, quality=90, progressive=True), Case("440", 131, 67, seed=10, progressive=True)
    for c, (st, arr, _) in zip((small, big), ctxs(False, sem).decode_batch([small.data, big.data])):
        assert st == 0, (c.label, st, _lib().last_error())
        _same(arr, c.ref(sem), c.label)
    st, arr, meta = ctxs(True, sem).decode_batch([big.data])[0]
    assert st == 0
    (tw, th), ref = _resized_ref(big, sem)
    assert (meta.width, meta.height) == (tw, th)
    _same(arr, ref, big.label + " resized")


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_other_outputs(ctxs, sem):
    L = _lib()
    cases = [Case("440", 131, 67, seed=41, quality=90), Case("luma_sub_v2", 37, 29, seed=42, restart=3)]
    datas = [c.data for c in cases]
    # image_to_rgb8: these layouts are RGB already
    for c, (st, arr, m) in zip(cases, ctxs(False, sem, image_to_rgb8=True).decode_batch(datas)):
        assert st == 0 and (m.channels, m.bit_depth) == (3, 8), c.label
        _same(arr, c.ref(sem), c.label)
    # the JPEG re-encoder takes the decoded pixels
    enc = ctxs(False, sem, pre_encode_images=True, encode_format=1, jpeg_quality=92)
    for c, (st, buf, m) in zip(cases, enc.decode_batch(datas)):
        assert st == 0 and m.is_encoded == 1, c.label
        assert buf.tobytes() == O.jpeg_encode(c.ref(sem), 92), c.label
    # dg_decode_one
    st, arr, m = ctxs(False, sem).decode_one(datas[0])
    assert st == L.DG_OK and (m.width, m.height) == (131, 67)
    _same(arr, cases[0].ref(sem), cases[0].label)
