"""Four-component Adobe JPEGs (APP14 transform 0 = CMYK, 2 = YCCK) behind
context option "jpeg_cmyk": bit-exact in both decode semantics against
tests/ref_jpeg_cmyk.py (its planes pinned against Pillow in
test_jpeg_cmyk_cpu.py; the oracle refuses these files) and, in libjpeg mode,
against the blinn rule over Pillow's own planes.  Covers the entropy passes'
four-component instantiations (restart intervals, workgroup borders, split
ranges), k_cmyk, the resize passes over its RGB image, the kernel options that
stand down for these files, the progressive path and the other outputs."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_craft as J
import ref_jpeg_cmyk as R
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEMS = [0, 1]
SEM_IDS = ["libjpeg", "zune"]
CFG = (224, 16, 0.5, 2.0)
SIZES = [(1, 1), (2, 33), (3, 5), (5, 2), (9, 17), (37, 29), (131, 67)]
RESTARTS = [0, 1, 3]
OLD_WHY = "CMYK/2-component JPEG"
# every layout in the transform its name says, and the other one where the layout is as plausible
LAYOUT_T = [("cmyk_444", 0), ("cmyk_444", 2), ("ycck_420", 2), ("ycck_420", 0), ("ycck_422", 2), ("k_sub", 0),
            ("k_sub", 2), ("ycck_440", 2)]


def _lib():
    from datago_amd import _lib as L
    return L


class Case:
    """A crafted file with its coefficients; reference pixels per semantics, computed once."""

    def __init__(self, name, t, w, h, seed, quality=75, restart=0, tables="std", progressive=False):
        self.label = "%s t%d %dx%d r%d%s" % (name, t, w, h, restart, " prog" if progressive else "")
        self.samp, self.t, self.w, self.h = R.CMYK_LAYOUTS[name], t, w, h
        self.comps, self.qtabs, self.tq = R.craft(self.samp, w, h, t, seed=seed, quality=quality)
        if progressive:
            self.data = R.progressive(self.comps, self.samp, w, h, self.qtabs, self.tq, t)
            self.comps = R.visible_coefs(self.comps, self.samp, w, h)
        else:
            self.data = R.baseline(self.comps, self.samp, w, h, self.qtabs, self.tq, t, restart=restart, tables=tables)
        self._ref = {}

    def ref(self, sem):
        if sem not in self._ref:
            self._ref[sem] = R.decode(self.comps, self.samp, self.w, self.h, self.qtabs, self.tq, self.t, sem)
        return self._ref[sem]


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (resize, decode semantics, jpeg_cmyk), made once per module."""
    cache = {}

    def get(resize, sem, cmyk=True, **extra):
        key = (resize, sem, cmyk, tuple(sorted(extra.items())))
        if key not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if resize else {}
            cache[key] = _lib().Context(0, decode_semantics=sem, **kw, **extra)
            if cmyk:
                cache[key].set_option("jpeg_cmyk", 1)
                cache[key].set_option("jpeg_h1v2", 1)  # for ycck_440
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


def _pil_rgb(data):
    """The blinn rule over Pillow's planes (255 - its CMYK image: the stored convention)."""
    im = Image.open(io.BytesIO(data))
    assert im.mode == "CMYK"
    return R.rgb_of_planes(255 - np.asarray(im))


def _same(arr, ref, label):
    assert arr.shape[:2] == ref.shape[:2], label
    got = arr.reshape(ref.shape)
    assert np.array_equal(got, ref), (label, int((got != ref).sum()))


def test_option_off_refuses_with_the_old_text(ctxs):
    L = _lib()
    ctx = ctxs(False, 0, cmyk=False)
    cases = [Case(name, t, 37, 29, seed=3) for name, t in LAYOUT_T] + [Case("ycck_420", 2, 9, 17, seed=4, progressive=True)]
    for c, (st, arr, _) in zip(cases, ctx.decode_batch([c.data for c in cases])):
        assert st == L.DG_ERR_UNSUPPORTED and arr is None, c.label
        assert ctx.output_size(c.data)[0] == L.DG_ERR_UNSUPPORTED, c.label
        assert OLD_WHY in L.last_error(), (c.label, L.last_error())
        st, info = L.probe(c.data)  # dg_probe describes the default options
        assert info.gpu_supported == 0, c.label


def test_option_values():
    L = _lib()
    ctx = L.Context(0)
    data = Case("cmyk_444", 0, 37, 29, seed=3).data
    ctx.set_option("jpeg_cmyk", 1)
    assert ctx.output_size(data) == (L.DG_OK, 37 * 29 * 3)
    ctx.set_option("jpeg_cmyk", 0)
    assert ctx.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("jpeg_cmyk", bad)
        assert e.value.status == L.DG_ERR_INVALID and "jpeg_cmyk" in L.last_error()
    ctx.close()


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_refusals_with_the_option_on(ctxs, sem):
    L = _lib()
    good = Case("cmyk_444", 0, 37, 29, seed=3)
    adobe = good.data.index(b"Adobe")
    samp = good.samp
    refused = [
        (good.data[:adobe - 3] + b"\xfe" + good.data[adobe - 2:], "without an Adobe segment"),  # APP14 -> COM
        (good.data[:adobe + 11] + b"\x01" + good.data[adobe + 12:], "transform 1"),
        (R.baseline(good.comps, samp, 37, 29, good.qtabs, good.tq, 0, td=[0, 1, 2, 3], ta=[0, 1, 2, 3]),
         "more distinct Huffman tables"),
    ]
    six = R.baseline(good.comps, samp, 37, 29, good.qtabs, good.tq, 0, td=[0, 1, 2, 0], ta=[0, 1, 2, 1])
    ctx = ctxs(False, sem)
    files = [good.data] + [d for d, _ in refused] + [six, synth.make_jpeg(5, 64, 48, 85, "4:2:0")]
    res = ctx.decode_batch(files)
    for (d, text), (st, arr, _) in zip(refused, res[1:4]):
        assert st == L.DG_ERR_UNSUPPORTED and arr is None, text
        assert ctx.output_size(d)[0] == L.DG_ERR_UNSUPPORTED
        assert text in L.last_error() and OLD_WHY not in L.last_error(), (text, L.last_error())
    for k in (0, 4):  # the others of the batch are unaffected; six tables are inside the budget
        assert res[k][0] == 0
        _same(res[k][1], good.ref(sem), "beside refusals %d" % k)
    plain = ctxs(False, sem, cmyk=False).decode_batch([files[5]])[0]
    assert res[5][0] == 0 and np.array_equal(res[5][1], plain[1])


@pytest.fixture(scope="module")
def decode_cases():
    return [Case(name, t, w, h, seed=w + rst, quality=(50, 90, 100)[rst % 3], restart=rst,
                 tables="optimal" if rst == 1 else "std")
            for name, t in LAYOUT_T for w, h in SIZES for rst in RESTARTS]


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
    plain = ctxs(False, sem, cmyk=False).decode_batch([ordinary[k] for k in sorted(ordinary)])
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
        assert (meta.channels, meta.bit_depth) == (3, 8), c.label
        _same(arr, c.ref(sem), c.label)
        if sem == 0:
            assert np.array_equal(arr, _pil_rgb(c.data)), c.label
    assert ctx.stat("write_mismatch") == 0


@pytest.fixture(scope="module")
def border_cases():
    """Coded data past one workgroup's 256 subsequences of 2,048 bits (64 KiB): the workgroup-border fix and
    write_split's half ranges see component 3."""
    out = [Case("cmyk_444", 0, 900, 640, seed=50, quality=90, restart=rst) for rst in (0, 50)]
    for c in out:
        assert len(c.data) > 2 * 65536, len(c.data)
    return out


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_entropy_boundaries(ctxs, border_cases, sem):
    ctx = ctxs(False, sem)
    for c, (st, arr, _) in zip(border_cases, ctx.decode_batch([c.data for c in border_cases])):
        assert st == 0, (c.label, st, _lib().last_error())
        _same(arr, c.ref(sem), c.label)
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
def resize_cases(border_cases):
    out = []
    for name, t in (("cmyk_444", 0), ("ycck_420", 2)):
        sizes = [(150, 110), (420, 300), (900, 640), _bucket_sized_source(), (300, 420)]
        for k, (w, h) in enumerate(sizes):
            if (name, w) == ("cmyk_444", 900):
                out.append(border_cases[0])  # the same file: its reference is computed once
            else:
                out.append(Case(name, t, w, h, seed=20 + k, quality=60 if w * h > 200000 else 85, restart=(0, 7, 0, 3, 0)[k]))
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
        assert (meta.width, meta.height, meta.channels, meta.bit_depth) == (tw, th, 3, 8), c.label
        _same(arr, ref, c.label)
    assert ctx.stat("write_mismatch") == 0


@pytest.fixture(scope="module")
def sweep_cases():
    return [Case("ycck_420", 2, 131, 67, seed=31, quality=90, restart=3), Case("cmyk_444", 0, 420, 300, seed=32, quality=85)]


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
@pytest.mark.parametrize("option,value,default", [("write_split", 0, 1), ("idct_thread", 0, 1), ("sparse_coef", 0, 1),
                                                  ("multi_lead", 0, 1), ("v_tile", 0, 4), ("h_planar", 0, 1),
                                                  ("sync2", 1, 0), ("entropy_once", 1, 0), ("idct_fused", 1, 0),
                                                  ("band_dec", 1, 0), ("h_mfma", 1, 0), ("hv_fused", 1, 0)])
def test_options_leave_cmyk_exact(ctxs, sweep_cases, option, value, default, sem):
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


def _pillow_cmyk_file(w, h, seed, progressive):
    rng = np.random.default_rng(seed)
    px = np.concatenate([synth.synth_pixels(rng, w, h), synth.synth_pixels(rng, w, h)[:, :, :1]], axis=2)
    buf = io.BytesIO()
    Image.fromarray(px.astype(np.uint8), "CMYK").save(buf, "JPEG", quality=90, progressive=progressive)
    return buf.getvalue()


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_progressive(ctxs, sem):
    small = Case("ycck_420", 2, 9, 17, seed=9, quality=90, progressive=True)
    big = Case("ycck_420", 2, 131, 67, seed=10, progressive=True)
    other = Case("cmyk_444", 0, 37, 29, seed=11, progressive=True)
    cases = (small, big, other)
    for c, (st, arr, _) in zip(cases, ctxs(False, sem).decode_batch([c.data for c in cases])):
        assert st == 0, (c.label, st, _lib().last_error())
        _same(arr, c.ref(sem), c.label)
    st, arr, meta = ctxs(True, sem).decode_batch([big.data])[0]
    assert st == 0
    (tw, th), ref = _resized_ref(big, sem)
    assert (meta.width, meta.height) == (tw, th)
    _same(arr, ref, big.label + " resized")


def test_pillow_written_files(ctxs):
    """A foreign encoder's CMYK files (transform 0, all 1x1), baseline and progressive, in libjpeg mode."""
    files = [_pillow_cmyk_file(67, 45, 5, False), _pillow_cmyk_file(67, 45, 6, True)]
    for d, (st, arr, m) in zip(files, ctxs(False, 0).decode_batch(files)):
        assert st == 0, _lib().last_error()
        assert (m.width, m.height, m.channels, m.bit_depth) == (67, 45, 3, 8)
        assert np.array_equal(arr.reshape(45, 67, 3), _pil_rgb(d))


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_other_outputs(ctxs, sem):
    L = _lib()
    cases = [Case("ycck_420", 2, 131, 67, seed=41, quality=90), Case("k_sub", 0, 37, 29, seed=42, restart=3)]
    datas = [c.data for c in cases]
    # image_to_rgb8: these files are RGB already
    for c, (st, arr, m) in zip(cases, ctxs(False, sem, image_to_rgb8=True).decode_batch(datas)):
        assert st == 0 and (m.channels, m.bit_depth) == (3, 8), c.label
        _same(arr, c.ref(sem), c.label)
    # the JPEG re-encoder takes the decoded pixels
    enc = ctxs(False, sem, pre_encode_images=True, encode_format=1, jpeg_quality=92)
    for c, (st, buf, m) in zip(cases, enc.decode_batch(datas)):
        assert st == 0 and m.is_encoded == 1, c.label
        assert buf.tobytes() == O.jpeg_encode(c.ref(sem), 92), c.label
    # the PNG re-encoder round-trips to them
    penc = ctxs(False, sem, pre_encode_images=True, encode_format=0)
    for c, (st, buf, m) in zip(cases, penc.decode_batch(datas)):
        assert st == 0 and m.is_encoded == 1, c.label
        back = np.asarray(Image.open(io.BytesIO(buf.tobytes())))
        assert back.shape == (c.h, c.w, 3) and np.array_equal(back, c.ref(sem)), c.label
    # dg_decode_one
    st, arr, m = ctxs(False, sem).decode_one(datas[0])
    assert st == L.DG_OK and (m.width, m.height) == (131, 67)
    _same(arr, cases[0].ref(sem), cases[0].label)
