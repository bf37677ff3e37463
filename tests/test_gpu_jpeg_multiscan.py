"""Non-interleaved baseline JPEGs (one scan per one or two components) behind
context option "jpeg_multiscan": bit-exact in both decode semantics against the
oracle's decode of the single-scan twin (tests/ref_jpeg_multiscan.py; pinned to
Pillow in test_jpeg_multiscan_cpu.py).  Covers the parser's refusals through
the library, the scan descriptors' entropy passes (restart intervals, per-scan
tables, workgroup borders, split ranges, sparse and dense blocks), k_ms_zero
and k_huff_write's multiscan instantiation, the resize path, the kernel
options that stand down, mixed submissions, a truncated scan and the other
outputs."""
import numpy as np
import pytest

import jpeg_craft as J
import ref_jpeg_cmyk as RC
import ref_jpeg_h1v2 as RH
import ref_jpeg_multiscan as R
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEMS = [0, 1]
SEM_IDS = ["libjpeg", "zune"]
CFG = (224, 16, 0.5, 2.0)
SIZES = [(1, 1), (8, 8), (9, 17), (33, 17), (37, 29), (131, 67)]
RESTARTS = [0, 1, 3]
OLD_WHY = "non-interleaved multi-scan JPEG"


def _lib():
    from datago_amd import _lib as L
    return L


class Case:
    """A crafted multiscan file with its coefficients; reference pixels per semantics, computed once."""

    def __init__(self, name, w, h, script, seed, quality=75, restart=0, samp=None, coefs=None, **kw):
        self.label = "%s %dx%d %s r%s %s" % (name, w, h, script, restart, sorted(kw.items()))
        self.samp, self.w, self.h, self.script = samp or R.LAYOUTS[name], w, h, script
        self.comps, self.qtabs = coefs or R.craft(self.samp, w, h, seed=seed, quality=quality)
        self.data = R.multiscan(self.comps, self.samp, w, h, self.qtabs, script, restart=restart, **kw)
        self._ref = {}

    def twin(self, sem):
        return R.twin(self.comps, self.samp, self.w, self.h, self.qtabs, zeroed=self.script if sem else False)

    def ref(self, sem):
        if sem not in self._ref:
            self._ref[sem] = R.decode(self.comps, self.samp, self.w, self.h, self.qtabs, sem, self.script)
        return self._ref[sem]


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (resize, decode semantics, jpeg_multiscan, options), made once per module."""
    cache = {}

    def get(resize, sem, ms=True, opts=(), **extra):
        key = (resize, sem, ms, tuple(opts), tuple(sorted(extra.items())))
        if key not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if resize else {}
            cache[key] = _lib().Context(0, decode_semantics=sem, **kw, **extra)
            if ms:
                cache[key].set_option("jpeg_multiscan", 1)
            for k, v in opts:
                cache[key].set_option(k, v)
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


def _same(arr, ref, label):
    assert arr is not None and arr.shape[:2] == ref.shape[:2], label
    got = np.asarray(arr).reshape(ref.shape)
    assert np.array_equal(got, ref), (label, int((got != ref).sum()))


def test_option_off_refuses_with_the_old_text(ctxs):
    L = _lib()
    ctx = ctxs(False, 0, ms=False)
    cases = [Case(name, 37, 29, script, seed=3) for name in R.LAYOUTS for script in R.SCRIPTS[::2]]
    for c, (st, arr, _) in zip(cases, ctx.decode_batch([c.data for c in cases])):
        assert st == L.DG_ERR_UNSUPPORTED and arr is None, c.label
        assert ctx.output_size(c.data)[0] == L.DG_ERR_UNSUPPORTED, c.label
        assert OLD_WHY in L.last_error(), (c.label, L.last_error())
        st, info = L.probe(c.data)  # dg_probe describes the default options
        assert st == L.DG_OK and info.gpu_supported == 0 and info.components == 3, c.label
    for data, _, _ in R.refusal_files()[:2] + R.refusal_files()[3:]:  # (the four-component one keeps jpeg_cmyk's text)
        assert ctx.output_size(data)[0] == L.DG_ERR_UNSUPPORTED and OLD_WHY in L.last_error()


def test_option_values():
    L = _lib()
    ctx = L.Context(0)
    data = Case("420", 37, 29, R.SCRIPTS[0], seed=3).data
    ctx.set_option("jpeg_multiscan", 1)
    assert ctx.output_size(data) == (L.DG_OK, 37 * 29 * 3)
    ctx.set_option("jpeg_multiscan", 0)
    assert ctx.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("jpeg_multiscan", bad)
        assert e.value.status == L.DG_ERR_INVALID and "jpeg_multiscan" in L.last_error()
    ctx.close()


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_refusals_with_the_option_on(ctxs, sem):
    L = _lib()
    good = Case("420", 37, 29, [[0], [1, 2]], seed=3, restart=2)
    refused = R.refusal_files()
    ctx = ctxs(False, sem, opts=(("jpeg_cmyk", 1),))
    files = [good.data] + [d for d, _, _ in refused] + [good.data, synth.make_jpeg(5, 64, 48, 85, "4:2:0")]
    res = ctx.decode_batch(files)
    for (d, status, text), (st, arr, _) in zip(refused, res[1:]):
        want = L.DG_ERR_UNSUPPORTED if status == J.UNSUPPORTED else L.DG_ERR_CORRUPT
        assert st == want and arr is None, text
        assert ctx.output_size(d)[0] == want
        assert text.decode() in L.last_error() and OLD_WHY not in L.last_error(), (text, L.last_error())
    for k in (0, len(refused) + 1):  # the others of the batch are unaffected
        assert res[k][0] == 0
        _same(res[k][1], good.ref(sem), "beside refusals %d" % k)
    plain = ctxs(False, sem, ms=False).decode_batch([files[-1]])[0]
    assert res[-1][0] == 0 and np.array_equal(res[-1][1], plain[1])


@pytest.fixture(scope="module")
def decode_cases():
    """Six layouts x six sizes x four scripts x three restart intervals, with Annex K tables sent once and with
    every scan's own optimal tables under one id; 4:4:0 (option "jpeg_h1v2") once."""
    out = []
    for name in R.LAYOUTS:
        for w, h in SIZES:
            for rst in RESTARTS:
                coefs = R.craft(R.LAYOUTS[name], w, h, seed=w + rst, quality=(50, 90, 100)[rst % 3])
                for script in R.SCRIPTS:
                    out.append(Case(name, w, h, script, 0, restart=rst, coefs=coefs))
                    out.append(Case(name, w, h, script, 0, restart=rst, coefs=coefs, tables="optimal", per_scan_dht=True))
    out.append(Case("440", 37, 29, R.SCRIPTS[1], seed=7, restart=[0, 2, 5], samp=RH.H1V2_LAYOUTS["440"],
                    tables="optimal", per_scan_dht=True))
    return out


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_decode_only_in_one_batch(ctxs, decode_cases, sem):
    ordinary = {40: synth.make_jpeg(5, 203, 117, 85, "4:2:0"),
                80: synth.make_jpeg(6, 64, 48, 92, "4:2:0", restart_marker_rows=1),
                100: synth.make_jpeg(7, 70, 53, 90, gray=True)}
    files = [c.data for c in decode_cases]
    for k in sorted(ordinary):
        files.insert(k, ordinary[k])
    ctx = ctxs(False, sem, opts=(("jpeg_h1v2", 1),))
    res = ctx.decode_batch(files)
    plain = ctxs(False, sem, ms=False).decode_batch([ordinary[k] for k in sorted(ordinary)])
    for k, (st0, a0, _) in zip(sorted(ordinary), plain):
        assert st0 == 0 and res[k][0] == 0
        assert np.array_equal(res[k][1], a0)
    cases = iter(decode_cases)
    refs = {}
    for k, (st, arr, meta) in enumerate(res):
        if k in ordinary:
            continue
        c = next(cases)
        assert st == 0, (c.label, st, _lib().last_error())
        assert arr.shape == (c.h, c.w, 3), c.label
        assert (meta.channels, meta.bit_depth) == (3, 8), c.label
        # cases of one (coefficients, script) share their reference: the tables and restart markers do not reach it
        key = (id(c.comps), str(c.script) if sem else "")
        if key not in refs:
            refs[key] = c.ref(sem)
        _same(arr, refs[key], c.label)
    assert ctx.stat("write_mismatch") == 0


@pytest.fixture(scope="module")
def border_case():
    """A luma scan longer than one workgroup's 256 ranges at 1,024 bits per range (option "sub_bits": the file
    stays small), so that the workgroup-border fix and write_split's half ranges run inside one scan."""
    c = Case("420", 400, 304, [[0], [1, 2]], seed=50, quality=95)
    _, parts = R.multiscan(c.comps, c.samp, c.w, c.h, c.qtabs, c.script, parts=True)
    c.luma_ranges = -(-(parts[0][1] - parts[0][0]) * 8 // 1024)
    return c


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
@pytest.mark.parametrize("sparse", [1, 0], ids=["sparse", "dense"])
@pytest.mark.parametrize("split", [1, 0], ids=["split", "whole"])
def test_workgroup_borders_and_split_ranges(ctxs, border_case, split, sparse, sem):
    c = border_case
    assert c.luma_ranges > 256, c.luma_ranges  # kSubPerWg
    ctx = ctxs(False, sem, opts=(("sub_bits", 1024),))
    ctx.set_option("write_split", split)
    ctx.set_option("sparse_coef", sparse)
    try:
        st, arr, _ = ctx.decode_batch([c.data])[0]
    finally:
        ctx.set_option("write_split", 1)
        ctx.set_option("sparse_coef", 1)
    assert st == 0, (st, _lib().last_error())
    assert ctx.stat("sub_bits") == 1024
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
def resize_cases():
    """An upscale (8-tap class), the 16- and 32-tap classes, the copy path and a portrait source, as the CMYK
    tests cover them."""
    out = []
    for name, script in (("444", R.SCRIPTS[0]), ("420", R.SCRIPTS[2]), ("422", R.SCRIPTS[3]), ("mixed_12", R.SCRIPTS[1])):
        sizes = [(150, 110), (420, 300), (900, 640), _bucket_sized_source(), (300, 420)]
        for k, (w, h) in enumerate(sizes):
            if w == 900 and name not in ("444", "420"):
                continue
            out.append(Case(name, w, h, script, seed=20 + k, quality=60 if w * h > 200000 else 85,
                            restart=(0, 7, 0, 3, 0)[k]))
    return out


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_crop_and_resize_equals_the_twin(ctxs, resize_cases, sem):
    """Nothing after the coefficients differs: the same context's output for the single-scan twin."""
    ctx = ctxs(True, sem)
    res = ctx.decode_batch([c.data for c in resize_cases])
    twins = ctx.decode_batch([c.twin(sem) for c in resize_cases])
    t = B.ARAwareTransform(*CFG)
    for c, (st, arr, meta), (st2, arr2, meta2) in zip(resize_cases, res, twins):
        assert st == 0 and st2 == 0, (c.label, st, st2, _lib().last_error())
        assert (meta.width, meta.height, meta.channels, meta.bit_depth) == t.target_size(c.w, c.h) + (3, 8), c.label
        assert np.array_equal(arr, arr2), (c.label, int((arr != arr2).sum()))
    assert ctx.stat("write_mismatch") == 0


@pytest.fixture(scope="module")
def sweep_cases():
    return [Case("420", 131, 67, R.SCRIPTS[0], seed=31, quality=90, restart=3),
            Case("422", 420, 300, R.SCRIPTS[2], seed=32, quality=85, tables="optimal", per_scan_dht=True)]


def _resized_ref(c, sem):
    tw, th = B.ARAwareTransform(*CFG).target_size(c.w, c.h)
    return O.crop_and_resize(c.ref(sem), tw, th, O.MODE_FIR)


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
@pytest.mark.parametrize("option,value,default", [("idct_fused", 1, 0), ("entropy_once", 1, 0), ("sync2", 1, 0),
                                                  ("band_dec", 1, 0), ("hv_fused", 1, 0), ("sparse_coef", 0, 1),
                                                  ("idct_thread", 0, 1)])
def test_options_leave_multiscan_exact(ctxs, sweep_cases, option, value, default, sem):
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
        _same(arr, _resized_ref(c, sem), c.label)
        assert np.array_equal(a0, arr), c.label


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_mixed_submission(ctxs, sem):
    """Multiscan, ordinary baseline, progressive, PNG and (option "jpeg_cmyk") four-component members together:
    the batch runs k_huff_write<4, true>."""
    import io

    from PIL import Image
    ms = [Case("420", 131, 67, R.SCRIPTS[0], seed=61, restart=5), Case("luma_sub_420", 37, 29, R.SCRIPTS[3], seed=62),
          Case("444", 33, 17, R.SCRIPTS[1], seed=63, tables="optimal", per_scan_dht=True)]
    buf = io.BytesIO()
    Image.fromarray(synth.synth_pixels(np.random.default_rng(64), 120, 90).astype(np.uint8)).save(
        buf, "JPEG", quality=85, progressive=True)
    others = [synth.make_jpeg(65, 203, 117, 85, "4:2:0"), buf.getvalue(), synth.make_png(66, 77, 55, "RGB"),
              synth.make_jpeg(67, 64, 48, 92, "4:2:2", restart_marker_rows=1), synth.make_jpeg(68, 70, 53, 90, gray=True)]
    files = [ms[0].data, others[0], others[1], ms[1].data, others[2], others[3], ms[2].data, others[4]]
    where_ms, where_other = [0, 3, 6], [1, 2, 4, 5, 7]
    cm_samp = RC.CMYK_LAYOUTS["ycck_420"]
    cm_comps, cm_q, cm_tq = RC.craft(cm_samp, 37, 29, 2, seed=69)
    files.append(RC.baseline(cm_comps, cm_samp, 37, 29, cm_q, cm_tq, 2, restart=3))
    res = ctxs(False, sem, opts=(("jpeg_cmyk", 1),)).decode_batch(files)
    assert res[8][0] == 0, (res[8][0], _lib().last_error())
    _same(res[8][1], RC.decode(cm_comps, cm_samp, 37, 29, cm_q, cm_tq, 2, sem), "ycck beside multiscan")
    plain = ctxs(False, sem, ms=False).decode_batch(others)
    for c, k in zip(ms, where_ms):
        assert res[k][0] == 0, (c.label, res[k][0], _lib().last_error())
        _same(res[k][1], c.ref(sem), c.label)
    for k, (st0, a0, _) in zip(where_other, plain):
        assert st0 == 0 and res[k][0] == 0, k
        assert np.array_equal(res[k][1], a0), k
    for k in (1, 5, 7):  # and the ordinary members are the oracle's
        with O.semantics(O.SEM_ZUNE if sem else O.SEM_LIBJPEG):
            ref = O.jpeg_decode(files[k])[1]
        _same(res[k][1], ref, "ordinary %d" % k)


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_file_cut_inside_its_second_scan(ctxs, sem):
    L = _lib()
    c = Case("420", 131, 67, [[0], [1, 2]], seed=71, quality=90)
    _, parts = R.multiscan(c.comps, c.samp, c.w, c.h, c.qtabs, c.script, parts=True)
    cut = c.data[:(parts[1][0] + parts[1][1]) // 2]
    whole_cut = synth.make_jpeg(72, 131, 67, 90, "4:2:0")
    whole_cut = whole_cut[:len(whole_cut) * 2 // 3]  # an ordinary truncated file: the status to match
    good = Case("422", 37, 29, R.SCRIPTS[0], seed=73)
    plainf = synth.make_jpeg(74, 64, 48, 85, "4:2:0")
    ctx = ctxs(False, sem)
    res = ctx.decode_batch([good.data, cut, plainf, whole_cut, c.data])
    assert res[3][0] != 0 and res[1][0] == res[3][0] == L.DG_ERR_CORRUPT and res[1][1] is None
    _same(res[0][1], good.ref(sem), good.label)
    _same(res[4][1], c.ref(sem), c.label)
    plain = ctxs(False, sem, ms=False).decode_batch([plainf])[0]
    assert res[2][0] == 0 and np.array_equal(res[2][1], plain[1])


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_other_paths(ctxs, sem):
    L = _lib()
    cases = [Case("420", 131, 67, R.SCRIPTS[2], seed=41, quality=90), Case("mixed_12", 37, 29, R.SCRIPTS[0], seed=42, restart=3)]
    datas = [c.data for c in cases]
    # dg_decode_one
    st, arr, m = ctxs(False, sem).decode_one(datas[0])
    assert st == L.DG_OK and (m.width, m.height) == (131, 67)
    _same(arr, cases[0].ref(sem), cases[0].label)
    # image_to_rgb8 with the JPEG re-encoder
    enc = ctxs(False, sem, image_to_rgb8=True, pre_encode_images=True, encode_format=1, jpeg_quality=92)
    for c, (st, buf, m) in zip(cases, enc.decode_batch(datas)):
        assert st == 0 and m.is_encoded == 1, c.label
        assert buf.tobytes() == O.jpeg_encode(c.ref(sem), 92), c.label
    # coded bytes in device memory (dg_submit_device): a scan is addressed inside the caller's buffer
    for c, (st, t, m) in zip(cases, ctxs(False, sem).decode_batch_torch(datas)):
        assert st == 0, c.label
        _same(t.cpu().numpy(), c.ref(sem), c.label)


def test_submission_split_under_a_device_budget():
    """A split never separates an image from its scan descriptors: every member stays bit-exact."""
    L = _lib()
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)

    def ctx(budget):
        c = L.Context(0, **kw)
        c.set_option("coef_cache_mb", 0)
        c.set_option("jpeg_multiscan", 1)
        if budget is None:
            c.set_option("budget_plan", 0)
        c.set_option("max_device_mb", (1 << 20) if budget is None else budget)
        return c
    base = ctx(None)
    assert base.decode_batch([synth.make_jpeg(1, 32, 32, 90)])[0][0] == 0
    base_mb = base.stat("device_mb")
    base.close()
    rng = np.random.default_rng(5)
    datas = []
    for k in range(16):
        w, h = int(rng.integers(300, 640)), int(rng.integers(300, 640))
        if k % 2:
            datas.append(synth.make_jpeg(100 + k, w, h, 90, "4:2:0"))
        else:
            name = ("420", "422", "444")[k // 2 % 3]
            datas.append(Case(name, w, h, R.SCRIPTS[k // 2 % 4], seed=k, quality=85, restart=(0, 9)[k // 2 % 2]).data)
    ref = ctx(None)
    want = ref.decode_batch(datas)
    peak = ref.stat("peak_device_mb")
    ref.close()
    assert peak > base_mb
    c = ctx(base_mb + max(8, (peak - base_mb) // 3))
    got = c.decode_batch(datas)
    assert c.stat("budget_splits") > 0, (peak, base_mb)
    for (s0, a0, _), (s1, a1, _) in zip(want, got):
        assert s0 == s1 == 0
        assert np.array_equal(a0, a1)
    c.close()
