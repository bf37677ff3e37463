"""Every format in one batch with every format option on: batch = alone = reference.

test_gpu_batch_vs_alone.py guards what a batch carries from one image to the next (blob offsets of palettes, segment
tables and encoder tables, the shift of the aliased late region, chunk and flag numbering, the per-format launch
gates, the walk that skips failed images) over JPEG and PNG.  Here the corpus of all_formats_cases.py -- JPEG in all
its forms, PNG, GIF, the three kinds of WebP, BMP and the three kinds of TIFF, with header-level and stream-level
refusals between them -- is decoded alone, then as one batch in every rotation that puts another family first,
through the host path and the device-pointer path; the same under the transform and both encoders, through one
context over changing batches, and split under a device budget.  The last section brings TIFF level with the other
formats' own tests.  Every comparison is exact."""
import numpy as np
import pytest

import all_formats_cases as A
import ref_resize16 as R16
import tiff16_craft as S
import tiff_craft as T
import tiff_deflate_craft as D
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O
from test_gpu_batch_vs_alone import _bytes, _meta
from test_gpu_tiff import CFG, RESIZE, _check as _check8, _written
from test_gpu_tiff16 import _check as _check16

pytestmark = pytest.mark.gpu

BUCKETS = dict(crop_and_resize=True, default_image_size=64, downsampling_ratio=8, min_aspect_ratio=0.5,
               max_aspect_ratio=2.0)
# (id, context arguments, options, sample bits of the members it takes)
CONFIGS = {"raw": ({}, {}, 8),
           "enc_png": (dict(pre_encode_images=True, encode_format=0), {}, 8),
           "enc_jpeg": (dict(pre_encode_images=True, encode_format=1), {}, 8),
           "deep_png": (dict(pre_encode_images=True, encode_format=0), dict(resize16=1, penc16=1, penc_dynamic=1), 16)}
BITS = {m[1]: m[4] for m in A.corpus()}


def _lib():
    from datago_amd import _lib as L
    return L


def _ctx(transform=False, opts=(), **kw):
    ctx = _lib().Context(0, **(BUCKETS if transform else {}), **kw)
    for k, v in list(A.ALL_ON.items()) + list(dict(opts).items()):
        ctx.set_option(k, v)
    ctx.set_option("inf_chunk", 4096)
    ctx.set_option("prog_split", 0)  # the progressive member stays in the batch, between the others
    return ctx


def _status(name):
    L = _lib()
    return {A.CORRUPT: L.DG_ERR_CORRUPT, A.UNSUPPORTED: L.DG_ERR_UNSUPPORTED}[name]


def _one(res):
    st, arr, m = res
    return st, _bytes(arr), _meta(m)


def _alone(ctx, batch):
    """{label: (status, bytes, meta)} of one submit per file."""
    return {label: _one(ctx.decode_batch([data])[0]) for label, data, _ in batch}


def _assert_batch(ctx, batch, alone, what):
    """The batch through the host path and the device-pointer path: status, every meta field and the bytes as alone."""
    L = _lib()
    datas = [data for _, data, _ in batch]
    for path, res in (("host", ctx.decode_batch(datas)), ("device", ctx.decode_batch_torch(datas))):
        assert len(res) == len(batch)
        for (label, _, _), r in zip(batch, res):
            st, raw, meta = _one(r)
            st1, raw1, meta1 = alone[label]
            assert st == st1, (what, path, label, L.STATUS_NAMES.get(st, st), L.STATUS_NAMES.get(st1, st1))
            assert meta == meta1, (what, path, label)
            assert raw == raw1, (what, path, label)


# ------------------------------------------------------------------ a. decode only, every rotation

@pytest.fixture(scope="module")
def decoded():
    """Every file of the order decoded alone, once: {label: (status, bytes, meta)}."""
    ctx = _ctx()
    out = _alone(ctx, A.order())
    assert ctx.stat("png_chunks") > 0
    ctx.close()
    return out


@pytest.fixture(scope="module")
def batch_ctx():
    ctx = _ctx()
    yield ctx
    ctx.close()


def test_alone_equals_the_reference(decoded):
    L = _lib()
    corpus = A.corpus()
    assert len(corpus) >= 40
    for fam, label, data, ref, bits in corpus:
        st, raw, meta = decoded[label]
        assert st == L.DG_OK, (label, L.STATUS_NAMES.get(st, st))
        got = np.frombuffer(raw, np.uint16 if bits == 16 else np.uint8)
        assert got.size == ref.size and np.array_equal(got.reshape(ref.shape), ref), (label, got.size, ref.shape)
        m = dict(zip([f for f, _ in L.PayloadMeta._fields_], meta))
        assert (m["original_width"], m["original_height"], m["width"], m["height"]) == (ref.shape[1], ref.shape[0]) * 2, label
        assert (m["channels"], m["bit_depth"], m["is_encoded"]) == (ref.shape[2], bits, 0), label
    for label, data, status, fam in A.bad():
        assert decoded[label][0] == _status(status) and decoded[label][1] is None, (label, decoded[label][0])


@pytest.mark.parametrize("k", range(1 + len(A.FAMILIES)), ids=["bad_first"] + [f + "_first" for f in A.FAMILIES])
def test_batch_equals_alone_in_every_rotation(decoded, batch_ctx, k):
    name, batch = A.rotations()[k]
    assert len(batch) >= 48 and {m[2] for m in batch} == set(A.FAMILIES) | {None}
    assert batch[0][2] == (A.FAMILIES[k - 1] if k else None)
    c0 = batch_ctx.stat("png_chunks")
    _assert_batch(batch_ctx, batch, decoded, name)
    assert batch_ctx.stat("png_chunks") > c0


# ------------------------------------------------------------------ b. under the transform and both encoders

def _members(bits):
    """The order's members of one sample depth, the failing files among them."""
    return [m for m in A.order() if m[2] is None or BITS[m[0]] == bits]


@pytest.fixture(scope="module")
def transformed():
    """{config: {label: (status, bytes, meta)}}: every member alone under each configuration, computed once."""
    cache = {}

    def get(cfg):
        if cfg not in cache:
            kw, opts, bits = CONFIGS[cfg]
            ctx = _ctx(True, opts, **kw)
            cache[cfg] = _alone(ctx, _members(bits))
            ctx.close()
        return cache[cfg]
    return get


def _target(w, h):
    return B.ARAwareTransform(BUCKETS["default_image_size"], BUCKETS["downsampling_ratio"], 0.5, 2.0).target_size(w, h)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_transformed_batch_equals_alone(transformed, cfg):
    L = _lib()
    kw, opts, bits = CONFIGS[cfg]
    members, alone = _members(bits), transformed(cfg)
    fields = [f for f, _ in L.PayloadMeta._fields_]
    resized = 0
    for fam, label, data, ref, b in A.corpus():
        if b != bits:
            continue
        st, raw, meta = alone[label]
        assert st == L.DG_OK, (cfg, label, L.STATUS_NAMES.get(st, st), L.last_error())
        m = dict(zip(fields, meta))
        tw, th = _target(ref.shape[1], ref.shape[0])
        assert (m["width"], m["height"], m["is_encoded"]) == (tw, th, int(bool(kw))), (cfg, label)
        resized += (tw, th) != (ref.shape[1], ref.shape[0])
        if cfg == "raw":  # the families' own tests pin the resize of their decoded pixels to the oracle exactly
            exp = O.crop_and_resize(ref, tw, th, O.MODE_FIR) if (tw, th) != (ref.shape[1], ref.shape[0]) else ref
            got = np.frombuffer(raw, np.uint8)
            assert got.size == exp.size and np.array_equal(got.reshape(exp.shape), exp), (label, got.size, exp.shape)
    assert resized >= (20 if bits == 8 else 5), resized
    for label, data, status, fam in A.bad():
        assert alone[label][0] == _status(status), (cfg, label)
    first = [next(m[0] for m in members if m[2] == ("tiff" if bits == 8 else "tiff16")),
             A.BMP_NO_INDEX if bits == 8 else next(m[0] for m in members if m[2] == "png"),
             next(m[0] for m in members if m[2] == ("jpeg" if bits == 8 else "tiff16") and "lzw" not in m[0])]
    assert len(set(first)) == 3
    ctx = _ctx(True, opts, **kw)
    for label in first:
        _assert_batch(ctx, A.rotated(members, label), alone, (cfg, label + " first"))
    ctx.close()


# ------------------------------------------------------------------ c. one context, changing batches

def test_one_context_over_changing_batches(transformed):
    """A kernel that relied on arena bytes an earlier batch left behind, or a launch gate that was not reset, would
    show when a batch of one kind follows a batch of another in the same context (slots at its default)."""
    alone = transformed("raw")
    mixed = _members(8)
    stream = {b[0]: b[3] for b in A.bad()}  # a stream-level refusal goes with its format's batch
    only = lambda fams: [m for m in mixed if (m[2] or stream[m[0]]) in fams]  # noqa: E731
    tiff, jpeg, webp_gif = only(("tiff", "tiff_deflate")), only(("jpeg",)), only(("webp", "gif"))
    assert len(tiff) >= 8 and len(jpeg) >= 9 and len(webp_gif) >= 14
    ctx = _ctx(True)
    for step, batch in enumerate([tiff, jpeg, mixed, webp_gif, mixed[::-1], tiff]):
        _assert_batch(ctx, batch, alone, "step %d" % step)
    ctx.close()


# ------------------------------------------------------------------ d. a split under a device budget

BUDGET_KW = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5,
                 max_aspect_ratio=2.0)


def _budget_ctx(exact):
    """test_gpu_budget.py's contexts: no Lanczos table cache; exact: exact-size buffers under a huge budget."""
    c = _lib().Context(0, **BUDGET_KW)
    for k, v in list(A.ALL_ON.items()) + [("resize16", 1), ("coef_cache_mb", 0)]:
        c.set_option(k, v)
    if exact:
        c.set_option("budget_plan", 0)
        c.set_option("max_device_mb", 1 << 20)
    return c


def test_split_under_a_device_budget():
    """Three members of every family, 400 to 700 px a side, in one submission under a third of their footprint.
    Measured on an MI355X: peak_device_mb 436 of the unbudgeted run, base 234 (peak - base 202 MB); the budget of
    301 MB then gave 3 splits and a peak of 284 MB."""
    L = _lib()
    files = A.large()
    datas = [m[2] for m in files]
    assert {m[0] for m in files} == set(A.FAMILIES)
    c = _budget_ctx(True)
    assert c.decode_batch([synth.make_jpeg(1, 32, 32, 90)])[0][0] == 0
    base = c.stat("device_mb")
    c.close()
    ref = _budget_ctx(True)
    want = ref.decode_batch(datas)
    peak = ref.stat("peak_device_mb")
    ref.close()
    print("budget: peak_device_mb %d base %d" % (peak, base))
    assert peak - base >= 24, (peak, base)
    budget = base + max(8, (peak - base) // 3)
    c = _budget_ctx(False)
    c.set_option("max_device_mb", budget)
    got = c.decode_batch(datas)
    print("budget: %d splits %d peak %d" % (budget, c.stat("budget_splits"), c.stat("peak_device_mb")))
    assert c.stat("budget_splits") > 0, (peak, base, budget)
    for (fam, label, _), (s0, a0, m0), (s1, a1, m1) in zip(files, want, got):
        assert s0 == s1 == L.DG_OK, (label, s0, s1)
        assert _meta(m0) == _meta(m1) and _bytes(a0) == _bytes(a1), label
    assert c.stat("peak_device_mb") <= budget + 16, (c.stat("peak_device_mb"), budget)
    c.close()


# ------------------------------------------------------------------ e. TIFF level with the other formats

def test_tiff_both_decode_semantics():
    L = _lib()
    eight = T.cases()[::4] + [c[1:] for c in D.cases()[::3]]
    deep = S.forms()[::2]
    assert len(eight) >= 20 and len(deep) >= 8
    for sem in (0, 1):
        c = L.Context(0, tiff=True, tiff_deflate=True, tiff16=True, decode_semantics=sem)
        _check8(L, eight, c.decode_batch([f[1] for f in eight]))
        _check16(L, deep, c.decode_batch([f[1] for f in deep]))
        c.close()


# (form, channels, WhiteIsZero, arguments of tiff_craft.tiff)
FORMS8 = [("L8", 1, False, dict(comp=5, pred=2, rps=16)), ("WhiteIsZero L8", 1, True, dict(comp=32773, photo=0)),
          ("La8", 2, False, dict(comp=5, pred=2, tile=(64, 48))), ("Rgb8", 3, False, dict(comp=32773, rps=9)),
          ("Rgba8", 4, False, dict(comp=8, pred=2, rps=32, pack=D.z()))]


@pytest.mark.parametrize("form,c,inverted,kw", FORMS8, ids=[f[0].replace(" ", "_") for f in FORMS8])
def test_every_8_bit_channel_count_downstream(form, c, inverted, kw):
    """Resized to its bucket, a TIFF of every channel count gives the oracle's crop_and_resize of its pixels, and what
    the PNG twin of those pixels gives."""
    L = _lib()
    ctx = L.Context(0, tiff=True, tiff_deflate=True, **RESIZE)
    for k, (w, h) in enumerate(((300, 200), (150, 260))):
        stored = T.noise(h, w, c, 70 + 10 * k + c)
        stored[h // 4:h // 2] = stored[0, 0]
        pix = 255 - stored if inverted else stored
        tw, th = B.ARAwareTransform(*CFG).target_size(w, h)
        exp = O.crop_and_resize(pix, tw, th, O.MODE_FIR)
        (st, arr, m), (tst, tarr, tm) = ctx.decode_batch([T.tiff(stored, **kw), synth.pil_png(pix)])
        assert st == tst == L.DG_OK, (form, st, tst, L.last_error())
        assert (m.bucket, m.width, m.height, m.channels, m.bit_depth) == (tm.bucket, tw, th, c, 8), (form, w, h)
        assert (m.original_width, m.original_height) == (w, h)
        assert np.array_equal(np.asarray(arr).reshape(exp.shape), exp), (form, w, h)
        assert np.array_equal(np.asarray(tarr).reshape(exp.shape), exp), (form, w, h, "twin")
    ctx.close()


@pytest.mark.parametrize("c,ctype", [(2, 4), (4, 6)], ids=["La16", "Rgba16"])
def test_16_bit_alpha_forms_downstream(c, ctype):
    """The two forms test_gpu_tiff16.py's twin test leaves out: resized, converted and re-encoded as the 16-bit PNG
    twin of the same samples, and resized as tests/ref_resize16.py resizes them."""
    L = _lib()
    opts = dict(tiff=True, tiff_deflate=True, tiff16=True, png16=True, **RESIZE)
    for k, (w, h) in enumerate(((300, 200), (150, 260))):
        pix = S.noise16(h, w, c, 80 + k)
        data = S.tiff16("", pix, comp=8, pred=2, rps=16, be=k == 1, pack=D.z())[1]
        twin = synth.encode_png16(pix, ctype, np.random.default_rng(5))
        for kw, enc in [(dict(resize16=True), 0), (dict(resize16=True, image_to_rgb8=True), 0),
                        (dict(resize16=True, penc16=True, penc_dynamic=True, pre_encode_images=True, encode_format=0), 1)]:
            ctx = L.Context(0, **opts, **kw)
            (st, arr, m), (tst, tarr, tm) = ctx.decode_batch([data, twin])
            assert st == tst == L.DG_OK, (kw, st, tst, L.last_error())
            assert _meta(m) == _meta(tm) and m.is_encoded == enc, (kw, w, h)
            assert arr.tobytes() == tarr.tobytes() and len(arr.tobytes()) > 0, (kw, w, h)
            if len(kw) == 1:
                assert (m.channels, m.bit_depth) == (c, 16)
                np.testing.assert_array_equal(arr, R16.resize_to_fill(pix, m.width, m.height))
            ctx.close()


def _sample(ref_member, mask):
    from datago_amd.samples import BinaryFile, TarballSample
    return TarballSample("shard-0.tar", [BinaryFile("k1.jpg", ref_member), BinaryFile("k1.png", mask)])


def test_sample_alignment_with_a_tiff_reference():
    """load_from_memory sniffs the content: a TIFF under the reference member's name decides the sample's bucket."""
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    from datago_amd.samples import process_sample
    cfg = ImageTransformConfig(True, CFG[0], CFG[1], CFG[2], CFG[3])
    label, tiff, pix = _written("RGB", "tiff_lzw", 1, 300, 200, 11)
    mask = synth.make_png(81, 300, 190, "L")
    out = process_sample(_sample(tiff, mask), ARAwareTransform(cfg, 0, tiff=True), ImageEncoding(), "jpg")
    assert out is not None and not out.unsupported
    target = B.ARAwareTransform(*CFG).target_size(300, 200)
    assert (out.image.width, out.image.height, out.image.channels, out.image.bit_depth) == target + (3, 8)
    assert (out.image.original_width, out.image.original_height) == (300, 200)
    assert np.frombuffer(out.image.data, np.uint8).tobytes() == O.crop_and_resize(pix, target[0], target[1], O.MODE_FIR).tobytes()
    m = out.additional_images["k1.png"]
    _, dec = O.decode_any(mask)
    assert (m.width, m.height) == target
    assert np.frombuffer(m.data, np.uint8).tobytes() == O.crop_and_resize(dec, target[0], target[1], O.MODE_FIR).tobytes()
    # without the option the TIFF member fails to load and is skipped: the mask is its own reference
    off = process_sample(_sample(tiff, mask), ARAwareTransform(cfg, 0), ImageEncoding(), "jpg")
    assert off is not None and off.image.width == 0 and "k1.png" in off.additional_images


def test_sample_alignment_with_a_16_bit_tiff_reference():
    """... and a 16-bit TIFF there gives what the 16-bit PNG of the same samples gives."""
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    from datago_amd.samples import process_sample
    cfg = ImageTransformConfig(True, CFG[0], CFG[1], CFG[2], CFG[3])
    pix = S.noise16(200, 300, 3, 91)
    twin = synth.encode_png16(pix, 2, np.random.default_rng(5))
    mask = synth.make_png(81, 300, 190, "L")
    tiff = S.tiff16("", pix, comp=32773, rps=16, be=True)[1]  # (ARAwareTransform has no tiff_deflate parameter)
    tfm = ARAwareTransform(cfg, 0, png16=True, resize16=True, tiff=True, tiff16=True)
    out = process_sample(_sample(tiff, mask), tfm, ImageEncoding(), "jpg")
    ref = process_sample(_sample(twin, mask), tfm, ImageEncoding(), "jpg")
    assert out is not None and not out.unsupported and ref is not None and not ref.unsupported
    target = B.ARAwareTransform(*CFG).target_size(300, 200)
    assert (out.image.width, out.image.height, out.image.channels, out.image.bit_depth) == target + (3, 16)
    assert out.image == ref.image
    np.testing.assert_array_equal(out.image.to_numpy_array(), R16.resize_to_fill(pix, target[0], target[1]))
    m = out.additional_images["k1.png"]
    assert (m.width, m.height) == target and m == ref.additional_images["k1.png"]


def _at_addresses(ctx, datas, phases):
    """dg_submit_device with file i at a device address of phases[i] mod 4 (decode_batch_torch puts every file on
    a 16-byte boundary): [(status, array or None, meta)]."""
    import torch
    offs, o = [], 64
    for d, ph in zip(datas, phases):
        o = (o + 63) // 64 * 64 + ph
        offs.append(o)
        o += len(d) + 16
    host = torch.zeros(o + 64, dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    for d, of in zip(datas, offs):
        hv[of:of + len(d)] = np.frombuffer(d, np.uint8)
    dev = torch.device("cuda", 0)
    dev_in = host.to(dev)
    sizes = [max(ctx.output_size(d)[1], 1) for d in datas]
    outs = [torch.empty(nb, dtype=torch.uint8, device=dev) for nb in sizes]
    torch.cuda.current_stream(dev).synchronize()
    assert [(dev_in.data_ptr() + of) % 4 for of in offs] == list(phases)
    tk, metas = ctx.submit_device([host.data_ptr() + of for of in offs], [dev_in.data_ptr() + of for of in offs],
                                  [len(d) for d in datas], [t.data_ptr() for t in outs], sizes)
    ctx.wait(tk)
    res = []
    for i, t in enumerate(outs):
        m = metas[i]
        res.append((m.status, t[:m.nbytes].cpu().numpy().reshape(m.height, m.width, -1) if m.status == 0 else None, m))
    return res


def test_segment_tables_from_every_device_address():
    """The eight images with different segment counts of test_gpu_tiff.py and test_gpu_tiff_deflate.py through the
    device-pointer path, each file at device addresses of all four alignments mod 4: k_tiff_lzw and k_tiff_inflate
    read their source in aligned dwords from the address the caller gave."""
    L = _lib()
    pix = [T.noise(70, 97, 3, 20 + k) for k in range(8)]
    rps = (1, 2, 3, 5, 7, 16, 35, 70)
    files = [("lzw rps %d" % r, T.tiff(p, comp=5, pred=2, rps=r, pack=lambda d, k=k: T.lzw(d, end=k % 2 == 0)), p)
             for k, (r, p) in enumerate(zip(rps, pix))]
    files += [("deflate rps %d" % r, T.tiff(p, comp=8, pred=2, rps=r, pack=D.z(1 + k)), p)
              for k, (r, p) in enumerate(zip(rps, pix))]
    datas = [f[1] for f in files]
    ctx = L.Context(0, tiff=True, tiff_deflate=True)
    res = ctx.decode_batch_torch(datas)
    _check8(L, files, [(st, t.cpu().numpy() if st == 0 else None, m) for st, t, m in res])
    for turn in range(4):
        _check8(L, files, _at_addresses(ctx, datas, [(i + turn) % 4 for i in range(len(datas))]))
    ctx.close()
