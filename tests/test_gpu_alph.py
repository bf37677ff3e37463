"""Lossy WebP with alpha on the GPU behind context option "webp_alpha" beside "webp_lossy"
(dg_alph.hip): bit-exact against tests/ref_alph.py (pinned to Pillow in test_alph_cpu.py), and
past the decode against the oracle's result for the RGBA PNG twin of the same pixels.  Covers
the option (off, or on without webp_lossy: nothing changes), every Pillow-made and crafted file
of alph_cases.py, the refusals through the library with their texts, a mixed batch with
truncated alpha members, more images in one batch than a wave has lanes, and everything
downstream of the decode."""
import io

import numpy as np
import pytest
from PIL import Image

import alph_cases as K
import alph_craft as A
import ref_alph as R
import vp8_cases
import webp_cases
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CFG = (224, 16, 0.5, 2.0)
PILLOW = K.pillow_cases()
CRAFTED = K.crafted_cases()
REFUSED_OFF = "WebP: lossy WebP with alpha"


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (resize, options), made once per module."""
    cache = {}

    def get(resize=False, webp_lossy=True, webp_alpha=True, **extra):
        key = (resize, webp_lossy, webp_alpha, tuple(sorted(extra.items())))
        if key not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if resize else {}
            cache[key] = _lib().Context(0, webp_lossy=webp_lossy, webp_alpha=webp_alpha, **kw, **extra)
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


@pytest.fixture(scope="module")
def refs():
    """ref_alph's pixels of a file as an array, computed once."""
    cache = {}

    def get(data):
        if data not in cache:
            r = R.decode(data)
            assert r.status == R.OK, r.why
            cache[data] = np.frombuffer(r.pixels, np.uint8).reshape(r.height, r.width, r.channels)
        return cache[data]
    return get


@pytest.fixture(scope="module")
def downstream():
    """Files for everything past the decode, written by Pillow: a raw-coded and two VP8L-coded planes, one file of
    its bucket's size and one a column wider than a bucket (an x.5 crop)."""
    t = B.ARAwareTransform(*CFG)
    bw, bh = t.target_size(300, 200)
    assert t.target_size(bw + 1, bh) == (bw, bh) and t.target_size(bw, bh) == (bw, bh)
    out = []
    for seed, (w, h), alpha, hdr, kw in ((1, (300, 200), K.noise(5, 200, 300), 0, {}), (2, (131, 67), K.blob(67, 131), None, {}),
                                         (3, (260, 330), K.binary(330, 260), 1, dict(alpha_quality=100)),
                                         (4, (bw, bh), K.blob(bh, bw), None, dict(alpha_quality=50)),
                                         (5, (bw + 1, bh), K.hgrad(bh, bw + 1), None, dict(method=0))):
        data = A.save(np.dstack([A.photo(seed, h, w), alpha]), quality=75, **kw)
        assert hdr is None or A.alph_of(data)[0] == hdr
        out.append(data)
    assert {A.alph_of(d)[0] & 3 for d in out} == {0, 1}
    return out


def _same(arr, ref, label):
    assert arr is not None and tuple(arr.shape[:2]) == tuple(ref.shape[:2]), label
    got = np.asarray(arr).reshape(ref.shape)
    assert np.array_equal(got, ref), (label, int((got != ref).sum()))


def _twin(px):
    b = io.BytesIO()
    Image.fromarray(px).save(b, "PNG")
    return b.getvalue()


def _transformed(px, to_rgb8=False):
    """The oracle's result for these pixels in the CFG buckets."""
    t = B.ARAwareTransform(*CFG)
    tw, th = t.target_size(px.shape[1], px.shape[0])
    resized = (tw, th) != (px.shape[1], px.shape[0])
    out = O.crop_and_resize(px, tw, th, O.MODE_FIR) if resized else px
    return O.to_rgb8(out, resized) if to_rgb8 else out


# ------------------------------------------------------------------ the option

def test_option_on_decodes_and_off_changes_nothing(ctxs, refs):
    L = _lib()
    files = [PILLOW[0][1], PILLOW[2][1], dict(CRAFTED)["raw_f3_17x33"]]
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    on = ctxs().decode_batch([jpg] + files)
    assert on[0][0] == L.DG_OK
    for d, (st, arr, m) in zip(files, on[1:]):
        assert st == L.DG_OK and (m.channels, m.bit_depth, m.is_encoded) == (4, 8, 0), L.last_error()
        _same(arr, refs(d), "on")
    # off, with webp_lossy: the refusal of before, from every entry point, and a neighbouring JPEG's pixels unchanged
    for ctx in (ctxs(webp_alpha=False), ctxs(webp_alpha=False, webp=True)):
        res = ctx.decode_batch([jpg] + files + [jpg])
        assert res[0][0] == L.DG_OK and res[-1][0] == L.DG_OK
        assert np.array_equal(res[0][1], on[0][1]) and np.array_equal(res[-1][1], on[0][1])
        for d, (st, arr, m) in zip(files, res[1:-1]):
            assert st == L.DG_ERR_UNSUPPORTED and arr is None
            assert ctx.output_size(d)[0] == L.DG_ERR_UNSUPPORTED and REFUSED_OFF in L.last_error()
            assert ctx.decode_one(d)[0] == L.DG_ERR_UNSUPPORTED
    # on without webp_lossy: as if neither were set (an extended file is an unknown format, or "lossy WebP" under webp)
    alone = ctxs(webp_lossy=False)
    res = alone.decode_batch([jpg] + files)
    assert res[0][0] == L.DG_OK and np.array_equal(res[0][1], on[0][1])
    for d, (st, arr, m) in zip(files, res[1:]):
        assert st == L.DG_ERR_CORRUPT and arr is None and alone.output_size(d)[0] == L.DG_ERR_CORRUPT
    assert ctxs(webp_lossy=False, webp=True).output_size(files[0])[0] == L.DG_ERR_UNSUPPORTED
    assert "WebP: lossy WebP" in L.last_error() and "alpha" not in L.last_error()
    # a file without alpha is what it was, under either setting
    plain = vp8_cases.pillow_cases()[0][1]
    a, b = ctxs().decode_batch([plain])[0], ctxs(webp_alpha=False).decode_batch([plain])[0]
    assert a[0] == b[0] == L.DG_OK and a[2].channels == 3 and np.array_equal(a[1], b[1])


def test_option_values_and_probe():
    L = _lib()
    ctx = L.Context(0, webp_lossy=True)
    data = PILLOW[0][1]
    before = [L.probe(d) for d in (data, dict(CRAFTED)["vp8l_index_f1_17x33"])]
    assert ctx.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    ctx.set_option("webp_alpha", 1)
    assert ctx.output_size(data) == (L.DG_OK, 64 * 48 * 4)
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("webp_alpha", bad)
        assert e.value.status == L.DG_ERR_INVALID and "webp_alpha" in L.last_error()
    assert ctx.output_size(data) == (L.DG_OK, 64 * 48 * 4)  # a refused value changes nothing
    ctx.set_option("webp_alpha", 0)
    assert ctx.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    for bad in (2, -1):
        with pytest.raises(L.DgError):
            ctx.set_option("webp_alpha", bad)
    assert ctx.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    after = [L.probe(d) for d in (data, dict(CRAFTED)["vp8l_index_f1_17x33"])]  # dg_probe describes the default options
    for (st0, i0), (st1, i1) in zip(before, after):
        assert st0 == st1 and bytes(i0) == bytes(i1)
    ctx.close()


# ------------------------------------------------------------------ decode

def test_decode_bit_exact_in_one_batch(ctxs, refs):
    L = _lib()
    cases = PILLOW + CRAFTED + K.plain_cases()
    ctx = ctxs()
    res = ctx.decode_batch([d for _, d in cases])
    for (label, d), (st, arr, m) in zip(cases, res):
        assert st == L.DG_OK, (label, st, L.last_error())
        ref = refs(d)
        _same(arr, ref, label)
        assert (m.original_width, m.original_height, m.width, m.height) == (ref.shape[1], ref.shape[0]) * 2, label
        assert (m.channels, m.bit_depth, m.is_encoded) == (ref.shape[2], 8, 0), label
        assert m.nbytes == ref.size, label
    assert all(refs(d).shape[2] == 4 for _, d in PILLOW + CRAFTED) and all(refs(d).shape[2] == 3 for _, d in K.plain_cases())
    # the colour channels are those of the same VP8 chunk without the alpha
    for label, d in PILLOW[:3] + CRAFTED[::17]:
        (st, arr, m), = ctxs(webp_alpha=False).decode_batch([A.without_alph(d)])
        assert st == L.DG_OK
        _same(arr, refs(d)[..., :3], label)


def test_alone_and_through_decode_one(ctxs, refs):
    L = _lib()
    ctx = ctxs()
    for label, d in PILLOW[::2] + CRAFTED[::9]:
        (st, arr, m), = ctx.decode_batch([d])
        assert st == L.DG_OK, label
        _same(arr, refs(d), label)
        st, arr, m = ctx.decode_one(d)
        assert st == L.DG_OK and (m.channels, m.bit_depth) == (4, 8), label
        _same(arr, refs(d), label)
        assert ctx.output_size(d) == (L.DG_OK, refs(d).size), label


def test_refusals_through_the_library(ctxs, refs):
    L = _lib()
    ctx = ctxs()
    good = dict(CRAFTED)["vp8l_cache_f3_17x33"]
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    (_, jref, _), = ctx.decode_batch([jpg])
    refused = K.refusals()
    res = ctx.decode_batch([good] + [r[1] for r in refused] + [good, jpg])
    for (label, d, status, text, stream, _), (st, arr, m) in zip(refused, res[1:]):
        want = L.DG_ERR_UNSUPPORTED if status == "UNSUPPORTED" else L.DG_ERR_CORRUPT
        assert st == want and arr is None, (label, st)
    for st, arr, m in (res[0], res[-2]):  # the other members of the batch stay exact
        assert st == L.DG_OK
        _same(arr, refs(good), "good beside refused")
    assert res[-1][0] == L.DG_OK and np.array_equal(res[-1][1], jref)
    for label, d, status, text, stream, _ in refused:  # each names itself: the header's at planning, the stream's at completion
        want = L.DG_ERR_UNSUPPORTED if status == "UNSUPPORTED" else L.DG_ERR_CORRUPT
        if stream:
            assert ctx.output_size(d)[0] == L.DG_OK, label
            (st, arr, m), = ctx.decode_batch([d])
            assert arr is None, label
        else:
            st = ctx.output_size(d)[0]
        assert st == want and text in L.last_error(), (label, st, L.last_error())
        assert ctxs(webp_alpha=False).output_size(d)[0] == L.DG_ERR_UNSUPPORTED and REFUSED_OFF in L.last_error(), label


def test_mixed_batch_with_truncated_alpha_members(ctxs, refs):
    L = _lib()
    ctx = ctxs(webp=True)
    jpg = synth.make_jpeg(71, 300, 200, 90)
    png = synth.make_png(72, 150, 260, "RGBA")
    lossless = webp_cases.pillow_cases()[0][1]
    lossy = vp8_cases.pillow_cases()[0][1]
    raw, coded, few = dict(PILLOW)["noise"], dict(PILLOW)["blob"], dict(CRAFTED)["vp8l_index_f3_65x65"]
    cuts = [K.cut_stream(d, k) for d in (raw, coded, few) for k in (1, 2, 7, len(A.alph_of(d)) // 2)]
    members = [jpg, raw, cuts[0], png, coded, cuts[4], lossless, lossy, few] + cuts[1:4] + cuts[5:] + [coded, jpg]
    res = ctx.decode_batch(members)
    alone = [ctx.decode_batch([d])[0] for d in members]
    kinds = {"ok": 0, "corrupt": 0}
    for i, (d, (st, arr, m), (ast, aarr, am)) in enumerate(zip(members, res, alone)):
        assert st == ast and (m.channels, m.width, m.height) == (am.channels, am.width, am.height), i
        if d in (jpg, png, lossless):
            assert st == L.DG_OK and np.array_equal(arr, aarr), i
            continue
        r = R.decode(d)  # every WebP member, whole or cut, is ref_alph's answer
        if r.status == R.OK:
            _same(arr, np.frombuffer(r.pixels, np.uint8).reshape(r.height, r.width, r.channels), "member %d" % i)
            assert np.array_equal(arr, aarr), i
            kinds["ok"] += 1
        else:
            assert st == L.DG_ERR_CORRUPT and arr is None and aarr is None, (i, st)
            kinds["corrupt"] += 1
    assert kinds["ok"] >= 6 and kinds["corrupt"] >= 10  # a cut of one byte of the few-levels stream decodes
    assert np.array_equal(res[0][1], res[-1][1]) and np.array_equal(res[4][1], res[-2][1])


def test_seventy_of_one_file_in_one_batch(ctxs, refs):
    L = _lib()
    d = dict(PILLOW)["blob_aq50"]
    res = ctxs().decode_batch([d] * 70)  # more images, and more companion descriptors, than a wave has lanes
    for i, (st, arr, m) in enumerate(res):
        assert st == L.DG_OK, i
        _same(arr, refs(d), "copy %d" % i)


# ------------------------------------------------------------------ downstream of the decode

def test_resized_and_cropped_as_the_png_twin(ctxs, refs, downstream):
    L = _lib()
    ctx = ctxs(resize=True)
    res = ctx.decode_batch(downstream)
    twins = ctx.decode_batch([_twin(refs(d)) for d in downstream])
    for i, (d, (st, arr, m), (tst, tarr, tm)) in enumerate(zip(downstream, res, twins)):
        assert st == L.DG_OK and tst == L.DG_OK, (i, st)
        exp = _transformed(refs(d))
        _same(arr, exp, "file %d" % i)
        _same(tarr, exp, "twin %d" % i)
        assert (m.bucket, m.width, m.height, m.channels, m.bit_depth) == (tm.bucket, tm.width, tm.height, 4, 8), i
        assert (m.original_width, m.original_height) == (refs(d).shape[1], refs(d).shape[0]), i
    st, arr, m = ctx.decode_one(downstream[4])
    assert st == L.DG_OK
    _same(arr, _transformed(refs(downstream[4])), "decode_one, a column wider than its bucket")
    assert ctx.output_size(downstream[0]) == (L.DG_OK, _transformed(refs(downstream[0])).size)


@pytest.mark.parametrize("resize", [False, True], ids=["decode", "resize"])
def test_image_to_rgb8(ctxs, refs, downstream, resize):
    L = _lib()
    for i, (d, (st, arr, m)) in enumerate(zip(downstream, ctxs(resize=resize, image_to_rgb8=True).decode_batch(downstream))):
        assert st == L.DG_OK and (m.channels, m.bit_depth) == (3, 8), i
        exp = _transformed(refs(d), True) if resize else O.to_rgb8(refs(d), False)
        _same(arr, exp, "file %d" % i)


@pytest.mark.parametrize("fmt", [0, 1], ids=["png", "jpeg"])
def test_pre_encode_equals_the_twins_file(ctxs, refs, downstream, fmt):
    L = _lib()
    for resize in (False, True):
        ctx = ctxs(resize=resize, pre_encode_images=True, encode_format=fmt, jpeg_quality=92)
        res = ctx.decode_batch(downstream[:3])
        twins = ctx.decode_batch([_twin(refs(d)) for d in downstream[:3]])
        for i, ((st, buf, m), (tst, tbuf, tm)) in enumerate(zip(res, twins)):
            assert st == L.DG_OK and tst == L.DG_OK and m.is_encoded == 1 and m.channels == -1, i
            assert buf.tobytes() == tbuf.tobytes(), (fmt, resize, i)
        if fmt == 0:  # and the PNG round-trips to the transformed pixels
            back = np.asarray(Image.open(io.BytesIO(res[0][1].tobytes())))
            _same(back, _transformed(refs(downstream[0])) if resize else refs(downstream[0]), "round trip")


def test_host_and_device_submission(ctxs, refs, downstream):
    L = _lib()
    ctx = ctxs(resize=True)
    files = [synth.make_jpeg(71, 300, 200, 90), downstream[1], synth.make_png(72, 150, 260, "RGBA"), downstream[0]]
    host = ctx.decode_batch(files)
    dev = ctx.decode_batch_torch(files)
    for i, ((hst, harr, hm), (dst, darr, dm)) in enumerate(zip(host, dev)):
        assert hst == dst == L.DG_OK, i
        assert np.array_equal(harr, darr.cpu().numpy()), i
    _same(host[1][1], _transformed(refs(files[1])), "the VP8L-coded alpha")
    _same(host[3][1], _transformed(refs(files[3])), "the raw-coded alpha")


def test_sample_alignment_with_an_alpha_member(refs, downstream):
    """A lossy WebP with alpha under the reference member's name decides the sample's bucket (dg_probe reads its VP8X
    canvas) and comes back RGBA."""
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    from datago_amd.samples import BinaryFile, TarballSample, process_sample
    tfm = ARAwareTransform(ImageTransformConfig(True, CFG[0], CFG[1], CFG[2], CFG[3]), 0, webp_lossy=True, webp_alpha=True)
    webp = downstream[1]
    px = refs(webp)
    mask = synth.make_png(81, px.shape[1], px.shape[0] - 10, "L")
    s = TarballSample("shard-0.tar", [BinaryFile("k1.jpg", webp), BinaryFile("k1.png", mask)])
    out = process_sample(s, tfm, ImageEncoding(), "jpg")
    assert out is not None and not out.unsupported
    t = B.ARAwareTransform(*CFG)
    target = t.target_size(px.shape[1], px.shape[0])
    assert (out.image.width, out.image.height, out.image.channels) == target + (4,)
    assert (out.image.original_width, out.image.original_height) == (px.shape[1], px.shape[0])
    assert np.frombuffer(out.image.data, np.uint8).tobytes() == _transformed(px).tobytes()
    m = out.additional_images["k1.png"]
    _, dec = O.decode_any(mask)
    assert (m.width, m.height) == target
    assert np.frombuffer(m.data, np.uint8).tobytes() == O.crop_and_resize(dec, target[0], target[1], O.MODE_FIR).tobytes()
