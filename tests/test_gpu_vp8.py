"""Lossy WebP on the GPU behind context option "webp_lossy" (dg_vp8.hip): bit-exact
against tests/ref_vp8.py (pinned to Pillow in test_vp8_cpu.py), and past the decode
against the oracle's result for the RGB PNG twin of the same pixels.  Covers the
option (off: nothing changes), every Pillow-made and crafted file of vp8_cases.py,
the refusals through the library with their texts, a mixed batch with truncated
members, everything downstream of the decode, and more images in one batch than a
wave has lanes."""
import io

import numpy as np
import pytest
from PIL import Image

import ref_vp8 as R
import vp8_cases as K
import vp8_craft as C
import webp_cases
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CFG = (224, 16, 0.5, 2.0)
PILLOW = K.pillow_cases()
CRAFTED = K.crafted_cases()
EXTENDED_LOSSY = dict((r[0], r[1]) for r in webp_cases.refusals())["extended_lossy"]


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (resize, options), made once per module."""
    cache = {}

    def get(resize=False, webp_lossy=True, **extra):
        key = (resize, webp_lossy, tuple(sorted(extra.items())))
        if key not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if resize else {}
            cache[key] = _lib().Context(0, webp_lossy=webp_lossy, **kw, **extra)
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


@pytest.fixture(scope="module")
def refs():
    """ref_vp8's pixels of a file as an array, computed once."""
    cache = {}

    def get(data):
        if data not in cache:
            r = R.decode(data)
            assert r.status == R.OK, r.why
            cache[data] = np.frombuffer(r.rgb, np.uint8).reshape(r.height, r.width, 3)
        return cache[data]
    return get


@pytest.fixture(scope="module")
def downstream():
    """Files for everything past the decode: a photo, an extended file, a gray one, one of its bucket's size and one
    a column wider than a bucket (an x.5 crop)."""
    t = B.ARAwareTransform(*CFG)
    bw, bh = t.target_size(300, 200)
    assert t.target_size(bw + 1, bh) == (bw, bh) and t.target_size(bw, bh) == (bw, bh)
    rng = np.random.default_rng(62)
    ext = io.BytesIO()
    Image.fromarray(K._photo(rng, 330, 260)).save(ext, "WEBP", quality=80, method=2, exif=b"Exif\0\0II*\0\x08\0\0\0\0\0")
    assert ext.getvalue()[12:16] == b"VP8X"
    return [K.save(K._photo(rng, 200, 300), 75, 4), ext.getvalue(), K.save(np.repeat(K._photo(rng, 67, 131)[..., :1], 3, -1), 60, 0),
            K.save(K._photo(rng, bh, bw), 90, 6), K.save(K._photo(rng, bh, bw + 1), 40, 4)]


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

def test_option_off_changes_nothing(ctxs):
    L = _lib()
    simple = [PILLOW[0][1], CRAFTED[0][1], webp_cases.SIMPLE_LOSSY]
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    for ctx in (ctxs(webp_lossy=False), ctxs(webp_lossy=False, webp=True)):
        res = ctx.decode_batch([jpg] + simple + [jpg])
        assert res[0][0] == L.DG_OK and res[-1][0] == L.DG_OK and np.array_equal(res[0][1], res[-1][1])
        for d, (st, arr, m) in zip(simple, res[1:-1]):  # a simple lossy file: an unknown format from every entry point
            assert st == L.DG_ERR_CORRUPT and arr is None
            assert ctx.output_size(d)[0] == L.DG_ERR_CORRUPT
            assert ctx.decode_one(d)[0] == L.DG_ERR_CORRUPT
    for d in simple:
        st, info = L.probe(d)
        assert st == L.DG_ERR_CORRUPT and info.format == L.DG_FMT_UNKNOWN
    # an extended lossy file: DG_ERR_UNSUPPORTED "WebP: lossy WebP" under webp, DG_ERR_CORRUPT without
    assert ctxs(webp_lossy=False, webp=True).output_size(EXTENDED_LOSSY)[0] == L.DG_ERR_UNSUPPORTED
    assert "WebP: lossy WebP" in L.last_error() and "alpha" not in L.last_error()
    assert ctxs(webp_lossy=False).output_size(EXTENDED_LOSSY)[0] == L.DG_ERR_CORRUPT
    assert L.Context(0).output_size(PILLOW[0][1])[0] == L.DG_ERR_CORRUPT  # the default of a plain context


def test_option_values_and_independence_of_webp():
    L = _lib()
    ctx = L.Context(0)
    data = dict(PILLOW)["photo_130x100"]
    ctx.set_option("webp_lossy", 1)
    assert ctx.output_size(data) == (L.DG_OK, 130 * 100 * 3)
    for d in (PILLOW[0][1], data):  # dg_probe keeps describing the default options
        assert L.probe(d)[0] == L.DG_ERR_CORRUPT
    ctx.set_option("webp_lossy", 0)
    assert ctx.output_size(data)[0] == L.DG_ERR_CORRUPT
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("webp_lossy", bad)
        assert e.value.status == L.DG_ERR_INVALID and "webp_lossy" in L.last_error()
    assert ctx.output_size(data)[0] == L.DG_ERR_CORRUPT  # a refused value changes nothing
    ctx.set_option("webp_lossy", 1)  # without "webp" a lossless file is still refused, simple or extended
    lossless = [K.lossless_file()] + [d for _, d in webp_cases.pillow_cases()[:3]]
    for d in lossless:
        assert ctx.output_size(d)[0] == L.DG_ERR_CORRUPT
        assert ctx.decode_batch([d])[0][0] == L.DG_ERR_CORRUPT
    ctx.set_option("webp", 1)  # and with it both decode in one context
    assert ctx.output_size(lossless[0])[0] == L.DG_OK and ctx.output_size(data)[0] == L.DG_OK
    ctx.close()


# ------------------------------------------------------------------ decode

@pytest.mark.parametrize("which", ["pillow", "crafted"])
def test_decode_bit_exact_in_one_batch(ctxs, refs, which):
    L = _lib()
    cases = PILLOW if which == "pillow" else CRAFTED
    res = ctxs().decode_batch([d for _, d in cases])
    for (label, d), (st, arr, m) in zip(cases, res):
        assert st == L.DG_OK, (label, st, L.last_error())
        ref = refs(d)
        _same(arr, ref, label)
        assert (m.original_width, m.original_height, m.width, m.height) == (ref.shape[1], ref.shape[0]) * 2, label
        assert (m.channels, m.bit_depth, m.is_encoded) == (3, 8, 0), label


def test_alone_and_through_decode_one(ctxs, refs):
    L = _lib()
    ctx = ctxs()
    for label, d in PILLOW[::6] + CRAFTED[::4]:
        (st, arr, m), = ctx.decode_batch([d])
        assert st == L.DG_OK, label
        _same(arr, refs(d), label)
        st, arr, m = ctx.decode_one(d)
        assert st == L.DG_OK and (m.channels, m.bit_depth) == (3, 8), label
        _same(arr, refs(d), label)
        assert ctx.output_size(d) == (L.DG_OK, refs(d).size), label


def test_refusals_through_the_library(ctxs, refs):
    L = _lib()
    ctx = ctxs()
    good = dict(CRAFTED)["bpred_mixed"]
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    (_, jref, _), = ctx.decode_batch([jpg])
    refused = K.refusals()
    res = ctx.decode_batch([good] + [r[1] for r in refused] + [good, jpg])
    for (label, d, status, text, stream), (st, arr, m) in zip(refused, res[1:]):
        want = L.DG_ERR_UNSUPPORTED if status == "UNSUPPORTED" else L.DG_ERR_CORRUPT
        assert st == want and arr is None, (label, st)
    for st, arr, m in (res[0], res[-2]):  # the other members of the batch stay exact
        assert st == L.DG_OK
        _same(arr, refs(good), "good beside refused")
    assert res[-1][0] == L.DG_OK and np.array_equal(res[-1][1], jref)
    for label, d, status, text, stream in refused:  # each names itself: the header's at planning, the stream's at completion
        want = L.DG_ERR_UNSUPPORTED if status == "UNSUPPORTED" else L.DG_ERR_CORRUPT
        if stream:
            assert ctx.output_size(d)[0] == L.DG_OK, label
            (st, arr, m), = ctx.decode_batch([d])
        else:
            st = ctx.output_size(d)[0]
        assert st == want and text in L.last_error(), (label, st, L.last_error())
    both = ctxs(webp=True)  # ALPH and animation under both options: the lossy path's texts
    by = {r[0]: r for r in refused}
    for label in ("alpha", "animation flag", "animation chunks"):
        assert both.output_size(by[label][1])[0] == L.DG_ERR_UNSUPPORTED and by[label][3] in L.last_error(), label


def test_mixed_batch_with_truncated_members(ctxs, refs):
    L = _lib()
    ctx = ctxs(webp=True)
    jpg = synth.make_jpeg(71, 300, 200, 90)
    png = synth.make_png(72, 150, 260, "RGB")
    lossless = webp_cases.pillow_cases()[0][1]
    lossy = [dict(PILLOW)["photo_130x100"], dict(CRAFTED)["parts4_20x77"], dict(CRAFTED)["seg_abs"]]
    cuts = []
    for d in lossy:
        off = R.parse(d)["off"]
        for k in range(5):
            cuts.append(K.fitted_cut(d, off + 12 + k * (len(d) - off - 14) // 4))
    members = [jpg, lossy[0], cuts[0], png, cuts[1], lossless, lossy[1]] + cuts[2:] + [lossy[2], jpg]
    res = ctx.decode_batch(members)
    alone = {id(d): ctx.decode_batch([d])[0] for d in (png, lossless)}
    corrupt = 0
    for i, (d, (st, arr, m)) in enumerate(zip(members, res)):
        if d in lossy:
            assert st == L.DG_OK, i
            _same(arr, refs(d), "lossy member %d" % i)
        elif d in cuts:
            r = R.decode(d)
            if r.status == R.OK:  # the cut took only bytes no reader needed
                _same(arr, np.frombuffer(r.rgb, np.uint8).reshape(r.height, r.width, 3), "cut %d" % i)
            else:
                assert st == L.DG_ERR_CORRUPT and arr is None, (i, st)
                corrupt += 1
        elif d is not jpg:
            assert st == L.DG_OK and np.array_equal(arr, alone[id(d)][1]), i
    assert corrupt >= 12
    assert res[0][0] == L.DG_OK and res[-1][0] == L.DG_OK and np.array_equal(res[0][1], res[-1][1])
    assert np.array_equal(res[0][1], ctx.decode_batch([jpg])[0][1])


def test_seventy_of_one_file_in_one_batch(ctxs, refs):
    L = _lib()
    d = dict(PILLOW)["photo_40x36"]
    res = ctxs().decode_batch([d] * 70)  # more images than a wave has lanes, more than one list chunk
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
        assert (m.bucket, m.width, m.height, m.channels, m.bit_depth) == (tm.bucket, tm.width, tm.height, 3, 8), i
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
    _same(host[1][1], _transformed(refs(files[1])), "the extended lossy WebP")
    _same(host[3][1], _transformed(refs(files[3])), "the simple lossy WebP")


def test_sample_alignment_with_a_lossy_member(refs, downstream):
    """An extended lossy WebP under the reference member's name decides the sample's bucket (dg_probe reads its
    VP8X canvas); a simple lossy file stays unknown to dg_probe, so it is skipped as the reference, as before."""
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    from datago_amd.samples import BinaryFile, TarballSample, process_sample
    L = _lib()
    tfm = ARAwareTransform(ImageTransformConfig(True, CFG[0], CFG[1], CFG[2], CFG[3]), 0, webp_lossy=True)
    webp = downstream[1]
    px = refs(webp)
    mask = synth.make_png(81, px.shape[1], px.shape[0] - 10, "L")
    s = TarballSample("shard-0.tar", [BinaryFile("k1.jpg", webp), BinaryFile("k1.png", mask)])
    out = process_sample(s, tfm, ImageEncoding(), "jpg")
    assert out is not None and not out.unsupported
    t = B.ARAwareTransform(*CFG)
    target = t.target_size(px.shape[1], px.shape[0])
    assert (out.image.width, out.image.height, out.image.channels) == target + (3,)
    assert (out.image.original_width, out.image.original_height) == (px.shape[1], px.shape[0])
    assert np.frombuffer(out.image.data, np.uint8).tobytes() == _transformed(px).tobytes()
    m = out.additional_images["k1.png"]
    _, dec = O.decode_any(mask)
    assert (m.width, m.height) == target
    assert np.frombuffer(m.data, np.uint8).tobytes() == O.crop_and_resize(dec, target[0], target[1], O.MODE_FIR).tobytes()
    table = tfm.table
    assert L.sample_align(table, [webp, mask])[1] >= 0 and L.sample_align(table, [downstream[0], mask]) == [-1, -1]
