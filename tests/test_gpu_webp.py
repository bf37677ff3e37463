"""Lossless WebP on the GPU behind context option "webp" (dg_vp8l.hip): bit-exact
against tests/ref_webp.py (pinned to Pillow in test_webp_cpu.py), and past the
decode against the oracle's result for the RGB / RGBA PNG twin of the same
pixels.  Covers the option, every Pillow-made and crafted file of webp_cases.py,
the refusals through the library with their texts, truncations beside an intact
neighbour and everything downstream of the decode, where a lossless WebP is an
8-bit PNG's pixels of colour type 2 or 6."""
import io

import numpy as np
import pytest
from PIL import Image

import ref_webp as R
import webp_cases as K
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CFG = (224, 16, 0.5, 2.0)
PILLOW = K.pillow_cases()
CRAFTED = K.crafted_cases()


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (resize, webp, options), made once per module."""
    cache = {}

    def get(resize=False, webp=True, **extra):
        key = (resize, webp, tuple(sorted(extra.items())))
        if key not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if resize else {}
            cache[key] = _lib().Context(0, webp=webp, **kw, **extra)
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


@pytest.fixture(scope="module")
def refs():
    """ref_webp's pixels of a file, computed once."""
    cache = {}

    def get(data):
        if data not in cache:
            r = R.decode(data)
            assert r.status == "OK", r.why
            cache[data] = r.pixels
        return cache[data]
    return get


def _save(a):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "WEBP", lossless=True, exact=True, method=3, quality=50)
    return b.getvalue()


@pytest.fixture(scope="module")
def downstream():
    """Files for everything past the decode: RGB and RGBA (alpha 0 over non-zero RGB), gray, one of its bucket's
    size and one a column wider than a bucket (an x.5 crop)."""
    t = B.ARAwareTransform(*CFG)
    bw, bh = t.target_size(300, 200)
    assert t.target_size(bw + 1, bh) == (bw, bh) and t.target_size(bw, bh) == (bw, bh)
    rng = np.random.default_rng(61)

    def rgba(h, w):
        a = np.concatenate([K._photo(rng, h, w), rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)
        a[h // 4:h // 2, w // 4:w // 2, 3] = 0
        return a
    return [_save(K._photo(rng, 200, 300)), _save(rgba(330, 260)), _save(np.repeat(K._photo(rng, 67, 131)[..., :1], 3, -1)),
            _save(rgba(bh, bw)), _save(K._photo(rng, bh, bw + 1))]


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

def test_option_off_is_corrupt_as_before(ctxs):
    L = _lib()
    ctx = ctxs(webp=False)
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    files = [d for _, d in PILLOW[:4] + CRAFTED[:3]]
    res = ctx.decode_batch([jpg] + files + [jpg])
    assert res[0][0] == L.DG_OK and res[-1][0] == L.DG_OK and np.array_equal(res[0][1], res[-1][1])
    for d, (st, arr, m) in zip(files, res[1:-1]):
        assert st == L.DG_ERR_CORRUPT and arr is None
        assert ctx.output_size(d)[0] == L.DG_ERR_CORRUPT
        st, info = L.probe(d)  # dg_probe names it, and describes the default options
        assert st == L.DG_OK and info.format == L.DG_FMT_WEBP and info.gpu_supported == 0
    assert L.Context(0).output_size(files[0])[0] == L.DG_ERR_CORRUPT  # the default of a plain context


def test_option_values():
    L = _lib()
    ctx = L.Context(0)
    data = dict(PILLOW)["rgba_130x64"]
    r = R.decode(data)
    ctx.set_option("webp", 1)
    assert ctx.output_size(data) == (L.DG_OK, r.pixels.size)
    ctx.set_option("webp", 0)
    assert ctx.output_size(data)[0] == L.DG_ERR_CORRUPT
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("webp", bad)
        assert e.value.status == L.DG_ERR_INVALID and "webp" in L.last_error()
    assert ctx.output_size(data)[0] == L.DG_ERR_CORRUPT  # a refused value changes nothing
    ctx.set_option("webp", 1)  # a simple lossy file stays an unknown format with the option on
    assert ctx.output_size(K.SIMPLE_LOSSY)[0] == L.DG_ERR_CORRUPT
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
        assert (m.channels, m.bit_depth, m.is_encoded) == (ref.shape[2], 8, 0), label


def test_each_file_alone_and_through_decode_one(ctxs, refs):
    L = _lib()
    ctx = ctxs()
    for label, d in PILLOW + CRAFTED:
        (st, arr, m), = ctx.decode_batch([d])
        assert st == L.DG_OK, label
        _same(arr, refs(d), label)
    for label, d in PILLOW + CRAFTED:
        st, arr, m = ctx.decode_one(d)
        assert st == L.DG_OK and (m.channels, m.bit_depth) == (refs(d).shape[2], 8), label
        _same(arr, refs(d), label)


def test_refusals_through_the_library(ctxs, refs):
    L = _lib()
    ctx = ctxs()
    good = dict(PILLOW)["mixed_129x63_m3_q0"]
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    (_, jref, _), = ctx.decode_batch([jpg])
    refused = K.refusals()
    res = ctx.decode_batch([good] + [d for _, d, _, _ in refused] + [good, jpg])
    for (label, d, status, text), (st, arr, m) in zip(refused, res[1:]):
        want = L.DG_ERR_UNSUPPORTED if status == "UNSUPPORTED" else L.DG_ERR_CORRUPT
        assert st == want and arr is None, (label, st)
    for st, arr, m in (res[0], res[-2]):  # the other members of the batch stay exact
        assert st == L.DG_OK
        _same(arr, refs(good), "good beside refused")
    assert res[-1][0] == L.DG_OK and np.array_equal(res[-1][1], jref)
    stream = (R.E_BITS, R.E_CODE, R.E_COPY, R.E_CACHE, R.E_TRANSFORM, R.E_GROUPS)
    for label, d, status, text in refused:  # each names itself: the header's at planning, the stream's at completion
        want = L.DG_ERR_UNSUPPORTED if status == "UNSUPPORTED" else L.DG_ERR_CORRUPT
        if text in stream:
            assert ctx.output_size(d)[0] == L.DG_OK, label
            (st, arr, m), = ctx.decode_batch([d])
        else:
            st = ctx.output_size(d)[0]
        assert st == want and text in L.last_error(), (label, st, L.last_error())
    (st, arr, m), = ctx.decode_batch([K.SIMPLE_LOSSY])
    assert st == L.DG_ERR_CORRUPT


def test_sixteen_truncations_beside_an_intact_neighbour(ctxs, refs):
    L = _lib()
    data = dict(PILLOW)["mixed_129x63_m3_q0"]
    f = R.parse(data)
    cuts = []
    for k in range(16):
        n = f["data_off"] + 1 + k * (len(data) - f["data_off"] - 2) // 15
        cut = bytearray(data[:n])  # the sizes made to fit, so the bitstream itself ends early
        cut[4:8] = (n - 8).to_bytes(4, "little")
        cut[f["data_off"] - 9:f["data_off"] - 5] = (n - f["data_off"] + 5).to_bytes(4, "little")
        cuts.append(bytes(cut))
    res = ctxs().decode_batch([data] + cuts + [data])
    corrupt = 0
    for cut, (st, arr, m) in zip(cuts, res[1:-1]):
        r = R.decode(cut)  # (a cut inside the last byte's padding bits still decodes)
        if r.status == "OK":
            assert st == L.DG_OK, len(cut)
            _same(arr, r.pixels, "cut at %d" % len(cut))
        else:
            assert r.status == "CORRUPT" and st == L.DG_ERR_CORRUPT and arr is None, (len(cut), st, r.status)
            corrupt += 1
    assert corrupt >= 14
    for st, arr, m in (res[0], res[-1]):
        assert st == L.DG_OK
        _same(arr, refs(data), "intact beside truncated")


# ------------------------------------------------------------------ downstream of the decode

def test_resized_and_cropped_as_the_png_twin(ctxs, refs, downstream):
    L = _lib()
    ctx = ctxs(resize=True)
    res = ctx.decode_batch(downstream)
    twins = ctx.decode_batch([_twin(refs(d)) for d in downstream])
    assert {refs(d).shape[2] for d in downstream} == {3, 4}  # colour types 2 and 6
    for i, (d, (st, arr, m), (tst, tarr, tm)) in enumerate(zip(downstream, res, twins)):
        assert st == L.DG_OK and tst == L.DG_OK, (i, st)
        exp = _transformed(refs(d))
        _same(arr, exp, "file %d" % i)
        _same(tarr, exp, "twin %d" % i)
        assert (m.bucket, m.width, m.height, m.channels, m.bit_depth) == (tm.bucket, tm.width, tm.height, refs(d).shape[2], 8), i
        assert (m.original_width, m.original_height) == (refs(d).shape[1], refs(d).shape[0]), i


@pytest.mark.parametrize("resize", [False, True], ids=["decode", "resize"])
def test_image_to_rgb8_blends_over_gray(ctxs, refs, downstream, resize):
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


def test_mixed_submission_host_and_device(ctxs, refs, downstream):
    import gif_cases
    L = _lib()
    ctx = ctxs(resize=True, gif=True)
    webp = downstream[1]
    files = [synth.make_jpeg(71, 300, 200, 90), synth.make_png(72, 150, 260, "RGBA"), webp,
             dict(gif_cases.stream_cases())["photo 131x67"], downstream[0]]
    alone = [ctx.decode_batch([f])[0] for f in files]
    host = ctx.decode_batch(files)
    dev = ctx.decode_batch_torch(files)
    for i, ((st, arr, m), (hst, harr, hm), (dst, darr, dm)) in enumerate(zip(alone, host, dev)):
        assert st == hst == dst == L.DG_OK, i
        assert np.array_equal(arr, harr) and np.array_equal(arr, darr.cpu().numpy()), i
    _same(host[2][1], _transformed(refs(webp)), "the RGBA WebP of the mixed batch")
    _same(host[4][1], _transformed(refs(files[4])), "the RGB WebP of the mixed batch")


def test_one_batch_under_a_device_budget(ctxs, refs, downstream):
    L = _lib()
    files = downstream + [d for _, d in PILLOW[::5] + CRAFTED[::5]]
    c = L.Context(0, webp=True, crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                  min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3])
    c.set_option("max_device_mb", 1 << 20)
    res = c.decode_batch(files)
    assert c.stat("peak_device_mb") > 0
    for i, (d, (st, arr, m)) in enumerate(zip(files, res)):
        assert st == L.DG_OK, i
        _same(arr, _transformed(refs(d)), "file %d" % i)
    c.close()


def test_both_decode_semantics(refs):
    L = _lib()
    cases = PILLOW[::7] + CRAFTED[::3]
    for sem in (0, 1):
        c = L.Context(0, webp=True, decode_semantics=sem)
        for (label, d), (st, arr, m) in zip(cases, c.decode_batch([d for _, d in cases])):
            assert st == L.DG_OK, (sem, label)
            _same(arr, refs(d), label)
        c.close()


def test_sample_alignment_with_a_webp_reference(refs, downstream):
    """load_from_memory sniffs the content: a WebP under the reference member's name decides the sample's bucket."""
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    from datago_amd.samples import BinaryFile, TarballSample, process_sample
    tfm = ARAwareTransform(ImageTransformConfig(True, CFG[0], CFG[1], CFG[2], CFG[3]), 0, webp=True)
    webp = downstream[0]
    mask = synth.make_png(81, 300, 190, "L")
    s = TarballSample("shard-0.tar", [BinaryFile("k1.jpg", webp), BinaryFile("k1.png", mask)])
    out = process_sample(s, tfm, ImageEncoding(), "jpg")
    assert out is not None and not out.unsupported
    t = B.ARAwareTransform(*CFG)
    target = t.target_size(300, 200)
    assert (out.image.width, out.image.height, out.image.channels) == target + (3,)
    assert (out.image.original_width, out.image.original_height) == (300, 200)
    assert np.frombuffer(out.image.data, np.uint8).tobytes() == _transformed(refs(webp)).tobytes()
    m = out.additional_images["k1.png"]
    _, dec = O.decode_any(mask)
    assert (m.width, m.height) == target
    assert np.frombuffer(m.data, np.uint8).tobytes() == O.crop_and_resize(dec, target[0], target[1], O.MODE_FIR).tobytes()
    # without the option the WebP member fails to load and is skipped: the mask is its own reference
    off = process_sample(s, ARAwareTransform(ImageTransformConfig(True, CFG[0], CFG[1], CFG[2], CFG[3]), 0),
                         ImageEncoding(), "jpg")
    assert off is not None and off.image.width == 0 and "k1.png" in off.additional_images
