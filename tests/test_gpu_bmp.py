"""Windows bitmaps on the GPU behind context option "bmp" (dg_bmp.hip):
bit-exact against tests/ref_bmp.py (pinned to Pillow in test_bmp_cpu.py), and
past the decode against the oracle's result for the PNG twin of the same
pixels.  Covers the option, every uncompressed form at every width phase and
data alignment, the RLE cases (runs, absolute blocks across step windows, hop
loops, stream ends), the refusals through the library and everything
downstream of the decode, where a BMP is an 8-bit RGB / RGBA PNG's pixels."""
import io

import numpy as np
import pytest
from PIL import Image

import bmp_cases as C
import bmp_craft as G
import gif_cases as GC
import gif_craft as GG
import ref_bmp as R
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CFG = (224, 16, 0.5, 2.0)


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (resize, bmp, options), made once per module."""
    cache = {}

    def get(resize=False, bmp=True, opts=(), **extra):
        key = (resize, bmp, tuple(opts), tuple(sorted(extra.items())))
        if key not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if resize else {}
            cache[key] = _lib().Context(0, bmp=bmp, **kw, **extra)
            for k, v in opts:
                cache[key].set_option(k, v)
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


@pytest.fixture(scope="module")
def refs():
    """ref_bmp's decode of a file, computed once."""
    cache = {}

    def get(data):
        if data not in cache:
            st, why, pix, h = R.decode(data)
            assert st == R.OK, why
            cache[data] = pix
        return cache[data]
    return get


@pytest.fixture(scope="module")
def downstream():
    """Files for everything past the decode: an RGB and an RGBA file, an RLE8 and a 4-bit one, one of its bucket's
    size and one a column wider than a bucket (an x.5 crop), for RGB and for RGBA."""
    t = B.ARAwareTransform(*CFG)
    bw, bh = t.target_size(300, 200)
    assert t.target_size(bw + 1, bh) == (bw, bh) and t.target_size(bw, bh) == (bw, bh)
    ph = C.photo(150, 200, 256, 63)
    bf = dict(compression=G.BITFIELDS, masks=G.MASKS32[5], header=108)
    out = [G.bmp(300, 200, 24, C.rgb(200, 300, 61)),
           G.bmp(260, 330, 32, C.rgb(330, 260, 62, 4), top_down=True, **bf),
           G.bmp(200, 150, 8, data=G.rle_bytes(G.rle_commands(ph, False, "mixed")), compression=G.RLE8,
                 pal=G.palette(256, 64)),
           G.bmp(131, 67, 4, C.noise(67, 131, 16, 65), pal=G.palette(16, 66)),
           G.bmp(bw, bh, 24, C.rgb(bh, bw, 67)),
           G.bmp(bw + 1, bh, 24, C.rgb(bh, bw + 1, 68), top_down=True),
           G.bmp(bw, bh, 32, C.rgb(bh, bw, 69, 4), **bf),
           G.bmp(bw + 1, bh, 32, C.rgb(bh, bw + 1, 70, 4), **bf)]
    return out


def _same(arr, ref, label):
    assert arr is not None and tuple(arr.shape[:2]) == tuple(ref.shape[:2]), label
    got = np.asarray(arr).reshape(ref.shape)
    assert np.array_equal(got, ref), (label, int((got != ref).sum()))


def _twin(pix):
    return synth.pil_png(pix)


def _transformed(pix, to_rgb8=False):
    """The oracle's result for these RGB / RGBA pixels in the CFG buckets."""
    t = B.ARAwareTransform(*CFG)
    tw, th = t.target_size(pix.shape[1], pix.shape[0])
    resized = (tw, th) != (pix.shape[1], pix.shape[0])
    out = O.crop_and_resize(pix, tw, th, O.MODE_FIR) if resized else pix
    return O.to_rgb8(out, resized) if to_rgb8 else out


# ------------------------------------------------------------------ the option

def test_option_off_is_corrupt_as_before(ctxs):
    L = _lib()
    ctx = ctxs(bmp=False)
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    files = [c[1] for c in C.pixel_cases()[:4] + C.rle_cases()[:3]]
    res = ctx.decode_batch([jpg] + files + [jpg])
    assert res[0][0] == L.DG_OK and res[-1][0] == L.DG_OK and np.array_equal(res[0][1], res[-1][1])
    for d, (st, arr, m) in zip(files, res[1:-1]):
        assert st == L.DG_ERR_CORRUPT and arr is None
        assert ctx.output_size(d)[0] == L.DG_ERR_CORRUPT
        st, info = L.probe(d)  # dg_probe names it, and describes the default options
        assert st == L.DG_OK and info.format == L.DG_FMT_BMP and info.gpu_supported == 0 and info.components == 3
    assert L.Context(0).output_size(files[0])[0] == L.DG_ERR_CORRUPT  # the default of a plain context


def test_option_values():
    L = _lib()
    ctx = L.Context(0)
    data = dict((c[0], c[1]) for c in C.pixel_cases())["24 131x67"]
    ctx.set_option("bmp", 1)
    assert ctx.output_size(data) == (L.DG_OK, 131 * 67 * 3)
    ctx.set_option("bmp", 0)
    assert ctx.output_size(data)[0] == L.DG_ERR_CORRUPT
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("bmp", bad)
        assert e.value.status == L.DG_ERR_INVALID and "bmp" in L.last_error()
    assert ctx.output_size(data)[0] == L.DG_ERR_CORRUPT  # a refused value changes nothing
    ctx.close()


# ------------------------------------------------------------------ decode

@pytest.mark.parametrize("which", ["pixels", "rle"])
def test_decode_bit_exact_in_one_batch(ctxs, refs, which):
    L = _lib()
    cases = C.pixel_cases() if which == "pixels" else C.rle_cases()
    res = ctxs().decode_batch([c[1] for c in cases])
    for (label, d, _, _), (st, arr, m) in zip(cases, res):
        assert st == L.DG_OK, (label, st, L.last_error())
        ref = refs(d)
        _same(arr, ref, label)
        assert (m.original_width, m.original_height, m.width, m.height) == (ref.shape[1], ref.shape[0]) * 2, label
        assert (m.channels, m.bit_depth, m.is_encoded) == (ref.shape[2], 8, 0), label


def test_each_file_alone_and_through_decode_one(ctxs, refs):
    L = _lib()
    ctx = ctxs()
    by = dict((c[0], c[1]) for c in C.pixel_cases() + C.rle_cases())
    picks = ["1-bit 1x3 bottom-up", "24 300x200 top-down", "bf32:3 131x67", "4 131x67", "RLE8 300x200 photo",
             "RLE4 510x2 run 255 and absolute 254", "RLE8 odd bfOffBits, absolute odd", "RLE4 131x3 absolute odd"]
    for label in picks:
        d = by[label]
        (st, arr, m), = ctx.decode_batch([d])
        assert st == L.DG_OK, label
        _same(arr, refs(d), label)
        st, arr, m = ctx.decode_one(d)
        assert st == L.DG_OK and (m.channels, m.bit_depth) == (refs(d).shape[2], 8), label
        _same(arr, refs(d), label)


def test_refusals_through_the_library(ctxs, refs):
    L = _lib()
    ctx = ctxs()
    good = dict((c[0], c[1]) for c in C.rle_cases())["RLE8 131x67 noise"]
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    (_, jref, _), = ctx.decode_batch([jpg])
    refused = C.refusals()
    res = ctx.decode_batch([good] + [d for _, d, _, _ in refused] + [good, jpg])
    for (label, d, status, text), (st, arr, m) in zip(refused, res[1:]):
        want = L.DG_ERR_UNSUPPORTED if status == R.UNSUPPORTED else L.DG_ERR_CORRUPT
        assert st == want and arr is None, (label, st)
    for st, arr, m in (res[0], res[-2]):  # the other members of the batch stay exact
        assert st == L.DG_OK
        _same(arr, refs(good), "good beside refused")
    assert res[-1][0] == L.DG_OK and np.array_equal(res[-1][1], jref)
    for label, d, status, text in refused:  # each names itself: the header's at planning, the stream's at completion
        want = L.DG_ERR_UNSUPPORTED if status == R.UNSUPPORTED else L.DG_ERR_CORRUPT
        if text in R.STREAM_TEXTS:
            assert ctx.output_size(d)[0] == L.DG_OK, label
            (st, arr, m), = ctx.decode_batch([d])
        else:
            st = ctx.output_size(d)[0]
        assert st == want and text in L.last_error(), (label, st, L.last_error())


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
        c = refs(d).shape[2]
        assert (m.bucket, m.width, m.height, m.channels, m.bit_depth) == (tm.bucket, tm.width, tm.height, c, 8), i
        assert (m.original_width, m.original_height) == (refs(d).shape[1], refs(d).shape[0]), i
    assert {refs(d).shape[2] for d in downstream} == {3, 4}


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


def test_mixed_submission_host_and_device(ctxs, refs, downstream):
    L = _lib()
    kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1], min_aspect_ratio=CFG[2],
              max_aspect_ratio=CFG[3])
    ctx = L.Context(0, bmp=True, gif=True, **kw)
    gif = GG.gif(131, 67, GC.photo(67, 131, 32, 64), 5, gct=GG.palette(32, 61))
    files = [synth.make_jpeg(71, 300, 200, 90), synth.make_png(72, 150, 260, "RGBA"), gif, downstream[1],
             synth.make_jpeg(73, 200, 300, 90, progressive=True), downstream[2], downstream[0]]
    alone = [ctx.decode_batch([f])[0] for f in files]
    host = ctx.decode_batch(files)
    dev = ctx.decode_batch_torch(files)
    for i, ((st, arr, m), (hst, harr, hm), (dst, darr, dm)) in enumerate(zip(alone, host, dev)):
        assert st == hst == dst == L.DG_OK, i
        assert np.array_equal(arr, harr) and np.array_equal(arr, darr.cpu().numpy()), i
    _same(host[3][1], _transformed(refs(files[3])), "the RGBA BMP of the mixed batch")
    _same(host[5][1], _transformed(refs(files[5])), "the RLE8 BMP of the mixed batch")
    _same(host[6][1], _transformed(refs(files[6])), "the 24-bit BMP of the mixed batch")
    ctx.close()


def test_one_batch_under_a_device_budget(ctxs, refs, downstream):
    L = _lib()
    files = downstream + [c[1] for c in C.rle_cases()[::3]] + [c[1] for c in C.pixel_cases()[::7]]
    c = L.Context(0, bmp=True, crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
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
    cases = C.rle_cases()[::2] + C.pixel_cases()[::5]
    for sem in (0, 1):
        c = L.Context(0, bmp=True, decode_semantics=sem)
        for (label, d, _, _), (st, arr, m) in zip(cases, c.decode_batch([x[1] for x in cases])):
            assert st == L.DG_OK, (sem, label)
            _same(arr, refs(d), label)
        c.close()


def test_sample_alignment_with_a_bmp_reference(refs, downstream):
    """load_from_memory sniffs the content: a BMP under the reference member's name decides the sample's bucket."""
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    from datago_amd.samples import BinaryFile, TarballSample, process_sample
    tfm = ARAwareTransform(ImageTransformConfig(True, CFG[0], CFG[1], CFG[2], CFG[3]), 0, bmp=True)
    bmp = downstream[0]
    mask = synth.make_png(81, 300, 190, "L")
    s = TarballSample("shard-0.tar", [BinaryFile("k1.jpg", bmp), BinaryFile("k1.png", mask)])
    out = process_sample(s, tfm, ImageEncoding(), "jpg")
    assert out is not None and not out.unsupported
    t = B.ARAwareTransform(*CFG)
    target = t.target_size(300, 200)
    assert (out.image.width, out.image.height, out.image.channels) == target + (3,)
    assert (out.image.original_width, out.image.original_height) == (300, 200)
    assert np.frombuffer(out.image.data, np.uint8).tobytes() == _transformed(refs(bmp)).tobytes()
    m = out.additional_images["k1.png"]
    _, dec = O.decode_any(mask)
    assert (m.width, m.height) == target
    assert np.frombuffer(m.data, np.uint8).tobytes() == O.crop_and_resize(dec, target[0], target[1], O.MODE_FIR).tobytes()
    # without the option the BMP member fails to load and is skipped: the mask is its own reference
    off = process_sample(s, ARAwareTransform(ImageTransformConfig(True, CFG[0], CFG[1], CFG[2], CFG[3]), 0),
                         ImageEncoding(), "jpg")
    assert off is not None and off.image.width == 0 and "k1.png" in off.additional_images
