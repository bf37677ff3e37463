"""TIFF files on the GPU behind context option "tiff" (dg_tiff.hip): bit-exact against Pillow (libtiff), whose decode
of every file is itself compared with the array the file was made from, and past the decode against the oracle's
result for the PNG twin of the same pixels.  tiff_craft.cases says why the stream that never clears comes in strips."""
import io

import numpy as np
import pytest
from PIL import Image

import tiff_craft as T
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CFG = (224, 16, 0.5, 2.0)
RESIZE = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1], min_aspect_ratio=CFG[2],
              max_aspect_ratio=CFG[3])
CASES = T.cases()
GROUPS = ["lzw", "packbits", "pred", "tiles", "other"]


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ctx():
    c = _lib().Context(0, tiff=True)
    yield c
    c.close()


def _check(L, files, res):
    for (label, data, pix), (st, arr, m) in zip(files, res):
        assert st == L.DG_OK, (label, st, L.last_error())
        ref = np.asarray(Image.open(io.BytesIO(data)))  # Pillow's decode, which must be what the file was made from
        assert np.array_equal(ref, pix), label
        ref = ref.reshape(ref.shape[0], ref.shape[1], -1)
        got = np.asarray(arr).reshape(ref.shape)
        assert np.array_equal(got, ref), (label, int((got != ref).sum()))
        assert (m.original_width, m.original_height, m.width, m.height) == (ref.shape[1], ref.shape[0]) * 2, label
        assert (m.channels, m.bit_depth, m.is_encoded) == (ref.shape[2], 8, 0), label


def _written(mode, comp, pred, w=97, h=70, seed=7):
    pix = np.random.default_rng(seed).integers(0, 256, (h, w, len(mode)), dtype=np.uint8)
    pix[h // 4:h // 2] = pix[0, 0]  # something for PackBits and LZW to find
    pix = pix[:, :, 0] if mode == "L" else pix
    out = io.BytesIO()
    Image.fromarray(pix).save(out, "TIFF", compression=comp, **({"tiffinfo": {317: 2}} if pred else {}))
    return ("Pillow %s %s%s" % (mode, comp, " pred" if pred else ""), out.getvalue(), pix)


def test_option_off_is_corrupt_and_on_decodes(ctx):
    L = _lib()
    label, data, pix = CASES[0]
    off = L.Context(0)
    assert off.output_size(data)[0] == L.DG_ERR_CORRUPT and off.decode_batch([data])[0][0] == L.DG_ERR_CORRUPT
    st, info = L.probe(data)  # dg_probe names it either way, and describes the default options
    assert st == L.DG_OK and (info.format, info.width, info.height, info.components, info.gpu_supported) == (6, 97, 70, 3, 0)
    off.set_option("tiff", 1)
    assert off.output_size(data) == (L.DG_OK, pix.size)
    _check(L, [CASES[0]], off.decode_batch([data]))
    off.close()


@pytest.mark.parametrize("group", GROUPS)
def test_crafted_files_bit_exact_in_one_batch(ctx, group):
    files = [c for c in CASES if (c[0].split()[0] if c[0].split()[0] in GROUPS else "other") == group]
    assert len(files) >= 3
    _check(_lib(), files, ctx.decode_batch([c[1] for c in files]))


@pytest.mark.parametrize("comp,pred", [("raw", 0), ("packbits", 0), ("tiff_lzw", 0), ("tiff_lzw", 1)])
def test_pillow_written_files(ctx, comp, pred):
    files = [_written(mode, comp, pred) for mode in ("L", "LA", "RGB", "RGBA")]
    _check(_lib(), files, ctx.decode_batch([c[1] for c in files]))


def test_eight_images_with_different_segment_counts(ctx):
    pix = [T.noise(70, 97, 3, 20 + k) for k in range(8)]
    files = [("rps %d" % rps, T.tiff(p, comp=5, pred=2, rps=rps, pack=lambda d, k=k: T.lzw(d, end=k % 2 == 0)), p)
             for k, (rps, p) in enumerate(zip((1, 2, 3, 5, 7, 16, 35, 70), pix))]
    _check(_lib(), files, ctx.decode_batch([c[1] for c in files]))
    _check(_lib(), files[::3], [ctx.decode_one(c[1]) for c in files[::3]])  # and alone, through decode_one


@pytest.mark.parametrize("mode", ["RGB", "RGBA"])
def test_downstream_as_the_png_twin(mode):
    """Resize to a bucket, and the PNG re-encode, equal the oracle's result for the PNG twin of the same pixels."""
    L = _lib()
    label, data, pix = _written(mode, "tiff_lzw", 1, 300, 200, 11)
    t = B.ARAwareTransform(*CFG)
    tw, th = t.target_size(300, 200)
    exp = O.crop_and_resize(pix, tw, th, O.MODE_FIR)
    c = L.Context(0, tiff=True, **RESIZE)
    (st, arr, m), (tst, tarr, tm) = c.decode_batch([data, synth.pil_png(pix)])
    assert st == tst == L.DG_OK and (m.bucket, m.width, m.height, m.channels) == (tm.bucket, tw, th, len(mode))
    assert np.array_equal(np.asarray(arr).reshape(exp.shape), exp) and np.array_equal(np.asarray(tarr).reshape(exp.shape), exp)
    c.close()
    c = L.Context(0, tiff=True, pre_encode_images=True, encode_format=0, **RESIZE)
    (st, buf, m), (tst, tbuf, tm) = c.decode_batch([data, synth.pil_png(pix)])
    assert st == tst == L.DG_OK and m.is_encoded == 1 and buf.tobytes() == tbuf.tobytes()
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(buf.tobytes()))), exp)
    c.close()


def test_refusals_and_the_good_files_beside_them(ctx):
    L = _lib()
    good, refused = CASES[4], T.refusals()
    res = ctx.decode_batch([good[1]] + [d for _, d, _ in refused] + [good[1]])
    for (label, d, corrupt), (st, arr, m) in zip(refused, res[1:-1]):
        assert st == (L.DG_ERR_CORRUPT if corrupt else L.DG_ERR_UNSUPPORTED) and arr is None, (label, st)
    _check(L, [good, good], [res[0], res[-1]])
    for label, d, corrupt in refused:  # each names itself: the header's at planning, the stream's at completion
        st = ctx.output_size(d)[0]
        if label.startswith("stream"):
            assert st == L.DG_OK, label
            st = ctx.decode_batch([d])[0][0]
        assert st == (L.DG_ERR_CORRUPT if corrupt else L.DG_ERR_UNSUPPORTED) and L.last_error().startswith("TIFF: "), (label, st)
        assert "stays full" in L.last_error() or "stays full" not in label, label
