"""16-bit TIFFs on the GPU behind context option "tiff16" (k_tiff_expand16, dg_tiff.hip): bit-exact against the uint16
array each file was made from, against Pillow (libtiff) where it holds the form (gray exactly, the high bytes of RGB
and RGBA), and past the decode against the 16-bit PNG twin of the same pixels."""
import io

import numpy as np
import pytest
from PIL import Image

import tiff16_craft as S
import tiff_craft as T
from datago_amd import synth
from test_gpu_tiff import RESIZE, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib().Context(0, tiff=True, tiff16=True, tiff_deflate=True)
    yield c
    c.close()


def _check(L, files, res):
    for (label, data, pix), (st, arr, m) in zip(files, res):
        assert st == L.DG_OK, (label, st, L.last_error())
        ref = pix.reshape(pix.shape[0], pix.shape[1], -1)
        if ref.shape[2] != 2:  # Pillow does not open gray + alpha; it holds 16-bit gray, and 8 bits of 16-bit colour
            pil = np.asarray(Image.open(io.BytesIO(data)))
            assert np.array_equal(pil, pix if pix.ndim == 2 else pix >> 8), label
        got = np.asarray(arr).reshape(ref.shape)
        assert got.dtype == np.uint16 and np.array_equal(got, ref), (label, int((got != ref).sum()))
        assert (m.original_width, m.original_height, m.width, m.height, m.channels, m.bit_depth, m.is_encoded) == \
               (ref.shape[1], ref.shape[0]) * 2 + (ref.shape[2], 16, 0), label


def test_option_gates():
    L = _lib()
    old = dict((r[0], r[1]) for r in T.refusals())["16-bit"]
    label, data, pix = S.tiff16("gray16", S.noise16(70, 97, 1, 1), comp=5, pred=2)
    c = L.Context(0, tiff=True)
    assert c.output_size(old)[0] == L.DG_ERR_UNSUPPORTED and c.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    c.set_option("tiff16", 1)
    assert c.output_size(data) == (L.DG_OK, 2 * pix.size)
    _check(L, [(label, data, pix)], c.decode_batch([data]))
    c.close()
    c = L.Context(0, tiff16=True)
    assert c.output_size(data)[0] == L.DG_ERR_CORRUPT and c.decode_batch([data])[0][0] == L.DG_ERR_CORRUPT
    c.close()


@pytest.mark.parametrize("be", [False, True], ids=["II", "MM"])
@pytest.mark.parametrize("spp", [1, 2, 3, 4])
def test_predictor_at_lane_wave_and_trip_edges(ctx, spp, be):
    files = [S.tiff16("pred %dx3x%d" % (w, spp), S.noise16(3, w, spp, 10 * w + spp), be=be, comp=5, pred=2)
             for w in (1, 63, 64, 65, 129, 257)]
    _check(_lib(), files, ctx.decode_batch([f[1] for f in files]))


@pytest.mark.parametrize("group", ["raw", "packbits", "lzw", "tiles", "other"])
def test_forms_bit_exact_in_one_batch(ctx, group):
    files = [c for c in S.forms() if (c[0].split()[0] if c[0].split()[0] in ("raw", "lzw", "tiles") else
                                      "packbits" if "packbits" in c[0] else "other") == group]
    assert len(files) >= 2
    _check(_lib(), files, ctx.decode_batch([c[1] for c in files]))


@pytest.mark.parametrize("c,ctype", [(1, 0), (3, 2)])
def test_downstream_as_the_16_bit_png_twin(c, ctype):
    L = _lib()
    pix = S.noise16(200, 300, c, 11).reshape(200, 300, c)
    data, twin = S.tiff16("", pix, comp=5, pred=2, rps=16, be=True)[1], synth.encode_png16(pix, ctype, np.random.default_rng(5))
    opts = dict(tiff=True, tiff16=True, png16=True, **RESIZE)
    for kw, enc in [(dict(resize16=True), 0), (dict(resize16=True, image_to_rgb8=True), 0),
                    (dict(resize16=True, penc16=True, penc_dynamic=True, pre_encode_images=True, encode_format=0), 1)]:
        ctx = L.Context(0, **opts, **kw)
        (st, arr, m), (tst, tarr, tm) = ctx.decode_batch([data, twin])
        assert st == tst == L.DG_OK, (kw, st, tst, L.last_error())
        assert (m.bucket, m.width, m.height, m.channels, m.bit_depth, m.is_encoded) == \
               (tm.bucket, tm.width, tm.height, tm.channels, tm.bit_depth, enc), kw
        assert arr.tobytes() == tarr.tobytes() and len(arr.tobytes()) > 0, kw
        ctx.close()
    ctx = L.Context(0, **opts)  # without resize16 only a 16-bit image of its bucket's size decodes
    assert ctx.decode_batch([data])[0][0] == L.DG_ERR_UNSUPPORTED and L.last_error().startswith("TIFF: "), L.last_error()
    ctx.close()


def test_refusals_and_the_good_files_beside_them(ctx):
    L = _lib()
    good, refused = S.tiff16("good", S.noise16(8, 20, 3, 6), comp=5, pred=2, be=True), S.refusals()
    res = ctx.decode_batch([good[1]] + [d for _, d, _ in refused] + [good[1]])
    _check(L, [good, good], [res[0], res[-1]])
    for (label, d, corrupt), (st, arr, m) in zip(refused, res[1:-1]):
        want = L.DG_ERR_CORRUPT if corrupt else L.DG_ERR_UNSUPPORTED
        assert st == want and arr is None, (label, st)
        st = ctx.output_size(d)[0]  # each names itself: the header's at planning, the stream's at completion
        if label.startswith("stream"):
            assert st == L.DG_OK, label
            st = ctx.decode_batch([d])[0][0]
        assert st == want and L.last_error().startswith("TIFF: "), (label, st, L.last_error())
    assert ctx.output_size(refused[0][1])[0] and L.last_error() == "TIFF: 16-bit WhiteIsZero"
