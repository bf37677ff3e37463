"""1-bit TIFFs on the GPU behind context option "tiff_bilevel" (k_tiff_g4 in dg_tiff_g4.hip, k_tiff_expand1 in
dg_tiff.hip): bit-exact against the 0 / 1 array each file was made from and against Pillow (libtiff), under every
compression, photometric, byte order and segment layout; the option gates; the refusals; and past the decode against
the 8-bit gray PNG twin."""
import io

import numpy as np
import pytest
from PIL import Image

import tiff_bilevel_cases as B
import tiff_craft as T
from datago_amd import synth
from test_gpu_tiff import RESIZE, _lib

pytestmark = pytest.mark.gpu
CASES = B.cases()
PAGE = CASES[-1][1]


@pytest.fixture(scope="module")
def ctx():
    c = _lib().Context(0, tiff=True, tiff_bilevel=True, tiff_deflate=True)
    yield c
    c.close()


def _check(L, files, res):
    for (label, data, pix), (st, arr, m) in zip(files, res):
        assert st == L.DG_OK, (label, st, L.last_error())
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("L")), pix), label
        got = np.asarray(arr).reshape(pix.shape)
        assert np.array_equal(got, pix), (label, int((got != pix).sum()), np.argwhere(got != pix)[:4].tolist())
        assert (m.original_width, m.original_height, m.width, m.height, m.channels, m.bit_depth, m.is_encoded) == \
               (pix.shape[1], pix.shape[0]) * 2 + (1, 8, 0), label


@pytest.mark.parametrize("comp", list(B.COMP))
def test_case_list_in_one_batch(ctx, comp):
    files = [(label, B.written(arr, comp, rps), np.asarray(arr, np.uint8) * 255) for label, arr, rps in CASES]
    _check(_lib(), files, ctx.decode_batch([f[1] for f in files]))


@pytest.mark.parametrize("tile", [None, (16, 16), (32, 16)], ids=["strips", "16x16", "32x16"])
@pytest.mark.parametrize("be", [False, True], ids=["II", "MM"])
@pytest.mark.parametrize("photo", [0, 1])
def test_photometric_byte_order_and_tiles(ctx, photo, be, tile):
    files = [("%s g4=%d" % (label, g4), B.crafted(arr, g4, photo, be, tile), np.asarray(arr if photo else 1 - arr, np.uint8) * 255)
             for label, arr, rps in CASES if label in ("noise 65", "edge +3", "page") for g4 in (True, False)]
    _check(_lib(), files, ctx.decode_batch([f[1] for f in files]))


def test_option_gates():
    L = _lib()
    g4, zipped = B.written(PAGE, "g4"), B.written(PAGE, "deflate")
    for kw, st, text in [(dict(tiff=True), L.DG_ERR_UNSUPPORTED, "TIFF: samples not 8 bits"), (dict(tiff_bilevel=True), L.DG_ERR_CORRUPT, None)]:
        c = L.Context(0, **kw)
        for d in (g4, B.written(PAGE, "raw")):
            assert c.output_size(d)[0] == st and text in (None, L.last_error()) and c.decode_batch([d])[0][0] == st, (kw, L.last_error())
        c.close()
    c = L.Context(0, tiff=True, tiff_bilevel=True)
    assert c.output_size(zipped)[0] == L.DG_ERR_UNSUPPORTED and L.last_error() == "TIFF: compression other than none, LZW and PackBits"
    assert c.output_size(g4) == (L.DG_OK, PAGE.size)
    c.close()


def test_refusals_and_the_good_files_beside_them(ctx):
    L = _lib()
    g8, strip = T.noise(8, 24, 2, 3), B.g4_strip(1 - PAGE)
    refused = [  # (the text in dg_last_error, the file, refused by the kernel)
        ("Modified Huffman or Group 3 compression", B.crafted(PAGE, False, tags=[(259, 3, [2])]), False),
        ("Modified Huffman or Group 3 compression", B.crafted(PAGE, False, tags=[(259, 3, [3])]), False),
        ("Group 4 uncompressed mode", B.crafted(PAGE, True, tags=[(293, 4, [2])]), False),
        ("predictor 2 on 1-bit samples", B.crafted(PAGE, False, tags=[(317, 3, [2])]), False),
        ("2- or 4-bit samples", T.tiff(g8[:, :, 0], tags=[(258, 3, [2])]), False),
        ("2- or 4-bit samples", T.tiff(g8[:, :, 0], tags=[(258, 3, [4])]), False),
        ("bilevel with an extra sample", T.tiff(g8, tags=[(258, 3, [1, 1])]), False),
        ("Group 4 row wider than 16,384 pixels", B.crafted(np.ones((1, 16385), int), True, pack=lambda d: b"\0"), False),
        ("irregular Group 4 stream", B.crafted(PAGE, True, pack=lambda d: strip[:len(strip) // 2]), True),  # cut short
        ("irregular Group 4 stream", B.crafted(PAGE, True, pack=lambda d: b"\x02" + strip[1:]), True)]  # 0000001x: the extension code
    good = ("page", B.written(PAGE, "g4", 16), np.asarray(PAGE, np.uint8) * 255)
    res = ctx.decode_batch([good[1]] + [d for _, d, _ in refused] + [good[1]])
    _check(L, [good, good], [res[0], res[-1]])
    for (text, d, stream), (st, arr, m) in zip(refused, res[1:-1]):
        assert st == L.DG_ERR_UNSUPPORTED and arr is None, (text, st)
        st = ctx.output_size(d)[0]  # each names itself: the header's at planning, the stream's at completion
        if stream:
            assert st == L.DG_OK, text
            st = ctx.decode_batch([d])[0][0]
        assert st == L.DG_ERR_UNSUPPORTED and L.last_error() == "TIFF: " + text, (text, st, L.last_error())


def test_downstream_as_the_gray_png_twin():
    L = _lib()
    y, x = np.mgrid[0:200, 0:300]
    pix = (((x // 7 + y // 5) % 3 > 0) | ((x * y) % 11 == 0)).astype(np.uint8) * 255
    data, twin = B.written(pix // 255, "g4"), synth.pil_png(pix)
    for kw in (dict(), dict(image_to_rgb8=True), dict(pre_encode_images=True, encode_format=0)):
        c = L.Context(0, tiff=True, tiff_bilevel=True, **RESIZE, **kw)
        (st, arr, m), (tst, tarr, tm) = c.decode_batch([data, twin])
        assert st == tst == L.DG_OK, (kw, st, tst, L.last_error())
        assert (m.bucket, m.width, m.height, m.channels, m.bit_depth, m.is_encoded) == \
               (tm.bucket, tm.width, tm.height, tm.channels, tm.bit_depth, tm.is_encoded) and (m.width, m.height) != (300, 200), kw
        assert arr.tobytes() == tarr.tobytes() and len(arr.tobytes()) > 0, kw
        c.close()
