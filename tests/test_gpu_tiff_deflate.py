"""Deflate-compressed TIFFs on the GPU behind context option "tiff_deflate" (k_tiff_inflate, dg_tiff_inflate.hip):
bit-exact against Pillow (libtiff over zlib), whose decode of every file is itself compared with the array the file was
made from; the streams zlib refuses are refused; past the decode, the oracle's result for the PNG twin."""
import io

import numpy as np
import pytest
from PIL import Image

import tiff_craft as T
import tiff_deflate_craft as D
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O
from test_gpu_tiff import CFG, RESIZE, _check, _lib, _written

pytestmark = pytest.mark.gpu

CASES = D.cases()


@pytest.fixture(scope="module")
def ctx():
    c = _lib().Context(0, tiff=True, tiff_deflate=True)
    yield c
    c.close()


def test_option_acts_only_beside_tiff():
    L = _lib()
    group, label, data, pix = CASES[2]
    c = L.Context(0, tiff=True)
    assert c.output_size(data)[0] == L.DG_ERR_UNSUPPORTED and c.decode_batch([data])[0][0] == L.DG_ERR_UNSUPPORTED
    c.set_option("tiff_deflate", 1)
    assert c.output_size(data) == (L.DG_OK, pix.size)
    _check(L, [CASES[2][1:]], c.decode_batch([data]))
    c.close()
    c = L.Context(0, tiff_deflate=True)
    assert c.output_size(data)[0] == L.DG_ERR_CORRUPT and c.decode_batch([data])[0][0] == L.DG_ERR_CORRUPT
    c.close()


@pytest.mark.parametrize("group", ["blocks", "matches", "layout"])
def test_crafted_files_bit_exact_in_one_batch(ctx, group):
    files = [c[1:] for c in CASES if c[0] == group]
    assert len(files) >= 4
    _check(_lib(), files, ctx.decode_batch([c[1] for c in files]))


@pytest.mark.parametrize("comp,pred", [("tiff_adobe_deflate", 0), ("tiff_adobe_deflate", 1), ("tiff_deflate", 0), ("tiff_deflate", 1)])
def test_pillow_written_files(ctx, comp, pred):
    files = [_written(mode, comp, pred) for mode in ("L", "LA", "RGB", "RGBA")]
    _check(_lib(), files, ctx.decode_batch([c[1] for c in files]))


def test_eight_images_with_different_segment_counts(ctx):
    pix = [T.noise(70, 97, 3, 20 + k) for k in range(8)]
    files = [("rps %d" % rps, T.tiff(p, comp=8, pred=2, rps=rps, pack=D.z(1 + k)), p)
             for k, (rps, p) in enumerate(zip((1, 2, 3, 5, 7, 16, 35, 70), pix))]
    others = [c for c in T.cases() if c[0] in ("lzw pred rps 7", "packbits across rows")]
    assert len(others) == 2
    batch = files[:3] + others[:1] + files[3:6] + others[1:] + files[6:]
    _check(_lib(), batch, ctx.decode_batch([c[1] for c in batch]))
    _check(_lib(), files[::3], [ctx.decode_one(c[1]) for c in files[::3]])  # and alone, through decode_one


def test_refusals_and_the_good_files_beside_them(ctx):
    L = _lib()
    good, refused = next(c[1:] for c in CASES if c[1] == "mix"), D.refusals()
    res = ctx.decode_batch([good[1]] + [d for _, d in refused] + [good[1]])
    for (label, d), (st, arr, m) in zip(refused, res[1:-1]):
        assert st == L.DG_ERR_CORRUPT and arr is None, (label, st)
        with pytest.raises(OSError):
            Image.open(io.BytesIO(d)).load()
    _check(L, [good, good], [res[0], res[-1]])
    for label, d in refused:  # each names itself at completion
        assert ctx.output_size(d)[0] == L.DG_OK, label
        assert ctx.decode_batch([d])[0][0] == L.DG_ERR_CORRUPT and L.last_error().startswith("TIFF: "), (label, L.last_error())
        assert ("Adler" in L.last_error()) == (label == "wrong Adler-32"), (label, L.last_error())


def test_downstream_as_the_png_twin():
    """Resize to a bucket equals the oracle's result for the pixels and the PNG twin's result."""
    L = _lib()
    label, data, pix = _written("RGBA", "tiff_adobe_deflate", 1, 300, 200, 11)
    tw, th = B.ARAwareTransform(*CFG).target_size(300, 200)
    exp = O.crop_and_resize(pix, tw, th, O.MODE_FIR)
    c = L.Context(0, tiff=True, tiff_deflate=True, **RESIZE)
    (st, arr, m), (tst, tarr, tm) = c.decode_batch([data, synth.pil_png(pix)])
    assert st == tst == L.DG_OK and (m.bucket, m.width, m.height, m.channels) == (tm.bucket, tw, th, 4)
    assert np.array_equal(np.asarray(arr).reshape(exp.shape), exp) and np.array_equal(np.asarray(tarr).reshape(exp.shape), exp)
    c.close()
