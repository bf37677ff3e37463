"""The encoder edge cases (tests/enc_cases.py) against their references alone,
without a GPU: every case's property must hold on what the reference makes of
it -- oracle.jpeg_encode for JPEG, tests/ref_penc.py for PNG -- so that the
GPU comparisons built on these inputs (test_gpu_encode_edges.py) cannot pass
without meeting the edge they are named for.  The references' output is also
put through independent readers: PIL, zlib, the chunk CRCs and the oracle's
own PNG decoder."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import enc_cases as E
from oracle import oracle as O

JPEG = E.jpeg_cases()
PNG = E.png_cases()


def test_labels_are_unique():
    for cases in (JPEG, PNG):
        labels = [c[0] for c in cases]
        assert len(set(labels)) == len(labels)
        assert all(a.dtype == np.uint8 and a.ndim == 3 for _, a, _ in cases)


@pytest.mark.parametrize("label,arr,prop", JPEG, ids=[c[0] for c in JPEG])
def test_jpeg_case(label, arr, prop):
    assert prop(lambda q: E.jpeg_ref(label, arr, q)), label
    h, w, c = arr.shape
    for q in E.JPEG_QUALITIES:
        f = E.jpeg_ref(label, arr, q)
        assert len(f.file) <= O.jpeg_encode_bound(w, h, c)
        im = Image.open(io.BytesIO(f.file))
        im.load()
        assert im.size == (w, h) and im.mode == ("L" if c == 1 else "RGB")


@pytest.mark.parametrize("name,pred", E.JPEG_SET_PROPERTIES, ids=[p[0] for p in E.JPEG_SET_PROPERTIES])
def test_jpeg_set_property(name, pred):
    assert pred({label: E.jpeg_ref(label, arr, 100) for label, arr, _ in JPEG}), name


def test_jpeg_low_qualities_keep_their_edges():
    """Quality 1 (every divisor clamped to 255) and 50 on the noise and basis cases: the files differ from
    quality 100's, and quality 1 still holds non-zero AC coefficients to code."""
    for label, arr, _ in JPEG:
        if label.startswith(("noise_64", "basis")):
            f1, f50, f100 = (E.jpeg_ref(label, arr, q) for q in (1, 50, 100))
            assert f1.bits < f50.bits < f100.bits, label
            assert f1.coefs[:, 1:].any(), label
    assert (O.jpeg_qtables(1) == 255).all() and (O.jpeg_qtables(100) == 1).all()


@pytest.mark.parametrize("label,arr,prop", PNG, ids=[c[0] for c in PNG])
def test_png_case(label, arr, prop):
    ref = E.png_ref(label, arr)
    assert prop(ref), label
    filt = E.png_independent_checks(ref.file, arr)
    h, w, c = arr.shape
    rows = np.frombuffer(filt, np.uint8).reshape(h, w * c + 1)
    assert np.array_equal(rows[:, 0], ref.filters)
    assert filt == ref.stream.tobytes()
    assert ref.cn == 4 + struct.unpack(">I", ref.file[33:37])[0]
    # the input file the GPU tests feed decodes to the array too
    st, dec = O.png_decode(E.png_input(arr))
    assert st == 0 and np.array_equal(dec, arr)


@pytest.mark.parametrize("name,pred", E.PNG_SET_PROPERTIES, ids=[p[0] for p in E.PNG_SET_PROPERTIES])
def test_png_set_property(name, pred):
    assert pred({label: E.png_ref(label, arr) for label, arr, _ in PNG}), name


def test_length_symbols_match_zlib():
    """ref_penc's length table against zlib's own reading: a stream of one literal and one match of every
    length inflates to that many bytes."""
    import ref_penc
    for n in range(3, 259):
        s = np.concatenate([[7], np.full(n + 1, 9)]).astype(np.uint8)  # literal 7, literal 9, match of n
        body, syms, matches = ref_penc.deflate_fixed(s)
        assert matches == [(2, n)] and syms == [ref_penc.length_symbol(n)[0]]
        assert zlib.decompress(body, -15) == s.tobytes()
