"""The PNG re-encoder with LZ77 matches (context option "penc_match"; k_penc_match, k_penc_mtree, k_penc_mcount
and k_penc_mwrite of dg_penc.hip) against tests/ref_penc_match.py over penc_match_cases, whose edges
test_penc_match_cpu.py proves on the reference.  Inputs are PNG files that decode losslessly to the crafted
pixels and are encoded at their own size.  Every comparison is equality."""
import io

import numpy as np
import pytest

import enc_cases as E
import penc_match_cases as C
import ref_penc16
import ref_penc_match as R

pytestmark = pytest.mark.gpu

FMT_PNG = 0
CASES = [(label, arr) for label, arr, _, _ in C.cases()]
_inputs = {}


def _lib():
    from datago_amd import _lib as L
    return L


def _ctx(dynamic, match=True, **kw):
    return _lib().Context(0, pre_encode_images=True, encode_format=FMT_PNG, penc_dynamic=dynamic, penc_match=match, **kw)


def _input(label, arr):
    if label not in _inputs:
        _inputs[label] = E.png_input(arr)
    return _inputs[label]


def _encode(ctx, cases, expected):
    """One decode_batch of the cases; every file against expected(label, arr); returns the files."""
    out, failed = [], []
    for (label, arr), (st, enc, m) in zip(cases, ctx.decode_batch([_input(*c) for c in cases])):
        assert st == 0, (label, _lib().last_error())
        got, exp = enc.tobytes(), expected(label, arr)
        assert m.is_encoded == 1 and m.nbytes == len(got), label
        if got != exp:
            at = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
            failed.append(f"{label}: {len(got)} bytes against {len(exp)}, first difference at byte {at}")
        out.append(got)
    assert not failed, f"{len(failed)} of {len(cases)} files differ: {failed[:6]}"
    return out


def _shuffled(cases, seed):
    return [cases[i] for i in np.random.default_rng(seed).permutation(len(cases))]


@pytest.mark.parametrize("dynamic", [False, True], ids=["fixed", "dynamic"])
def test_files(dynamic):
    """Every case in one shuffled batch: all four kinds of block side by side."""
    _encode(_ctx(dynamic), _shuffled(CASES, 21), lambda k, a: C.ref(k, a, dynamic).file)


@pytest.mark.parametrize("dynamic", [False, True], ids=["fixed", "dynamic"])
def test_off_on_off(dynamic):
    L = _lib()
    cases = CASES[::3]
    ctx = _ctx(dynamic, match=False)
    _encode(ctx, cases, lambda k, a: R.parent(a, dynamic))
    ctx.set_option("penc_match", 1)
    _encode(ctx, cases, lambda k, a: C.ref(k, a, dynamic).file)
    ctx.set_option("penc_match", 0)
    _encode(ctx, cases, lambda k, a: R.parent(a, dynamic))
    with pytest.raises(L.DgError) as e:
        ctx.set_option("penc_match", 2)
    assert e.value.status == L.DG_ERR_INVALID and "penc_match" in L.last_error()


def test_batch_against_alone():
    cases = CASES[::4]
    ctx = _ctx(True)
    batch = _encode(ctx, cases, lambda k, a: C.ref(k, a, True).file)
    for case, b in zip(cases, batch):
        assert ctx.decode_batch([_input(*case)])[0][1].tobytes() == b, case[0]


def test_stale_arena():
    """One slot: histograms, token buffers and the atomicOr packing build on what the batch before left."""
    ctx = _ctx(True)
    ctx.set_option("slots", 1)
    dense = [c for c in CASES if c[0].startswith(("far_", "every", "synth", "text"))]
    sparse = [c for c in CASES if c[0].startswith(("stream_", "checker", "one_", "overlap"))][::-1]
    assert len(dense) >= 10 and len(sparse) >= 10 and len(dense) != len(sparse)
    for cases in (dense, sparse, dense, sparse[3:] + dense[:4]):
        _encode(ctx, cases, lambda k, a: C.ref(k, a, True).file)


def test_through_the_transform():
    """A crop_and_resize context with the option on: each file decodes through PIL and through the library's own
    PNG decoder to the pixels the same configuration returns un-encoded."""
    from PIL import Image

    from datago_amd import synth
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    L = _lib()
    kw = dict(crop_and_resize=True, default_image_size=256, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)
    tfm = ARAwareTransform(ImageTransformConfig(**kw), 0, penc_dynamic=True, penc_match=True)
    enc = tfm.context(ImageEncoding(encode_images=True, encode_format=FMT_PNG))
    raw, plain = L.Context(0, **kw), L.Context(0)
    datas = [synth.make_jpeg(40, 400, 300, 90), synth.make_png(41, 300, 260, "RGBA"), synth.make_png(42, 200, 150, "LA"),
             E.png_input(np.kron(CASES[-5][1], np.ones((3, 3, 1), np.uint8)))]  # the RGB tile, three times as large
    for i, ((se, pe, me), (sr, pr, mr)) in enumerate(zip(enc.decode_batch(datas), raw.decode_batch(datas))):
        assert se == 0 and sr == 0, (i, L.last_error())
        png = pe.tobytes()
        ref = pr.reshape(mr.height, mr.width, -1)
        if ref.shape[2] == 2 and (mr.original_width, mr.original_height) != (mr.width, mr.height):
            ref = ref.reshape(-1)[: mr.width * mr.height].reshape(mr.height, mr.width, 1)  # resized LA: a GrayImage
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))).reshape(ref.shape), ref), i
        (sb, pb, _), = plain.decode_batch([png])
        assert sb == 0 and np.array_equal(pb.reshape(ref.shape), ref), (i, L.last_error())


def test_sixteen_bit():
    from datago_amd import synth
    label, px = C.GRAY16
    ctx = _ctx(True, png16=True, penc16=True)
    (st, enc, m), = ctx.decode_batch([synth.encode_png16(px, 0, np.random.default_rng(5))])
    assert st == 0, _lib().last_error()
    assert enc.tobytes() == R.encode_rows(ref_penc16.be_rows(px), 16, True).file
