"""The JPEG and PNG re-encoders (pre_encode_images; dg_enc.hip, dg_penc.hip) at
their entropy-coding edges.  The inputs are tests/enc_cases.py's: PNG files
that decode losslessly to crafted pixels and are encoded at their own size, so
each 8x8 block and each filtered byte stream reaches the kernels as built.
test_encode_edges_cpu.py proves on the references that every case meets the
edge it is named for.

JPEG: the bytes must equal oracle.jpeg_encode's.  PNG: the bytes must equal
tests/ref_penc.py's (the documented format restated), and the file must pass
readers that share nothing with either (chunk CRCs, zlib, PIL, the oracle's
decoder).  Every comparison is equality."""
import numpy as np
import pytest

import enc_cases as E

pytestmark = pytest.mark.gpu

FMT_PNG, FMT_JPEG = 0, 1
RESIZE = dict(crop_and_resize=True, default_image_size=256, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)

JPEG = E.jpeg_cases()
PNG = E.png_cases()
_inputs = {}


def _lib():
    from datago_amd import _lib as L
    return L


def _ctx(fmt, quality=100, **kw):
    return _lib().Context(0, pre_encode_images=True, encode_format=fmt, jpeg_quality=quality, **kw)


def _input(label, arr):
    if label not in _inputs:
        _inputs[label] = E.png_input(arr)
    return _inputs[label]


def _expected(fmt, label, arr, quality):
    return E.jpeg_ref(label, arr, quality).file if fmt == FMT_JPEG else E.png_ref(label, arr).file


def _same(got, exp, label):
    if got != exp:
        n = min(len(got), len(exp))
        at = next((i for i in range(n) if got[i] != exp[i]), n)
        raise AssertionError(f"{label}: {len(got)} bytes against the reference's {len(exp)}, first difference at "
                             f"byte {at}: {got[at:at + 8].hex()} / {exp[at:at + 8].hex()}")


def _encode(ctx, fmt, cases, quality=100):
    """One decode_batch of the cases; every file checked; returns the files."""
    datas = [_input(label, arr) for label, arr, _ in cases]
    out = []
    for (label, arr, _), d, (st, enc, m) in zip(cases, datas, ctx.decode_batch(datas)):
        assert st == 0, (label, _lib().last_error())
        got = enc.tobytes()
        assert m.is_encoded == 1 and m.channels == -1 and m.nbytes == len(got), label
        assert (m.width, m.height) == (arr.shape[1], arr.shape[0]), label
        st, cap = ctx.output_size(d)
        assert st == 0 and m.nbytes <= cap, (label, m.nbytes, cap)
        if fmt == FMT_PNG:  # which side is wrong, should the bytes differ: these readers know neither
            E.png_independent_checks(got, arr)
        _same(got, _expected(fmt, label, arr, quality), label)
        out.append(got)
    return out


def _shuffled(cases, seed):
    return [cases[i] for i in np.random.default_rng(seed).permutation(len(cases))]


@pytest.mark.parametrize("quality", E.JPEG_QUALITIES)
def test_jpeg_bytes(quality):
    _encode(_ctx(FMT_JPEG, quality), FMT_JPEG, _shuffled(JPEG, quality), quality)


def test_png_bytes():
    _encode(_ctx(FMT_PNG), FMT_PNG, _shuffled(PNG, 7))


@pytest.mark.parametrize("fmt", [FMT_JPEG, FMT_PNG])
def test_batch_against_alone(fmt):
    """DC prediction, bit offsets and the shared zeroed region must not leak between the images of a batch."""
    cases = (JPEG[::6] if fmt == FMT_JPEG else PNG[::11])
    assert len(cases) >= 10
    ctx = _ctx(fmt)
    batch = _encode(ctx, fmt, cases)
    for case, b in zip(cases, batch):
        alone, = _encode(ctx, fmt, [case])
        assert alone == b, case[0]


def _dense_and_sparse(fmt):
    if fmt == FMT_JPEG:
        dense = [c for c in JPEG if c[0].startswith("noise")]
        sparse = [c for c in JPEG if c[0].startswith(("flat", "dc_", "b77", "basis"))]
    else:
        dense = [c for c in PNG if "noise" in c[0] or c[0].startswith(("expand", "crc"))]
        sparse = [c for c in PNG if "flat" in c[0] or c[0].startswith("run_")]
    assert len(dense) >= 20 and len(sparse) >= 10 and len(dense) != len(sparse)
    return dense, sparse[::-1]


@pytest.mark.parametrize("fmt", [FMT_JPEG, FMT_PNG])
def test_stale_arena(fmt):
    """One slot: every batch builds its bit streams with atomicOr in the arena the batch before left behind.
    Dense streams first, then few and sparse ones at other offsets, then the dense ones again."""
    ctx = _ctx(fmt)
    ctx.set_option("slots", 1)
    dense, sparse = _dense_and_sparse(fmt)
    _encode(ctx, fmt, dense)
    _encode(ctx, fmt, sparse)
    _encode(ctx, fmt, dense)
    _encode(ctx, fmt, sparse[3:] + dense[:5])


@pytest.mark.parametrize("fmt", [FMT_JPEG, FMT_PNG])
def test_slot_reuse(fmt):
    """The default slots, six batches: a slot's arena comes round again, sparse streams over dense ones
    (four dense batches first, so that with three or four slots the fifth and sixth land on used arenas)."""
    ctx = _ctx(fmt)
    dense, sparse = _dense_and_sparse(fmt)
    for k in range(6):
        _encode(ctx, fmt, _shuffled(dense if k < 4 else sparse, k)[: 20 - 2 * k])


@pytest.mark.parametrize("rgb8", [False, True])
@pytest.mark.parametrize("fmt", [FMT_JPEG, FMT_PNG])
def test_bucket_size_route(fmt, rgb8):
    """An input of exactly a bucket's size is copied, not resized: the pixels reach the encoder unchanged
    through a crop_and_resize context too."""
    ctx = _ctx(fmt, image_to_rgb8=rgb8, **RESIZE)
    w, h = max((b[:2] for b in ctx.buckets.buckets() if b[0] <= 330 and b[1] <= 300 and b[0] != b[1]),
               key=lambda b: b[0] * b[1])
    assert ctx.buckets.get(ctx.buckets.closest(w, h))[:2] == (w, h)
    pos = E.basis(4, 4) > 0
    tile = np.where(pos, 0, 255).astype(np.uint8)
    pattern = np.tile(np.concatenate([tile, 255 - tile], axis=1), (h // 8 + 1, w // 16 + 1))[:h, :w]
    pattern = np.stack([pattern, 255 - pattern, pattern], axis=2)
    cases = [(f"bucket_noise_{w}x{h}", E._noise(3000, h, w, 3), None),
             (f"bucket_pattern_{w}x{h}", np.ascontiguousarray(pattern), None)]
    _encode(ctx, fmt, cases)


@pytest.mark.parametrize("fmt", [FMT_JPEG, FMT_PNG])
def test_host_path_exact_buffer(fmt):
    """submit_host into a buffer of exactly output_size bytes: the bytes after it stay untouched."""
    label, arr, _ = next(c for c in (JPEG if fmt == FMT_JPEG else PNG)
                         if c[0] == ("noise_64x64_binary_rgb" if fmt == FMT_JPEG else "expand_rgb"))
    ctx = _ctx(fmt)
    d = _input(label, arr)
    st, cap = ctx.output_size(d)
    assert st == 0
    whole = np.full(cap + 8, 0xA5, np.uint8)
    ticket, metas, keep = ctx.submit_host([d], [whole[:cap]])
    ctx.wait(ticket)
    m = metas[0]
    assert m.status == 0 and m.is_encoded == 1 and m.nbytes <= cap
    _same(whole[:m.nbytes].tobytes(), _expected(fmt, label, arr, 100), label)
    assert (whole[cap:] == 0xA5).all()
    del keep
