"""The PNG re-encoder with per-image Huffman codes (context option
"penc_dynamic"; k_penc_tree and the histogram / table paths of dg_penc.hip).
Inputs are PNG files that decode losslessly to crafted pixels and are encoded
at their own size: enc_cases.png_cases() plus penc_dyn_cases.new_cases().
test_penc_dyn_cpu.py proves on the reference that the set reaches both
limiters, both block types and every run-length symbol.

With the option on the bytes must equal tests/ref_penc_dyn.py's; off (the
default) they must equal tests/ref_penc.py's.  Every comparison is equality."""
import io

import numpy as np
import pytest

import enc_cases as E
import penc_dyn_cases as C
import ref_penc_dyn as D

pytestmark = pytest.mark.gpu

FMT_PNG, FMT_JPEG = 0, 1
RESIZE = dict(crop_and_resize=True, default_image_size=256, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)
CASES = C.all_cases()
NAMED = (C.FIB_LABEL,) + C.CL_LIMITED  # the limiter cases: named in a failure message
_inputs = {}


def _lib():
    from datago_amd import _lib as L
    return L


def _ctx(dynamic=True, fmt=FMT_PNG, **kw):
    return _lib().Context(0, pre_encode_images=True, encode_format=fmt, jpeg_quality=90, penc_dynamic=dynamic, **kw)


def _input(label, arr):
    if label not in _inputs:
        _inputs[label] = E.png_input(arr)
    return _inputs[label]


def _same(got, exp, label):
    if got != exp:
        n = min(len(got), len(exp))
        at = next((i for i in range(n) if got[i] != exp[i]), n)
        kind = " (a limiter case)" if label in NAMED else ""
        raise AssertionError(f"{label}{kind}: {len(got)} bytes against the reference's {len(exp)}, first difference "
                             f"at byte {at}: {got[at:at + 8].hex()} / {exp[at:at + 8].hex()}; "
                             f"{D.explain_difference(got, exp)}")


def _expected(label, arr, dynamic):
    return C.dyn_ref(label, arr).file if dynamic else E.png_ref(label, arr).file


def _encode(ctx, cases, dynamic=True, independent=True):
    """One decode_batch of the cases; every file checked; returns the files."""
    datas = [_input(label, arr) for label, arr in cases]
    out, failed = [], []
    for (label, arr), d, (st, enc, m) in zip(cases, datas, ctx.decode_batch(datas)):
        assert st == 0, (label, _lib().last_error())
        got = enc.tobytes()
        assert m.is_encoded == 1 and m.channels == -1 and m.nbytes == len(got), label
        assert (m.width, m.height) == (arr.shape[1], arr.shape[0]), label
        st, cap = ctx.output_size(d)
        assert st == 0 and m.nbytes <= cap, (label, m.nbytes, cap)
        try:
            _same(got, _expected(label, arr, dynamic), label)
            if independent:
                E.png_independent_checks(got, arr)
        except AssertionError as err:
            failed.append((label, str(err)[:400]))
        out.append(got)
    named = [f for f in failed if f[0] in NAMED]
    assert not failed, (f"{len(failed)} of {len(cases)} files differ; limiter cases among them: "
                        f"{[f[0] for f in named]}; first: {(named or failed)[0]}")
    return out


def _shuffled(cases, seed):
    return [cases[i] for i in np.random.default_rng(seed).permutation(len(cases))]


def _dozen():
    want = ("photo_gray_176x80", "const_gray_128", "one_pixel_gray", "rgb_3x2", "random_rgba_64", "filt_vramp_c4",
            "filt_paeth_c3", "expand_gray_odd", "flat_zero", "run_258", "piece_1025_noise_25x10x4", "crc_1024")
    by = dict(CASES)
    return [(k, by[k]) for k in want]


def test_off_by_default():
    L = _lib()
    cases = _dozen()
    assert any(C.dyn_ref(k, a).dyn for k, a in cases) and not all(C.dyn_ref(k, a).dyn for k, a in cases)
    ctx = L.Context(0, pre_encode_images=True, encode_format=FMT_PNG)
    _encode(ctx, cases, dynamic=False)
    ctx.set_option("penc_dynamic", 1)
    _encode(ctx, cases, dynamic=True)
    ctx.set_option("penc_dynamic", 0)  # and off again: the fixed files
    _encode(ctx, cases, dynamic=False)
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("penc_dynamic", bad)
        assert e.value.status == L.DG_ERR_INVALID and "penc_dynamic" in L.last_error()
        assert str(bad) in L.last_error()


def test_jpeg_unchanged():
    datas = [_input(k, a) for k, a in _dozen() if a.shape[2] in (1, 3)]
    off = _ctx(False, FMT_JPEG).decode_batch(datas)
    on = _ctx(True, FMT_JPEG).decode_batch(datas)
    assert len(datas) >= 8
    for (s0, e0, _), (s1, e1, _) in zip(off, on):
        assert s0 == 0 and s1 == 0 and e0.tobytes() == e1.tobytes() and e0.tobytes()[:2] == b"\xff\xd8"


def test_files():
    """Every case in one shuffled batch: both block types side by side in one zeroed region."""
    _encode(_ctx(), _shuffled(CASES, 11))


def test_batch_against_alone():
    cases = CASES[::11] + [c for c in CASES if c[0] in ("photo_gray_176x80", "one_pixel_gray", "filt_paeth_c3")]
    ctx = _ctx()
    batch = _encode(ctx, cases, independent=False)
    for case, b in zip(cases, batch):
        alone, = _encode(ctx, [case], independent=False)
        assert alone == b, case[0]


def test_stale_arena():
    """One slot: the histograms, the header bits and the atomicOr packing all build on the arena the batch
    before left behind.  Dense streams, then few and sparse ones at other offsets, then the dense ones again."""
    ctx = _ctx()
    ctx.set_option("slots", 1)
    dense = [c for c in CASES if "noise" in c[0] or c[0].startswith(("expand", "crc", "photo", "random"))]
    sparse = [c for c in CASES if "flat" in c[0] or c[0].startswith(("run_", "const", "one_pixel"))][::-1]
    assert len(dense) >= 20 and len(sparse) >= 10 and len(dense) != len(sparse)
    assert any(C.dyn_ref(*c).dyn for c in sparse) and any(not C.dyn_ref(*c).dyn for c in sparse)
    _encode(ctx, dense, independent=False)
    _encode(ctx, sparse, independent=False)
    _encode(ctx, dense, independent=False)
    _encode(ctx, sparse[3:] + dense[:5], independent=False)


def test_through_the_transform():
    """A crop_and_resize context with the option on: each file decodes (PIL, and the library's own PNG decoder,
    which then reads a one-code distance tree) to the pixels the same configuration returns un-encoded."""
    from PIL import Image

    from datago_amd import synth
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    L = _lib()
    cfg = ImageTransformConfig(crop_and_resize=True, default_image_size=256, downsampling_ratio=16,
                               min_aspect_ratio=0.5, max_aspect_ratio=2.0)
    enc = ARAwareTransform(cfg, 0, penc_dynamic=True).context(ImageEncoding(encode_images=True, encode_format=FMT_PNG))
    raw = L.Context(0, **RESIZE)
    plain = L.Context(0)
    datas = [synth.make_jpeg(40, 400, 300, 90), synth.make_png(41, 300, 260, "RGBA"),
             synth.make_png(42, 200, 150, "LA")]
    for i, (d, (se, pe, me), (sr, pr, mr)) in enumerate(zip(datas, enc.decode_batch(datas), raw.decode_batch(datas))):
        assert se == 0 and sr == 0, (i, L.last_error())
        png = pe.tobytes()
        assert me.is_encoded == 1 and me.nbytes == len(png)
        ref = pr.reshape(mr.height, mr.width, -1)
        if ref.shape[2] == 2 and (mr.original_width, mr.original_height) != (mr.width, mr.height):
            # resized LA: a GrayImage over the first w * h LA bytes
            ref = ref.reshape(-1)[: mr.width * mr.height].reshape(mr.height, mr.width, 1)
        blk, _ = D.read_block(D.idat_deflate(png))
        assert blk.dyn and blk.distlen == [1], i  # resized photos: the dynamic block is the shorter one
        assert len(png) < ref.size, (i, len(png), ref.size)
        pil = np.asarray(Image.open(io.BytesIO(png)))
        assert np.array_equal(pil.reshape(ref.shape), ref), i
        (sb, pb, mb), = plain.decode_batch([png])
        assert sb == 0, (i, L.last_error())
        assert np.array_equal(pb.reshape(ref.shape), ref), i


def test_host_output_exact_buffer():
    """submit_host: exactly meta.nbytes bytes land in the caller's buffer.  The library takes no buffer below
    output_size (DG_ERR_SMALL_BUFFER, checked before anything is encoded), so the buffer has that capacity and
    every byte of it past the file -- a third of the buffer for a dynamic block -- must stay untouched."""
    label, arr = next(c for c in CASES if c[0] == "photo_rgb_128")
    exp = C.dyn_ref(label, arr)
    assert exp.dyn
    ctx = _ctx()
    d = _input(label, arr)
    n = len(exp.file)
    st, cap = ctx.output_size(d)
    assert st == 0 and n < cap
    whole = np.full(cap + 8, 0xA5, np.uint8)
    ticket, metas, keep = ctx.submit_host([d], [whole[:cap]])
    ctx.wait(ticket)
    m = metas[0]
    assert m.status == 0 and m.is_encoded == 1 and m.nbytes == n, (m.status, m.nbytes, n, _lib().last_error())
    _same(whole[:n].tobytes(), exp.file, label)
    assert (whole[n:] == 0xA5).all()
    del keep
