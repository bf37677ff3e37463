"""16-bit PNGs on the GPU (context option "png16"): unfilter with 6- and
8-byte units, the sample step (byte order, tRNS key, Adam7), the 16-bit copy
and the 16-to-8 conversion of image_to_rgb8.

Expected pixels are the uint16 arrays the files were written from
(synth.encode_png16, pinned against PIL in test_png16_cpu.py); tolerance 0."""
import io

import numpy as np
import pytest
from PIL import Image

from datago_amd import synth

pytestmark = pytest.mark.gpu

CTYPES = {0: 1, 2: 3, 4: 2, 6: 4}  # colour type -> samples per pixel
# 197 x 131: four 64-unit tiles across (all three LDS tile buffers, the tile-2
# store path) and three bands, one partial (previous row from HBM, band flags)
SIZES = [(1, 1), (1, 70), (70, 1), (67, 70), (197, 131)]


def _lib():
    from datago_amd import _lib as L
    return L


def _ctx(**kw):
    return _lib().Context(0, png16=True, **kw)


@pytest.fixture(scope="module")
def ctx16():
    return _ctx()


@pytest.fixture(scope="module")
def ctx16_rgb8():
    return _ctx(image_to_rgb8=True)


def _rand(rng, h, w, spp):
    return rng.integers(0, 65536, size=(h, w, spp), dtype=np.uint16)


def _check(res, want, channels=None):
    L = _lib()
    st, arr, m = res
    assert st == L.DG_OK, L.STATUS_NAMES.get(st, st)
    h, w, c = want.shape
    assert arr.dtype == np.uint16 and arr.shape == (h, w, c)
    assert (m.width, m.height, m.original_width, m.original_height) == (w, h, w, h)
    assert (m.channels, m.bit_depth, m.is_encoded, m.nbytes) == (channels or c, 16, 0, 2 * w * h * c)
    np.testing.assert_array_equal(arr, want)


@pytest.fixture(scope="module")
def decode_cases():
    """(id, file, source array): every colour type at every size with random
    per-row filters, and every single filter at the two multi-tile sizes."""
    rng = np.random.default_rng(1600)
    out = []
    for ct, spp in CTYPES.items():
        for (w, h) in SIZES:
            px = _rand(rng, h, w, spp)
            out.append((f"t{ct}-{w}x{h}-random", synth.encode_png16(px, ct, rng, filters="random"), px))
        for f in range(5):
            for (w, h) in [(67, 70), (197, 131)]:
                px = _rand(rng, h, w, spp)
                out.append((f"t{ct}-{w}x{h}-f{f}", synth.encode_png16(px, ct, rng, filters=str(f)), px))
    return out


def test_default_off():
    L = _lib()
    rng = np.random.default_rng(1)
    px = _rand(rng, 9, 13, 3)
    data = synth.encode_png16(px, 2, rng)
    off = L.Context(0)
    st, arr, m = off.decode_batch([data])[0]
    assert st == L.DG_ERR_UNSUPPORTED and arr is None
    assert off.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    on = L.Context(0)
    on.set_option("png16", 1)
    assert on.output_size(data) == (L.DG_OK, 2 * 13 * 9 * 3)
    _check(on.decode_batch([data])[0], px)
    on.set_option("png16", 0)  # and off again
    assert on.decode_batch([data])[0][0] == L.DG_ERR_UNSUPPORTED
    _check(_ctx().decode_batch([data])[0], px)
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            on.set_option("png16", bad)
        assert e.value.status == L.DG_ERR_INVALID and "png16" in L.last_error()


@pytest.mark.parametrize("uf_units", [1, 2])
def test_decode_bit_exact(decode_cases, uf_units):
    ctx = _ctx()
    ctx.set_option("uf_units", uf_units)
    res = ctx.decode_batch([d for _, d, _ in decode_cases])
    for (cid, _, px), r in zip(decode_cases, res):
        try:
            _check(r, px)
        except AssertionError as e:
            raise AssertionError(f"{cid}: {e}") from None


@pytest.mark.parametrize("interlace", [False, True])
def test_trns_key(ctx16, interlace):
    rng = np.random.default_rng(1601)
    w, h = 37, 21
    # gray: the key, and samples equal to it in one byte only (opaque)
    key = 0x12A5
    g = _rand(rng, h, w, 1)
    g[g == key] ^= 1
    sel = rng.integers(0, 4, size=(h, w))
    g[sel == 0] = key
    g[sel == 1] = (key & 0xFF00) | 0x5A   # high byte only
    g[sel == 2] = 0xED00 | (key & 0x00FF)  # low byte only
    want_g = np.concatenate([g, np.where(g == key, 0, 65535).astype(np.uint16)], axis=2)
    # RGB: all three samples must match
    k3 = np.array([0x0102, 0xFFFE, 0x8000], np.uint16)
    c = _rand(rng, h, w, 3)
    sel = rng.integers(0, 6, size=(h, w))
    c[sel == 0] = k3
    c[sel == 1] = [k3[0], k3[1], k3[2] ^ 0x0100]   # third differs in its high byte
    c[sel == 2] = [k3[0] ^ 0x0001, k3[1], k3[2]]   # first differs in its low byte
    c[sel == 3] = [k3[0], k3[1] ^ 0x8000, k3[2]]
    a = np.where((c == k3).all(axis=2, keepdims=True), 0, 65535).astype(np.uint16)
    want_c = np.concatenate([c, a], axis=2)
    assert 0 < (want_g[:, :, 1] == 0).sum() < w * h and 0 < (a == 0).sum() < w * h
    files = [synth.encode_png16(g, 0, rng, trns=[key], interlace=interlace),
             synth.encode_png16(c, 2, rng, trns=list(k3), interlace=interlace)]
    res = ctx16.decode_batch(files)
    _check(res[0], want_g)
    _check(res[1], want_c)


def test_adam7(ctx16):
    rng = np.random.default_rng(1602)
    files, want = [], []
    for ct in (0, 6):
        for (w, h) in [(1, 1), (9, 9), (40, 30)]:
            px = _rand(rng, h, w, CTYPES[ct])
            files.append(synth.encode_png16(px, ct, rng, interlace=True))
            want.append(px)
    for r, px in zip(ctx16.decode_batch(files), want):
        _check(r, px)


def test_chunked_inflate(ctx16):
    rng = np.random.default_rng(1603)
    p8 = synth.synth_pixels(rng, 600, 400)
    px = (p8.astype(np.uint16) << 8) | p8[::-1, ::-1]  # distinct high and low bytes
    data = synth.encode_png16(px, 2, rng, level=6)
    assert len(data) > 2 * 32768  # at least two inflate chunks
    s0, c0 = ctx16.stat("png_serial_fallbacks"), ctx16.stat("png_chunks")
    _check(ctx16.decode_batch([data])[0], px)
    assert ctx16.stat("png_chunks") > c0
    assert ctx16.stat("png_serial_fallbacks") == s0


def test_image_to_rgb8(ctx16_rgb8):
    L = _lib()
    rng = np.random.default_rng(1604)
    every = rng.permutation(65536).astype(np.uint16).reshape(256, 256, 1)  # each 16-bit value once
    la = _rand(rng, 33, 45, 2)
    rgba = _rand(rng, 33, 45, 4)
    rgb = _rand(rng, 20, 31, 3)
    files = [synth.encode_png16(every, 0, rng), synth.encode_png16(la, 4, rng), synth.encode_png16(rgba, 6, rng),
             synth.encode_png16(rgb, 2, rng), synth.encode_png16(la, 4, rng, interlace=True)]
    srcs = [every, la, rgba, rgb, la]
    for (st, arr, m), px in zip(ctx16_rgb8.decode_batch(files), srcs):
        assert st == L.DG_OK
        h, w, c = px.shape
        colour = px[:, :, :3] if c >= 3 else np.repeat(px[:, :, :1], 3, axis=2)  # alpha dropped, luma replicated
        want = ((colour.astype(np.uint32) + 128) // 257).astype(np.uint8)
        assert arr.dtype == np.uint8 and arr.shape == (h, w, 3)
        assert (m.channels, m.bit_depth, m.nbytes, m.width, m.height) == (3, 8, 3 * w * h, w, h)
        np.testing.assert_array_equal(arr, want)


def _smooth16(rng, w, h):
    p8 = synth.synth_pixels(rng, w, h, gray=True).reshape(h, w, 1)
    return (p8.astype(np.uint16) * 257) ^ (np.arange(w, dtype=np.uint16)[None, :, None] & 0xFF)


def test_buckets():
    L = _lib()
    rng = np.random.default_rng(1605)
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)
    ctx = _ctx(**kw)
    bw, bh, _ = min(ctx.buckets.buckets(), key=lambda b: b[0] * b[1])
    px = _smooth16(rng, bw, bh)
    exact = synth.encode_png16(px, 0, rng)
    other = synth.encode_png16(_smooth16(rng, bw - 16, bh + 5), 0, rng)
    res = ctx.decode_batch([exact, other])
    _check(res[0], px)
    assert res[0][2].bucket == ctx.buckets.closest(bw, bh)
    assert res[1][0] == L.DG_ERR_UNSUPPORTED
    assert "16-bit" in L.last_error()
    st, _ = ctx.output_size(other)
    assert st == L.DG_ERR_UNSUPPORTED and "16-bit resize" in L.last_error()
    # an encoder never sees 16-bit samples
    enc = _ctx(pre_encode_images=True, **kw)
    assert enc.decode_batch([exact])[0][0] == L.DG_ERR_UNSUPPORTED
    assert "16-bit" in L.last_error()
    # after image_to_rgb8 the image is RGB8 and the encoders take it
    want = np.repeat(((px.astype(np.uint32) + 128) // 257).astype(np.uint8), 3, axis=2)
    st, buf, m = _ctx(pre_encode_images=True, image_to_rgb8=True, encode_format=0, **kw).decode_batch([exact])[0]
    assert st == L.DG_OK and m.is_encoded == 1
    back = Image.open(io.BytesIO(buf.tobytes()))
    assert back.mode == "RGB"
    np.testing.assert_array_equal(np.array(back), want)
    st, buf, m = _ctx(pre_encode_images=True, image_to_rgb8=True, encode_format=1, **kw).decode_batch([exact])[0]
    assert st == L.DG_OK and m.is_encoded == 1
    back = Image.open(io.BytesIO(buf.tobytes()))
    assert back.format == "JPEG" and back.size == (bw, bh)


def test_mixed_batch(ctx16):
    L = _lib()
    rng = np.random.default_rng(1606)
    files = [synth.make_png(1700 + i, 33, 17, kind) for i, kind in enumerate(synth.PNG_KINDS)]
    files += [synth.make_png(1750, 40, 30, "RGBA", interlace=True), synth.make_jpeg(1751, 64, 48)]
    n8 = len(files)
    deep = [(_rand(rng, 19, 23, spp), ct) for ct, spp in CTYPES.items()]
    files += [synth.encode_png16(px, ct, rng) for px, ct in deep]
    order = rng.permutation(len(files))  # 16-bit files between the others
    got = ctx16.decode_batch([files[i] for i in order])
    ref = L.Context(0).decode_batch([files[i] for i in order])
    for k, i in enumerate(order):
        if i < n8:
            assert got[k][0] == L.DG_OK and ref[k][0] == L.DG_OK
            assert got[k][1].dtype == np.uint8 and got[k][2].bit_depth == 8
            np.testing.assert_array_equal(got[k][1], ref[k][1])
        else:
            assert ref[k][0] == L.DG_ERR_UNSUPPORTED
            _check(got[k], deep[i - n8][0])


def test_decode_one_and_torch(ctx16):
    import torch
    L = _lib()
    rng = np.random.default_rng(1607)
    px = _rand(rng, 70, 67, 3)
    data = synth.encode_png16(px, 2, rng)
    _check(ctx16.decode_one(data), px)
    buf = np.empty(2 * px.size, np.uint8)
    st, arr, m = ctx16.decode_one(data, out=buf)
    _check((st, arr, m), px)
    assert arr.ctypes.data == buf.ctypes.data  # a view of the caller's bytes
    st, t, m = ctx16.decode_batch_torch([data])[0]
    assert st == L.DG_OK and t.dtype == torch.uint16 and t.is_cuda and tuple(t.shape) == px.shape
    assert m.bit_depth == 16
    np.testing.assert_array_equal(t.cpu().numpy(), px)
    # submit_host into caller-owned bytes: payload_array is the typed view
    ticket, metas, keep = ctx16.submit_host([data], [buf])
    ctx16.wait(ticket)
    np.testing.assert_array_equal(L.payload_array(buf, metas[0]), px)


def test_bad_filter_byte(ctx16):
    L = _lib()
    rng = np.random.default_rng(1608)
    px = _rand(rng, 70, 67, 3)
    good = synth.encode_png16(px, 2, rng)
    bad = [synth.encode_png16(_rand(rng, 70, 67, spp), ct, rng, filters="5") for ct, spp in CTYPES.items()]
    res = ctx16.decode_batch(bad + [good])
    assert [r[0] for r in res[:-1]] == [L.DG_ERR_CORRUPT] * len(bad)
    _check(res[-1], px)
