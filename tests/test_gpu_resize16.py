"""16-bit PNGs resized to their bucket on the GPU (context option "resize16"
beside "png16"): the image crate's resize_to_fill(Lanczos3) as the reference
applies it to non-U8 pixel types (k_r16_taps / k_r16_v / k_r16_h).

Expected pixels come from the NumPy restatement tests/ref_resize16.py applied
to the uint16 arrays the files were written from; tolerance 0 everywhere.
Sources are chosen relative to the contexts' own bucket lists (128 / 16: 80 x
176 ... 176 x 80); a second context with 32 / 8 buckets (24 x 40 ... 40 x 24)
carries the steep downscales at small sources, a third with 256 / 32 buckets
one output wider than a horizontal pass's 256-pixel workgroup."""
import io

import numpy as np
import pytest
from PIL import Image

import ref_resize16 as R
from datago_amd import synth

pytestmark = pytest.mark.gpu

CTYPES = {0: 1, 2: 3, 4: 2, 6: 4}  # colour type -> samples per pixel
KW = dict(crop_and_resize=True, default_image_size=128, downsampling_ratio=16, min_aspect_ratio=0.5,
          max_aspect_ratio=2.0)
KW_SMALL = dict(KW, default_image_size=32, downsampling_ratio=8)
KW_WIDE = dict(KW, default_image_size=256, downsampling_ratio=32)


def _lib():
    from datago_amd import _lib as L
    return L


def _ctx(kw=KW, **more):
    return _lib().Context(0, png16=True, resize16=True, **kw, **more)


@pytest.fixture(scope="module")
def ctx():
    return _ctx()


def _rand(rng, w, h, spp):
    return rng.integers(0, 65536, size=(h, w, spp), dtype=np.uint16)


def _bucket(c, w, h, forced=-1):
    """(index, bw, bh) of the bucket an image of w x h lands on."""
    b = c.buckets.closest(w, h) if forced < 0 else forced
    bw, bh, _ = c.buckets.get(b)
    return b, bw, bh


def _check(res, src, want, c, forced=-1, channels=None):
    """status, meta and pixels of one resized 16-bit image (src: the file's samples, want: the restatement's)."""
    L = _lib()
    st, arr, m = res
    assert st == L.DG_OK, (L.STATUS_NAMES.get(st, st), L.last_error())
    h, w = src.shape[:2]
    b, bw, bh = _bucket(c, w, h, forced)
    ch = want.shape[2]
    assert arr.dtype == np.uint16 and arr.shape == (bh, bw, ch)
    assert (m.width, m.height, m.original_width, m.original_height, m.bucket) == (bw, bh, w, h, b)
    assert (m.channels, m.bit_depth, m.is_encoded, m.nbytes) == (channels or ch, 16, 0, 2 * bw * bh * ch)
    np.testing.assert_array_equal(arr, want)


def test_default_off():
    L = _lib()
    rng = np.random.default_rng(1620)
    px = _rand(rng, 150, 97, 3)
    data = synth.encode_png16(px, 2, rng)
    c = L.Context(0, png16=True, **KW)
    assert c.decode_batch([data])[0][0] == L.DG_ERR_UNSUPPORTED and "16-bit resize" in L.last_error()
    assert c.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    c.set_option("resize16", 1)
    b, bw, bh = _bucket(c, 150, 97)
    assert c.output_size(data) == (L.DG_OK, 2 * bw * bh * 3)
    want = R.resize_to_fill(px, bw, bh)
    _check(c.decode_batch([data])[0], px, want, c)
    c.set_option("resize16", 0)  # and off again
    assert c.decode_batch([data])[0][0] == L.DG_ERR_UNSUPPORTED
    assert c.output_size(data)[0] == L.DG_ERR_UNSUPPORTED and "16-bit resize" in L.last_error()
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            c.set_option("resize16", bad)
        assert e.value.status == L.DG_ERR_INVALID and "resize16" in L.last_error()
    # the option alone does nothing: without png16 a 16-bit PNG stays on the CPU path
    alone = L.Context(0, resize16=True, **KW)
    assert alone.decode_batch([data])[0][0] == L.DG_ERR_UNSUPPORTED


# (label, W, H, samples per pixel, bucket (w, h) or None for the closest, property of (w2, h2, x0, y0))
SWEEP = [
    ("down1.3-cropx", 171, 166, 1, (128, 128), lambda W, H, g: g[2] > 0 and 1.25 < H / g[1] < 1.35),
    ("down2.5-cropy", 321, 331, 1, (128, 128), lambda W, H, g: g[3] > 0 and 2.4 < W / g[0] < 2.6),
    ("down1.7-rgb-cropx", 299, 293, 3, (80, 176), lambda W, H, g: g[2] > 0 and 1.6 < H / g[1] < 1.7),
    ("up1.6-odd-remainder", 81, 77, 1, (128, 128), lambda W, H, g: g[0] - 128 == 7 and g[2] == 3),
    ("axis-ratio-1", 80, 175, 2, (80, 176), lambda W, H, g: g[0] == W and g[1] == 176 != H),
    ("pure-crop-y", 128, 133, 3, (128, 128), lambda W, H, g: g[:2] == (W, H) and g[3] == 2),
    ("pure-crop-x", 139, 128, 4, (128, 128), lambda W, H, g: g[:2] == (W, H) and g[2] == 5),
    ("thin-3x200", 3, 200, 1, None, lambda W, H, g: g[1] > 20 * H),
    ("thin-200x3", 200, 3, 1, None, lambda W, H, g: g[0] > 20 * W),
    ("odd-211x173-rgba", 211, 173, 4, None, lambda W, H, g: True),
    ("odd-97x151-la", 97, 151, 2, None, lambda W, H, g: True),
]


def _forced(c, wh):
    if wh is None:
        return -1
    return next(i for i, (w, h, _) in enumerate(c.buckets.buckets()) if (w, h) == wh)


def test_geometry_sweep(ctx):
    rng = np.random.default_rng(1621)
    ct_of = {v: k for k, v in CTYPES.items()}
    files, cases = [], []
    for label, w, h, spp, wh, prop in SWEEP:
        px = _rand(rng, w, h, spp)
        f = _forced(ctx, wh)
        b, bw, bh = _bucket(ctx, w, h, f)
        assert prop(w, h, R.geometry(w, h, bw, bh)), (label, R.geometry(w, h, bw, bh))
        files.append(synth.encode_png16(px, ct_of[spp], rng))
        cases.append((label, px, f, R.resize_to_fill(px, bw, bh)))
    res = ctx.decode_batch(files, [f for _, _, f, _ in cases])
    for (label, px, f, want), r in zip(cases, res):
        try:
            _check(r, px, want, ctx, f)
        except AssertionError as e:
            raise AssertionError(f"{label}: {e}") from None


def test_steep_downscales_and_wide_output():
    """~7x and ~9.5x downscales (about 43 and 58 taps per output) on the 32 / 8 buckets,
    and an output of more than 256 columns (two workgroups per row of the
    horizontal pass) from a source of more than 1024 samples per row (two per
    row of the vertical pass) on the 256 / 32 buckets."""
    rng = np.random.default_rng(1622)
    small = _ctx(KW_SMALL)
    srcs = [_rand(rng, 230, 224, 1), _rand(rng, 305, 310, 3)]
    files = [synth.encode_png16(p, {1: 0, 3: 2}[p.shape[2]], rng) for p in srcs]
    for px, r in zip(srcs, small.decode_batch(files)):
        h, w = px.shape[:2]
        _, bw, bh = _bucket(small, w, h)
        g = R.geometry(w, h, bw, bh)
        assert w / g[0] > 6.5
        _check(r, px, R.resize_to_fill(px, bw, bh), small)
    wide = _ctx(KW_WIDE)
    px = _rand(rng, 300, 141, 4)
    b, bw, bh = _bucket(wide, 300, 141)
    assert bw > 256 and 300 * 4 > 1024
    _check(wide.decode_batch([synth.encode_png16(px, 6, rng)])[0], px, R.resize_to_fill(px, bw, bh), wide)


def test_colour_types_trns_adam7(ctx):
    rng = np.random.default_rng(1623)
    w, h = 150, 97
    _, bw, bh = _bucket(ctx, w, h)
    files, cases = [], []
    for ct, spp in CTYPES.items():
        px = _rand(rng, w, h, spp)
        files.append(synth.encode_png16(px, ct, rng, filters="random"))
        cases.append((f"type{ct}", px, px))
    # tRNS: the key becomes a 16-bit alpha channel, which resizes like any other (no premultiply)
    g = _rand(rng, w, h, 1)
    g[rng.integers(0, 3, size=(h, w)) == 0] = 0x12A5
    files.append(synth.encode_png16(g, 0, rng, trns=[0x12A5]))
    cases.append(("trns-gray", g, np.concatenate([g, np.where(g == 0x12A5, 0, 65535).astype(np.uint16)], axis=2)))
    k3 = np.array([0x0102, 0xFFFE, 0x8000], np.uint16)
    c3 = _rand(rng, w, h, 3)
    c3[rng.integers(0, 3, size=(h, w)) == 0] = k3
    a3 = np.where((c3 == k3).all(axis=2, keepdims=True), 0, 65535).astype(np.uint16)
    files.append(synth.encode_png16(c3, 2, rng, trns=list(k3)))
    cases.append(("trns-rgb", c3, np.concatenate([c3, a3], axis=2)))
    a7 = _rand(rng, w, h, 4)
    files.append(synth.encode_png16(a7, 6, rng, interlace=True))
    cases.append(("adam7-rgba", a7, a7))
    # 0 / 65535 checkerboard of 8-pixel squares: Lanczos overshoots both ways at every edge
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy // 8 + xx // 8) & 1) * 65535).astype(np.uint16).reshape(h, w, 1)
    files.append(synth.encode_png16(board, 0, rng))
    cases.append(("checkerboard", board, board))
    want_board = R.resize_to_fill(board, bw, bh)
    assert (want_board == 0).any() and (want_board == 65535).any()  # the clamp is exercised
    for (label, src, dec), r in zip(cases, ctx.decode_batch(files)):
        try:
            _check(r, src, R.resize_to_fill(dec, bw, bh), ctx, channels=dec.shape[2])
        except AssertionError as e:
            raise AssertionError(f"{label}: {e}") from None


def test_image_to_rgb8_and_encoders():
    L = _lib()
    rng = np.random.default_rng(1624)
    srcs = [_rand(rng, 150, 97, spp) for spp in (1, 2, 3, 4)] + [_rand(rng, 128, 133, 3)]  # the last: a pure crop
    files = [synth.encode_png16(p, {1: 0, 2: 4, 3: 2, 4: 6}[p.shape[2]], rng) for p in srcs]
    c8 = _ctx(image_to_rgb8=True)
    want = []
    for px, (st, arr, m) in zip(srcs, c8.decode_batch(files)):
        assert st == L.DG_OK, L.last_error()
        h, w = px.shape[:2]
        _, bw, bh = _bucket(c8, w, h)
        want.append(R.to_rgb8(R.resize_to_fill(px, bw, bh)))
        assert arr.dtype == np.uint8 and arr.shape == (bh, bw, 3)
        assert (m.channels, m.bit_depth, m.nbytes, m.width, m.height) == (3, 8, 3 * bw * bh, bw, bh)
        assert (m.original_width, m.original_height) == (w, h)
        np.testing.assert_array_equal(arr, want[-1])
    # an encoder never sees 16-bit samples ...
    enc = _ctx(pre_encode_images=True)
    assert enc.decode_batch(files[:1])[0][0] == L.DG_ERR_UNSUPPORTED
    assert "16-bit image to an encoder" in L.last_error()
    # ... but the resized RGB8 reaches it as any RGB8 image does
    encp = _ctx(pre_encode_images=True, image_to_rgb8=True, encode_format=0)
    for w8, (st, buf, m) in zip(want, encp.decode_batch(files)):
        assert st == L.DG_OK and m.is_encoded == 1
        back = Image.open(io.BytesIO(buf.tobytes()))
        assert back.mode == "RGB"
        np.testing.assert_array_equal(np.array(back), w8)


def test_mixed_batch_and_alone(ctx):
    L = _lib()
    rng = np.random.default_rng(1625)
    files = [synth.make_png(1800 + i, 150, 97, kind) for i, kind in enumerate(synth.PNG_KINDS)]
    files += [synth.make_png(1850, 140, 130, "RGBA", interlace=True), synth.make_jpeg(1851, 300, 200)]
    n8 = len(files)
    deep = [(_rand(rng, 171, 166, spp), ct) for ct, spp in CTYPES.items()]
    deep.append((_rand(rng, 128, 133, 1), 0))  # a pure crop
    files += [synth.encode_png16(px, ct, rng) for px, ct in deep]
    order = rng.permutation(len(files))  # 16-bit files between the others
    got = ctx.decode_batch([files[i] for i in order])
    ref = L.Context(0, **KW).decode_batch([files[i] for i in order])
    for k, i in enumerate(order):
        if i < n8:  # 8-bit images resize exactly as a context without the options resizes them
            assert got[k][0] == L.DG_OK and ref[k][0] == L.DG_OK
            assert got[k][1].dtype == np.uint8 and got[k][2].bit_depth == 8
            np.testing.assert_array_equal(got[k][1], ref[k][1])
        else:
            px = deep[i - n8][0]
            assert ref[k][0] == L.DG_ERR_UNSUPPORTED
            _, bw, bh = _bucket(ctx, px.shape[1], px.shape[0])
            _check(got[k], px, R.resize_to_fill(px, bw, bh), ctx)
            st, arr, _ = ctx.decode_batch([files[i]])[0]  # alone: the same samples as in the batch
            assert st == L.DG_OK
            np.testing.assert_array_equal(arr, got[k][1])


def test_aligned_sample():
    """samples.py: a depth map rides beside its JPEG and lands on the JPEG's
    bucket, also where its own closest bucket is another."""
    from datago_amd import samples as S
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    L = _lib()
    rng = np.random.default_rng(1626)
    cfg = ImageTransformConfig(crop_and_resize=True, default_image_size=128, downsampling_ratio=16,
                               min_aspect_ratio=0.5, max_aspect_ratio=2.0)
    tfm = ARAwareTransform(cfg, 0, png16=True, resize16=True)
    jpg = synth.make_jpeg(1860, 300, 200)
    depth = _rand(rng, 300, 200, 1)  # the size of its photo
    mask = _rand(rng, 150, 160, 1)   # another shape: its own closest bucket is not the photo's
    k = tfm.table.closest(300, 200)
    bw, bh, _ = tfm.table.get(k)
    assert tfm.table.closest(150, 160) != k
    sample = S.TarballSample("s", [S.BinaryFile("a.jpg", jpg),
                                   S.BinaryFile("a.depth.png", synth.encode_png16(depth, 0, rng)),
                                   S.BinaryFile("a.mask.png", synth.encode_png16(mask, 0, rng))])
    out = S.process_sample(sample, tfm, ImageEncoding())
    assert out is not None and not out.unsupported
    assert (out.image.width, out.image.height, out.image.bit_depth) == (bw, bh, 8)
    for name, px in (("a.depth.png", depth), ("a.mask.png", mask)):
        p = out.additional_images[name]
        assert (p.width, p.height, p.channels, p.bit_depth) == (bw, bh, 1, 16)
        assert (p.original_width, p.original_height) == (px.shape[1], px.shape[0])
        np.testing.assert_array_equal(p.to_numpy_array(), R.resize_to_fill(px, bw, bh)[:, :, 0])
    # without the flag the 16-bit members go back to the caller's CPU path
    off = S.process_sample(sample, ARAwareTransform(cfg, 0, png16=True), ImageEncoding())
    assert set(off.unsupported) == {"a.depth.png", "a.mask.png"}
    assert all(st == L.DG_ERR_UNSUPPORTED for st in off.unsupported.values())


def test_entry_points(ctx):
    import torch
    L = _lib()
    rng = np.random.default_rng(1627)
    px = _rand(rng, 171, 166, 3)
    data = synth.encode_png16(px, 2, rng)
    _, bw, bh = _bucket(ctx, 171, 166)
    want = R.resize_to_fill(px, bw, bh)
    _check(ctx.decode_one(data), px, want, ctx)
    buf = np.empty(2 * want.size, np.uint8)
    st, arr, m = ctx.decode_one(data, out=buf)
    _check((st, arr, m), px, want, ctx)
    assert arr.ctypes.data == buf.ctypes.data  # a view of the caller's bytes
    st, t, m = ctx.decode_batch_torch([data])[0]
    assert st == L.DG_OK and t.dtype == torch.uint16 and t.is_cuda and tuple(t.shape) == want.shape
    assert m.bit_depth == 16
    np.testing.assert_array_equal(t.cpu().numpy(), want)
    buf[:] = 0
    ticket, metas, keep = ctx.submit_host([data], [buf])
    ctx.wait(ticket)
    np.testing.assert_array_equal(L.payload_array(buf, metas[0]), want)


def test_budget_split_allocates_nothing_later():
    L = _lib()
    rng = np.random.default_rng(1628)
    srcs = [_rand(rng, 300 - 7 * i, 290 + 3 * i, 4) for i in range(8)]
    files = [synth.encode_png16(p, 6, rng) for p in srcs]

    def fresh():
        c = _ctx()
        c.set_option("coef_cache_mb", 0)
        return c
    def exact_mb(datas):  # footprint at exact sizes: no growth headroom, no prewarmed idle slots
        r = fresh()
        r.set_option("budget_plan", 0)
        r.set_option("max_device_mb", 1 << 20)
        assert all(st == L.DG_OK for st, _, _ in r.decode_batch(datas))
        mb = r.stat("peak_device_mb")
        r.close()
        return mb
    base, one = exact_mb([synth.make_jpeg(1, 32, 32, 90)]), exact_mb(files[:1])
    budget = base + max(8, 3 * (one - base))  # a few of the eight images at a time
    c = fresh()
    c.set_option("max_device_mb", budget)
    want = []
    for p in srcs:
        _, bw, bh = _bucket(c, p.shape[1], p.shape[0])
        want.append(R.resize_to_fill(p, bw, bh))
    for r, p, w in zip(c.decode_batch(files), srcs, want):
        _check(r, p, w, c)
    assert c.stat("budget_splits") > 0
    a0, f0 = c.stat("allocs"), c.stat("budget_frees")
    for rep in range(2):
        for r, p, w in zip(c.decode_batch(files), srcs, want):
            _check(r, p, w, c)
    assert c.stat("allocs") == a0, (a0, c.stat("allocs"))
    assert c.stat("budget_frees") == f0
    assert c.stat("peak_device_mb") <= budget + 16, (c.stat("peak_device_mb"), budget)
    c.close()
