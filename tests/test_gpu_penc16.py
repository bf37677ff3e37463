"""16-bit PNGs re-encoded on the GPU (context option "penc16" beside "png16" /
"resize16"): k_penc_filter16 in front of the PNG re-encoder's byte stages.

Expected files come from tests/ref_penc16.py (the format's restatement over
the big-endian bytes; test_penc16_cpu.py pins it and the case set) and every
comparison is equality.  Files that went through the transform are read by
ref_penc16.read (PIL keeps only gray16 exact) and compared with what the same
context returns un-encoded.  Contexts are small: 128 / 16 and 32 / 8 buckets."""
import numpy as np
import pytest

import penc16_cases as C
import ref_penc16 as R
import ref_resize16 as R16
from datago_amd import synth

pytestmark = pytest.mark.gpu

FMT_PNG, FMT_JPEG = 0, 1
CT = R.COLOUR_TYPE  # samples per pixel -> colour type
KW = dict(crop_and_resize=True, default_image_size=128, downsampling_ratio=16, min_aspect_ratio=0.5,
          max_aspect_ratio=2.0)
KW_SMALL = dict(KW, default_image_size=32, downsampling_ratio=8)
CASES = C.all_cases()
_inputs = {}


def _lib():
    from datago_amd import _lib as L
    return L


def _enc_ctx(dynamic=False, kw=None, **more):
    """pre-encoding as PNG with the 16-bit chain on; kw: a transform's parameters (none: images keep their size)."""
    return _lib().Context(0, png16=True, resize16=True, penc16=True, penc_dynamic=dynamic, pre_encode_images=True,
                          encode_format=FMT_PNG, **(kw or {}), **more)


def _input(label, px):
    if label not in _inputs:
        _inputs[label] = synth.encode_png16(px, CT[px.shape[2]], np.random.default_rng(len(_inputs)))
    return _inputs[label]


def _rand(rng, w, h, spp):
    return rng.integers(0, 65536, size=(h, w, spp), dtype=np.uint16)


def _depth(rng, w, h, spp):
    """Smooth with +-40 noise: what a depth map looks like to the filters."""
    return (C.plane(h, w, spp).astype(np.int64) + rng.integers(-40, 41, size=(h, w, spp))).astype(np.uint16)


def _same(got, exp, label):
    assert got == exp, f"{label}: {R.first_difference(got, exp)}"


def _ok(res, label=""):
    L = _lib()
    st, buf, m = res
    assert st == L.DG_OK, (label, L.STATUS_NAMES.get(st, st), L.last_error())
    return buf.tobytes(), m


# ------------------------------------------------------------------ 1. default off

def test_default_off():
    L = _lib()
    rng = np.random.default_rng(1680)
    px = _depth(rng, 37, 21, 1)
    data = synth.encode_png16(px, 0, rng)
    c = L.Context(0, png16=True, pre_encode_images=True, encode_format=FMT_PNG)

    def refused(ctx, what):
        assert ctx.decode_batch([data])[0][0] == L.DG_ERR_UNSUPPORTED
        assert what in L.last_error(), L.last_error()
        assert ctx.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
        assert what in L.last_error(), L.last_error()
    refused(c, "16-bit image to an encoder")
    c.set_option("penc16", 1)
    st, cap = c.output_size(data)
    assert st == L.DG_OK
    got, m = _ok(c.decode_batch([data])[0])
    _same(got, R.encode(px).file, "on")
    assert len(got) <= cap
    c.set_option("penc16", 0)  # and off again
    refused(c, "16-bit image to an encoder")
    for bad in (2, -1):
        with pytest.raises(L.DgError) as e:
            c.set_option("penc16", bad)
        assert e.value.status == L.DG_ERR_INVALID and "penc16" in L.last_error() and str(bad) in L.last_error()
    # the option alone does nothing: without png16 a 16-bit PNG stays on the CPU path
    alone = L.Context(0, penc16=True, pre_encode_images=True, encode_format=FMT_PNG)
    assert alone.decode_batch([data])[0][0] == L.DG_ERR_UNSUPPORTED
    assert alone.output_size(data)[0] == L.DG_ERR_UNSUPPORTED
    # the JPEG encoder takes 8-bit samples only, as the reference's does
    jpg = L.Context(0, png16=True, penc16=True, pre_encode_images=True, encode_format=FMT_JPEG)
    refused(jpg, "JPEG encoder")
    jpg.set_option("penc16", 0)  # option off: the message existing callers read
    refused(jpg, "16-bit image to an encoder")


# ------------------------------------------------------------------ 2. bytes

@pytest.mark.parametrize("dynamic", [False, True], ids=["fixed", "dynamic"])
def test_bytes(dynamic):
    """Every case through a context with no transform: the encoder's input is the file's samples."""
    ctx = _enc_ctx(dynamic)
    order = np.random.default_rng(1681).permutation(len(CASES))
    cases = [CASES[i] for i in order]
    failed = []
    for (label, px), res in zip(cases, ctx.decode_batch([_input(*c) for c in cases])):
        got, m = _ok(res, label)
        assert (m.width, m.height, m.nbytes) == (px.shape[1], px.shape[0], len(got)), label
        exp = C.ref(label, px, dynamic).file
        if got != exp:
            failed.append(f"{label}: {R.first_difference(got, exp)}")
    assert not failed, f"{len(failed)} of {len(cases)} files differ; first: {failed[0]}"


# ------------------------------------------------------------------ 3. through the transform

def _transform_sources(rng):
    """(label, samples): per colour type one resized source, one pure crop, one image of its bucket's size."""
    out = []
    for spp in (1, 2, 3, 4):
        out += [(f"resized_s{spp}", _depth(rng, 50 + spp, 31, spp)),   # -> 40 x 24: both passes
                (f"crop_s{spp}", _depth(rng, 32, 35, spp)),            # 32 x 32 out of it: no pass
                (f"bucket_s{spp}", _depth(rng, 32, 32, spp))]          # its bucket's size: k_copy
    return out


@pytest.mark.parametrize("dynamic", [False, True], ids=["fixed", "dynamic"])
def test_through_the_transform(dynamic):
    L = _lib()
    rng = np.random.default_rng(1682)
    srcs = _transform_sources(rng)
    files = [synth.encode_png16(px, CT[px.shape[2]], rng) for _, px in srcs]
    enc = _enc_ctx(dynamic, KW_SMALL)  # (small outputs: the Python reference encodes every one)
    raw = L.Context(0, png16=True, resize16=True, **KW_SMALL)
    kinds = set()
    for (label, px), e, r in zip(srcs, enc.decode_batch(files), raw.decode_batch(files)):
        got, m = _ok(e, label)
        st, arr, mr = r
        assert st == L.DG_OK, (label, L.last_error())
        h, w, spp = px.shape
        bw, bh, _ = enc.buckets.get(enc.buckets.closest(w, h))
        back = R.read(got)
        assert back.colour_type == CT[spp], (label, back.colour_type)  # LA16 stays colour type 4
        np.testing.assert_array_equal(back.px, arr, err_msg=label)
        assert arr.shape == (bh, bw, spp) and arr.dtype == np.uint16
        if label.startswith("resized"):
            assert (w, h) != (bw, bh) and R16.geometry(w, h, bw, bh)[:2] != (w, h), label
            np.testing.assert_array_equal(arr, R16.resize_to_fill(px, bw, bh), err_msg=label)
        elif label.startswith("crop"):
            assert (w, h) != (bw, bh) and R16.geometry(w, h, bw, bh)[:2] == (w, h), label
        else:
            assert (w, h) == (bw, bh), label
            np.testing.assert_array_equal(arr, px, err_msg=label)
        # and byte for byte the reference's file of those samples
        _same(got, R.encode(arr, dynamic).file, label)
        kinds.add(label.split("_")[0])
    assert kinds == {"resized", "crop", "bucket"}


# ------------------------------------------------------------------ 4. meta and sizes

def test_meta_sizes_and_entry_points():
    L = _lib()
    rng = np.random.default_rng(1683)
    srcs = [_depth(rng, 171, 166, 1), _depth(rng, 97, 151, 2), _depth(rng, 128, 128, 3), _depth(rng, 139, 128, 4)]
    files = [synth.encode_png16(px, CT[px.shape[2]], rng) for px in srcs]
    ctx = _enc_ctx(True, KW)
    batch = []
    for px, d, res in zip(srcs, files, ctx.decode_batch(files)):
        got, m = _ok(res)
        h, w, spp = px.shape
        b = ctx.buckets.closest(w, h)
        bw, bh, _ = ctx.buckets.get(b)
        assert (m.channels, m.bit_depth, m.is_encoded) == (-1, 16, 1)
        assert (m.width, m.height, m.original_width, m.original_height, m.bucket) == (bw, bh, w, h, b)
        st, cap = ctx.output_size(d)
        assert st == L.DG_OK and m.nbytes == len(got) <= cap
        assert cap < (1 << 29) and cap > 2 * bw * bh * spp  # the bound is the 16-bit stream's
        batch.append(got)
    # host-out with exactly output_size bytes per image
    caps = [ctx.output_size(d)[1] for d in files]
    outs = [np.full(c, 0xA5, np.uint8) for c in caps]
    ticket, metas, keep = ctx.submit_host(files, outs)
    ctx.wait(ticket)
    for want, o, m in zip(batch, outs, metas):
        assert m.status == L.DG_OK and m.nbytes == len(want), (m.status, L.last_error())
        assert o[:m.nbytes].tobytes() == want and (o[m.nbytes:] == 0xA5).all()
    del keep
    # dg_decode_one
    for want, d in zip(batch, files):
        st, buf, m = ctx.decode_one(d)
        assert st == L.DG_OK and (m.channels, m.bit_depth, m.is_encoded, m.nbytes) == (-1, 16, 1, len(want))
        assert buf.tobytes() == want


# ------------------------------------------------------------------ 5. mixed batch

def test_mixed_batch_and_alone():
    L = _lib()
    rng = np.random.default_rng(1684)
    files = [synth.make_jpeg(1880, 300, 200), synth.make_jpeg(1881, 97, 150, gray=True)]
    files += [synth.make_png(1882 + i, 150, 97, kind) for i, kind in enumerate(synth.PNG_KINDS)]
    n8 = len(files)
    deep = [_depth(rng, 171, 166, 1), _depth(rng, 150, 97, 2), _rand(rng, 128, 133, 3), _depth(rng, 128, 128, 4),
            _depth(rng, 3, 200, 1)]
    files += [synth.encode_png16(px, CT[px.shape[2]], rng) for px in deep]
    files.append(synth.encode_png16(_rand(rng, 128, 128, 1), 0, rng, filters="5"))  # corrupt: found on the GPU
    order = rng.permutation(len(files))
    ctx = _enc_ctx(True, KW)
    base = L.Context(0, png16=True, resize16=True, penc_dynamic=True, pre_encode_images=True, encode_format=FMT_PNG, **KW)
    got = ctx.decode_batch([files[i] for i in order])
    ref = base.decode_batch([files[i] for i in order])
    for k, i in enumerate(order):
        if i == len(files) - 1:
            assert got[k][0] == L.DG_ERR_CORRUPT, got[k][0]
            continue
        g, m = _ok(got[k], f"member {i}")
        alone, _ = _ok(ctx.decode_batch([files[i]])[0], f"member {i} alone")
        assert g == alone, i
        if i < n8:  # 8-bit members: what a context without the option produces
            r, mr = _ok(ref[k], f"member {i} without the option")
            assert g == r and m.bit_depth == 8, i
        else:
            assert ref[k][0] == L.DG_ERR_UNSUPPORTED
            px = deep[i - n8]
            bw, bh, _ = ctx.buckets.get(ctx.buckets.closest(px.shape[1], px.shape[0]))
            want = px if (px.shape[1], px.shape[0]) == (bw, bh) else R16.resize_to_fill(px, bw, bh)
            back = R.read(g)
            np.testing.assert_array_equal(back.px, want, err_msg=f"member {i}")
            assert m.bit_depth == 16 and back.colour_type == CT[px.shape[2]]


# ------------------------------------------------------------------ 6. stale arena

def test_stale_arena():
    """One slot: the bit buffer is OR-ed into, the histograms are added to.  A large batch of dense streams, then
    a few sparse ones at other offsets, then dense ones again, all against the reference."""
    ctx = _enc_ctx(True)
    ctx.set_option("slots", 1)
    dense = [c for c in CASES if c[0].startswith(("noise", "runavg", "plane", "rb", "1x70", "70x1", "n"))]
    sparse = [c for c in CASES if c[0].startswith(("flat", "1x1", "w2", "hit80", "row0"))][::-1]
    assert len(dense) >= 25 and len(sparse) >= 10

    def run(cases):
        for (label, px), res in zip(cases, ctx.decode_batch([_input(*c) for c in cases])):
            got, _ = _ok(res, label)
            _same(got, C.ref(label, px, True).file, label)
    run(dense)
    run(sparse)
    run(dense[5:15])
    run(sparse[3:] + dense[:4])


# ------------------------------------------------------------------ 7. aligned sample

def test_aligned_sample():
    """samples.py: a depth map rides beside its JPEG, both pre-encoded as PNG on the photo's bucket."""
    from datago_amd import samples as S
    from datago_amd.image_processing import ARAwareTransform, EncodeFormat, ImageEncoding, ImageTransformConfig
    L = _lib()
    rng = np.random.default_rng(1686)
    cfg = ImageTransformConfig(crop_and_resize=True, default_image_size=128, downsampling_ratio=16,
                               min_aspect_ratio=0.5, max_aspect_ratio=2.0)
    tfm = ARAwareTransform(cfg, 0, png16=True, resize16=True, penc16=True, penc_dynamic=True)
    enc = ImageEncoding(encode_images=True, encode_format=EncodeFormat.PNG)
    jpg = synth.make_jpeg(1890, 300, 200)
    depth = _depth(rng, 300, 200, 1)
    k = tfm.table.closest(300, 200)
    bw, bh, _ = tfm.table.get(k)
    sample = S.TarballSample("s", [S.BinaryFile("a.jpg", jpg),
                                   S.BinaryFile("a.depth.png", synth.encode_png16(depth, 0, rng))])
    out = S.process_sample(sample, tfm, enc)
    assert out is not None and not out.unsupported, out and out.unsupported
    img = out.image
    assert (img.width, img.height, img.channels, img.bit_depth, img.is_encoded) == (bw, bh, -1, 8, True)
    assert img.data[:8] == b"\x89PNG\r\n\x1a\n"
    p = out.additional_images["a.depth.png"]
    assert (p.width, p.height, p.channels, p.bit_depth, p.is_encoded) == (bw, bh, -1, 16, True)
    assert (p.original_width, p.original_height) == (300, 200)
    back = R.read(p.data)
    assert back.colour_type == 0
    np.testing.assert_array_equal(back.px, R16.resize_to_fill(depth, bw, bh))
    # without the flag the depth map goes back to the caller's CPU path, the photo still encodes
    off = S.process_sample(sample, ARAwareTransform(cfg, 0, png16=True, resize16=True), enc)
    assert off.unsupported == {"a.depth.png": L.DG_ERR_UNSUPPORTED} and off.image.is_encoded


# ------------------------------------------------------------------ 8. budget

def test_budget_split_allocates_nothing_later():
    L = _lib()
    rng = np.random.default_rng(1687)
    srcs = [_depth(rng, 300 - 7 * i, 290 + 3 * i, 4) for i in range(8)]
    files = [synth.encode_png16(p, 6, rng) for p in srcs]

    def fresh():
        c = _enc_ctx(True, KW)
        c.set_option("coef_cache_mb", 0)
        return c

    def exact_mb(datas):  # footprint at exact sizes: no growth headroom, no prewarmed idle slots
        r = fresh()
        r.set_option("budget_plan", 0)
        r.set_option("max_device_mb", 1 << 20)
        res = r.decode_batch(datas)
        assert all(st == L.DG_OK for st, _, _ in res), L.last_error()
        mb = r.stat("peak_device_mb")
        r.close()
        return mb, [buf.tobytes() for _, buf, _ in res]
    base, _ = exact_mb([synth.make_jpeg(1, 32, 32, 90)])
    one, _ = exact_mb(files[:1])
    _, want = exact_mb(files)  # the unsplit run
    budget = base + max(8, 3 * (one - base))  # a few of the eight images at a time
    c = fresh()
    c.set_option("budget_plan", 1)
    c.set_option("max_device_mb", budget)
    for res, w in zip(c.decode_batch(files), want):
        assert _ok(res)[0] == w
    assert c.stat("budget_splits") > 0
    a0, f0 = c.stat("allocs"), c.stat("budget_frees")
    for rep in range(2):
        for res, w in zip(c.decode_batch(files), want):
            assert _ok(res)[0] == w
    assert c.stat("allocs") == a0, (a0, c.stat("allocs"))
    assert c.stat("budget_frees") == f0
    assert c.stat("peak_device_mb") <= budget + 16, (c.stat("peak_device_mb"), budget)
    c.close()
