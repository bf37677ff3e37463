"""A mixed batch with failing images between the good ones decodes every image
exactly as a submit of that image alone does.

What a batch carries from one image to the next -- subsequence and checkpoint
bases, inflate chunk and unfilter flag numbers, blob offsets of palettes and
encoder headers, the shift of the aliased late region, the walk over the
planned images that skips the failed ones -- must not leak into an image's
result.  The comparison is bytes to bytes against the same library, through
the host path and the device-pointer path: no tolerance."""
import numpy as np
import pytest

from datago_amd import synth

pytestmark = pytest.mark.gpu

BUCKETS = dict(crop_and_resize=True, default_image_size=64, downsampling_ratio=8, min_aspect_ratio=0.5,
               max_aspect_ratio=2.0)
# (id, context config): the transform alone, and with either encoder behind it
CONFIGS = [("raw", {}), ("enc_png", dict(pre_encode_images=True, encode_format=0)),
           ("enc_jpeg", dict(pre_encode_images=True, encode_format=1))]


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def images():
    """[(name, file, good, sixteen)]: none larger than 96 x 64, the three that
    fail planning first, in the middle and near the end."""
    rng = np.random.default_rng(4242)
    noise = rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    deep = rng.integers(0, 65536, size=(64, 64, 1), dtype=np.uint16)
    good = [
        ("jpeg_gray", synth.make_jpeg(1, 90, 61, 85, gray=True)),
        ("jpeg_444", synth.make_jpeg(2, 77, 64, 90, "4:4:4")),
        ("jpeg_420", synth.make_jpeg(3, 96, 64, 80, "4:2:0")),
        ("jpeg_restart", synth.make_jpeg(4, 95, 63, 88, "4:2:0", restart_marker_rows=1)),
        ("jpeg_progressive", synth.make_jpeg(5, 93, 58, 90, "4:2:0", progressive=True)),
        ("png_rgb", synth.make_png(6, 83, 59, "RGB")),
        ("png_palette", synth.make_png(7, 71, 64, "P8")),
        ("png_rgba_adam7", synth.make_png(8, 61, 47, "RGBA", interlace=True)),
        # incompressible: > 12 KiB of IDAT, three chunks at inf_chunk 4096
        ("png_noise_chunked", synth.encode_png(noise.reshape(64, 64 * 3), 64, 64, 8, 2, 3, rng, filters="none")),
        ("png_gray16", synth.encode_png16(deep, 0, rng)),  # a bucket's size: 16-bit images are never resized
        ("jpeg_422", synth.make_jpeg(9, 64, 96, 75, "4:2:2")),
    ]
    head = synth.make_jpeg(10, 80, 60, 90)
    bad = [("bad_truncated_header", head[:head.index(b"\xff\xc0") + 6]), ("bad_cmyk", synth.make_cmyk_jpeg(11, 72, 56)),
           ("bad_garbage", rng.integers(0, 256, size=700, dtype=np.uint8).tobytes())]
    order = [bad[0]] + good[:4] + [bad[1]] + good[4:9] + [bad[2]] + good[9:]
    return [(name, data, not name.startswith("bad_"), name == "png_gray16") for name, data in order]


def _ctx(cfg):
    ctx = _lib().Context(0, png16=True, **BUCKETS, **cfg)
    ctx.set_option("inf_chunk", 4096)
    ctx.set_option("prog_split", 0)  # the progressive member stays in the batch, between the others
    return ctx


def _meta(m):
    return tuple(getattr(m, f) for f, _ in _lib().PayloadMeta._fields_)


def _bytes(arr):
    if arr is None:
        return None
    if not isinstance(arr, np.ndarray):  # a device tensor (uint16 ones as the bytes they are)
        import torch
        arr = arr.contiguous().view(torch.uint8).cpu().numpy()
    return np.ascontiguousarray(arr).tobytes()


@pytest.mark.parametrize("cfg", [c for _, c in CONFIGS], ids=[i for i, _ in CONFIGS])
def test_batch_matches_each_image_alone(images, cfg):
    L = _lib()
    if cfg:  # the encoders take the 8-bit images
        images = [im for im in images if not im[3]]
    assert len(images) >= 13 and not images[0][2]
    datas = [data for _, data, _, _ in images]
    alone_ctx, batch_ctx = _ctx(cfg), _ctx(cfg)
    alone = [alone_ctx.decode_batch([d])[0] for d in datas]  # one submit per image
    for (name, _, good, _), (st, arr, m) in zip(images, alone):
        assert (st == L.DG_OK) == good, (name, L.STATUS_NAMES.get(st, st))
        assert m.status == st
    assert alone_ctx.stat("png_chunks") > 0
    resized = sum(1 for _, (st, _, m) in zip(images, alone)
                  if st == L.DG_OK and (m.width, m.height) != (m.original_width, m.original_height))
    assert resized >= 8
    c0 = batch_ctx.stat("png_chunks")
    for path, res in (("host", batch_ctx.decode_batch(datas)), ("device", batch_ctx.decode_batch_torch(datas))):
        for (name, _, good, _), (st, arr, m), (st1, arr1, m1) in zip(images, res, alone):
            assert st == st1, (path, name, L.STATUS_NAMES.get(st, st), L.STATUS_NAMES.get(st1, st1))
            assert _meta(m) == _meta(m1), (path, name)
            assert _bytes(arr) == _bytes(arr1), (path, name)
    assert batch_ctx.stat("png_chunks") > c0
    alone_ctx.close()
    batch_ctx.close()
