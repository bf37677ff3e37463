"""16-bit PNG support, the parts that need no GPU: the test writer
(synth.encode_png16) pinned against PIL, the 16-to-8 reduction of
image_to_rgb8, and dg_probe, which describes the default options."""
import io

import numpy as np
import pytest
from PIL import Image

from datago_amd import synth

W, H = 67, 70


def _pil(data: bytes) -> np.ndarray:
    return np.array(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("interlace", [False, True])
def test_writer_gray16_reads_back_exactly(interlace):
    rng = np.random.default_rng(16)
    px = rng.integers(0, 65536, size=(H, W, 1), dtype=np.uint16)
    data = synth.encode_png16(px, 0, rng, filters="random", interlace=interlace)
    im = Image.open(io.BytesIO(data))
    assert im.mode.startswith("I;16") and im.size == (W, H)
    got = np.array(im)
    assert got.dtype == np.uint16
    np.testing.assert_array_equal(got, px[:, :, 0])


@pytest.mark.parametrize("interlace", [False, True])
def test_writer_rgb16_high_bytes(interlace):
    # PIL reduces RGB16 to the high byte of every sample
    rng = np.random.default_rng(17)
    px = rng.integers(0, 65536, size=(H, W, 3), dtype=np.uint16)
    data = synth.encode_png16(px, 2, rng, filters="random", interlace=interlace)
    np.testing.assert_array_equal(_pil(data), (px >> 8).astype(np.uint8))


def test_writer_trns_chunk_is_big_endian():
    rng = np.random.default_rng(18)
    px = rng.integers(0, 65536, size=(3, 5, 1), dtype=np.uint16)
    data = synth.encode_png16(px, 0, rng, trns=[0x1234])
    i = data.index(b"tRNS")
    assert data[i - 4:i] == b"\x00\x00\x00\x02" and data[i + 4:i + 6] == b"\x12\x34"
    assert data[8 + 8 + 8] == 16 and data[8 + 8 + 9] == 0  # IHDR depth, colour type


def test_to_rgb8_reduction_is_round_to_nearest():
    # image's u16 -> u8 conversion as image_to_rgb8 applies it: (v + 128) / 257
    v = np.arange(65536, dtype=np.int64)
    a = (v + 128) // 257
    # round(v * 255 / 65535) in exact integer arithmetic (no tie exists: 65535 is odd)
    b = (2 * v * 255 + 65535) // (2 * 65535)
    np.testing.assert_array_equal(a, b)
    assert a[0] == 0 and a[-1] == 255


def test_probe_reports_default_options():
    # dg_probe takes no context: a 16-bit file stays outside the default GPU path
    from datago_amd import _lib as L
    rng = np.random.default_rng(19)
    px = rng.integers(0, 65536, size=(5, 8, 3), dtype=np.uint16)
    st, info = L.probe(synth.encode_png16(px, 2, rng))
    assert st == L.DG_OK
    assert (info.format, info.width, info.height, info.bit_depth) == (L.DG_FMT_PNG, 8, 5, 16)
    assert info.gpu_supported == 0
