"""The destuff count and write passes (k_destuff_count, k_destuff_write: a wave
per 4 KiB chunk, four chunks staged per workgroup and stored in row runs) at
their edges, bit-exact against the oracle in both decode semantics:

  * a 64 x 64 4:2:0 image and a 384 x 384 4:4:4 noise image at quality 100
    (a scan of 300-400 KB: more than three workgroup spans of 16 KiB), each
    without restart markers, with one per MCU and with one per MCU row;
  * every one of them behind 0..15 bytes of APPn payload, so that the scan
    starts at every address mod 16;
  * a stream with more than 10% stuffed bytes (coefficients whose codes and
    extra bits are runs of ones);
  * all of them in one batch with a gray image and a scan shorter than 64
    bytes, through dg_submit and dg_submit_device, each compared with the
    same file decoded alone;
  * option destuff_one (which shares the host lists and destuff16) gives the
    same bytes.
"""
import numpy as np
import pytest

import jpeg_craft as J
from datago_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEMS = [0, 1]
SEM_IDS = ["libjpeg", "zune"]
WG_SPAN = 4 * 4096  # raw bytes per workgroup of the count and write passes


def _lib():
    from datago_amd import _lib as L
    return L


def _pad(data, k):
    """`data` with an APP15 segment of k payload bytes after SOI: 4 + k more header bytes."""
    assert data[:2] == b"\xff\xd8"
    return data[:2] + b"\xff\xef" + (2 + k).to_bytes(2, "big") + bytes(range(1, k + 1)) + data[2:]


def _scan(data):
    """The entropy-coded bytes between the SOS header and EOI."""
    i = 2
    while data[i + 1] != 0xDA:
        i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    assert data[-2:] == b"\xff\xd9"
    return data[i:-2]


def _dense():
    """4:4:4, every AC coefficient 127 or 255 with unit quantisation: codes 11111000 / 1111110110 and 7 / 8 one bits."""
    rng = np.random.default_rng(77)
    samp = [(1, 1)] * 3
    comps = []
    for bh, bw in J.geometry(samp, 128, 128):
        z = rng.choice([127, 255], size=(bh, bw, 64)).astype(np.int64)
        z[:, :, 0] = rng.integers(-200, 200, size=(bh, bw))
        comps.append(z)
    ones = [[1] * 64, [1] * 64]
    return J.from_coefs(comps, samp, 128, 128, ones)


@pytest.fixture(scope="module")
def bases():
    """[(label, file)]: the unpadded images."""
    rng = np.random.default_rng(2024)
    small = synth.synth_pixels(rng, 64, 64)
    noise = (128 + rng.normal(0, 12, size=(384, 384, 3))).clip(0, 255).astype(np.uint8)  # sigma 12: ~360 KB of scan
    out = []
    for tag, kw in (("", {}), (" rst1", dict(restart_marker_blocks=1)), (" rstrow", dict(restart_marker_rows=1))):
        out.append(("small420" + tag, synth.encode_jpeg(small, 90, "4:2:0", **kw)))
        out.append(("noise444" + tag, synth.encode_jpeg(noise, 100, "4:4:4", **kw)))
    out.append(("dense", _dense()))
    by = dict(out)
    assert 300_000 <= len(_scan(by["noise444"])) <= 400_000
    assert all(len(_scan(by[k])) > 3 * WG_SPAN for k in by if k.startswith("noise444"))
    assert by["noise444 rst1"].count(b"\xff\xd0") > 100 and b"\xff\xdd" in by["small420 rstrow"]
    s = _scan(by["dense"])
    assert s.count(b"\xff\x00") > 0.10 * len(s) and len(s) > 3 * WG_SPAN, (s.count(b"\xff\x00"), len(s))
    return out


@pytest.fixture(scope="module")
def refs(bases):
    """{(label, sem): the oracle's pixels}, computed once."""
    out = {}
    for sem in SEMS:
        with O.semantics(sem):
            for label, data in bases:
                st, out[(label, sem)] = O.jpeg_decode(data)
                assert st == 0, label
    return out


@pytest.fixture(scope="module")
def padded(bases):
    """[(label, pad, file)]: every image behind 0..15 payload bytes."""
    return [(label, k, _pad(data, k)) for label, data in bases for k in range(16)]


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_every_scan_address_exact(padded, refs, sem):
    ctx = _lib().Context(0, decode_semantics=sem)
    res = ctx.decode_batch([d for _, _, d in padded])
    for (label, k, _), (st, arr, _) in zip(padded, res):
        ref = refs[(label, sem)]
        assert st == 0, (label, k, st)
        assert arr.shape == ref.shape, (label, k)
        assert np.array_equal(arr, ref), (label, k, int((arr != ref).sum()))
    assert ctx.stat("write_mismatch") == 0
    ctx.close()


def _bytes(arr):
    if not isinstance(arr, np.ndarray):  # a device tensor
        arr = arr.contiguous().cpu().numpy()
    return np.ascontiguousarray(arr).tobytes()


@pytest.fixture(scope="module")
def mixed(padded):
    gray = synth.make_jpeg(5, 150, 97, 85, gray=True)
    tiny = synth.encode_jpeg(np.full((8, 8), 128, np.uint8), 90)
    assert 0 < len(_scan(tiny)) < 64
    datas = [d for _, _, d in padded]
    datas.insert(7, gray)
    datas.insert(60, tiny)
    datas.append(_pad(tiny, 3))
    return datas


def test_mixed_batch_matches_alone_host_and_device(mixed):
    alone_ctx, ctx = _lib().Context(0), _lib().Context(0)
    alone = [alone_ctx.decode_batch([d])[0] for d in mixed]
    assert all(st == 0 for st, _, _ in alone)
    for path, res in (("host", ctx.decode_batch(mixed)), ("device", ctx.decode_batch_torch(mixed))):
        for i, ((st, arr, _), (_, arr1, _)) in enumerate(zip(res, alone)):
            assert st == 0, (path, i, st)
            assert _bytes(arr) == _bytes(arr1), (path, i)
    assert ctx.stat("write_mismatch") == 0 and alone_ctx.stat("write_mismatch") == 0
    alone_ctx.close()
    ctx.close()


def test_destuff_one_gives_the_same_bytes(mixed):
    ctx, one = _lib().Context(0), _lib().Context(0)
    one.set_option("destuff_one", 1)
    for i, ((st, a, _), (st1, b, _)) in enumerate(zip(ctx.decode_batch(mixed), one.decode_batch(mixed))):
        assert st == 0 and st1 == 0, (i, st, st1)
        assert np.array_equal(a, b), i
    assert one.stat("write_mismatch") == 0
    ctx.close()
    one.close()
