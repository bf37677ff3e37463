"""Four-component Adobe JPEGs (context option "jpeg_cmyk") without a GPU: the
reference module tests/ref_jpeg_cmyk.py is pinned against Pillow
(libjpeg-turbo) in decode_semantics 0 -- 255 - Pillow's CMYK image is the
planes in the stored convention -- baseline and progressive, on crafted files
and on files Pillow writes; the two facts about the blinn rule the GPU kernel
relies on; the header parser's allow_cmyk flag; dg_probe unchanged."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_craft as J
import ref_jpeg_cmyk as R
from datago_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SO = os.path.join(NATIVE, "libcmyk_parse.so")

SIZES = [(1, 1), (2, 33), (3, 5), (5, 2), (9, 17), (37, 29), (131, 67)]
RESTARTS = [0, 1, 3]
OLD_WHY = b"CMYK/2-component JPEG"
CASES = [(name, t) for name in R.CMYK_LAYOUTS for t in (0, 2)]


def _pil_planes(data):
    """Pillow's CMYK image, back in the stored convention (Pillow inverts Adobe files)."""
    im = Image.open(io.BytesIO(data))
    assert im.mode == "CMYK"
    return 255 - np.asarray(im)


def _case(samp, w, h, t, rst):
    comps, qtabs, tq = R.craft(samp, w, h, t, seed=w + rst, quality=(50, 90, 100)[rst % 3])
    data = R.baseline(comps, samp, w, h, qtabs, tq, t, restart=rst, tables="optimal" if rst == 1 else "std")
    return comps, qtabs, tq, data


@pytest.mark.parametrize("name,t", CASES, ids=["%s-t%d" % c for c in CASES])
def test_baseline_planes_equal_pillow(name, t):
    samp = R.CMYK_LAYOUTS[name]
    n = 0
    for w, h in SIZES:
        for rst in RESTARTS:
            comps, qtabs, tq, data = _case(samp, w, h, t, rst)
            ref = R.cmyk_planes(comps, samp, w, h, qtabs, tq, t, 0)
            pil = _pil_planes(data)
            assert ref.shape == pil.shape == (h, w, 4), (w, h, rst)
            assert np.array_equal(ref, pil), (w, h, rst, int((ref != pil).sum()))
            n += 1
    assert n == len(SIZES) * len(RESTARTS)  # no case skipped


@pytest.mark.parametrize("t", [0, 2])
@pytest.mark.parametrize("name", ["cmyk_444", "ycck_420", "k_sub"])
@pytest.mark.parametrize("w,h", [(9, 17), (131, 67)])
def test_progressive_planes_equal_pillow(w, h, name, t):
    samp = R.CMYK_LAYOUTS[name]
    comps, qtabs, tq = R.craft(samp, w, h, t, seed=w, quality=90)
    data = R.progressive(comps, samp, w, h, qtabs, tq, t)
    ref = R.cmyk_planes(R.visible_coefs(comps, samp, w, h), samp, w, h, qtabs, tq, t, 0)
    pil = _pil_planes(data)
    assert np.array_equal(ref, pil), int((ref != pil).sum())


def pillow_cmyk_file(w, h, seed, progressive=False, quality=90):
    """A CMYK JPEG as Pillow writes it (Adobe transform 0, all 1x1), with the planes Pillow reads back."""
    rng = np.random.default_rng(seed)
    px = np.concatenate([synth.synth_pixels(rng, w, h), synth.synth_pixels(rng, w, h)[:, :, :1]], axis=2)
    buf = io.BytesIO()
    Image.fromarray(px.astype(np.uint8), "CMYK").save(buf, "JPEG", quality=quality, progressive=progressive)
    return buf.getvalue()


@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
def test_pillow_written_file(native, progressive):
    """A foreign encoder's file: accepted by the parser as CMYK, and its coefficients, read back by the
    reference's own entropy-free route, are not needed -- Pillow's planes are the pin the GPU test uses."""
    data = pillow_cmyk_file(67, 45, 5, progressive)
    st, why, info = _parse(native, data, 1, 0)
    assert (st, why) == (J.OK, b""), why
    assert info[:2] == [4, 3]  # four components, CS_CMYK
    assert _parse(native, data, 0, 0)[:2] == (J.UNSUPPORTED, OLD_WHY)
    pl = _pil_planes(data)
    assert pl.shape == (45, 67, 4)
    rgb = R.rgb_of_planes(pl)
    # the rule against its closed form on a real image
    want = (pl[:, :, :3].astype(np.int64) * pl[:, :, 3:].astype(np.int64) + 127) // 255
    assert np.array_equal(rgb, want.astype(np.uint8))


def test_blinn_facts():
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    t = a * b + 128
    assert np.array_equal(R.blinn(a, b), (a * b + 127) // 255)  # all 65,536 pairs
    assert int((t + (t >> 8)).max()) == 65407 and int(t.max()) < 65536  # fits unsigned 16-bit lanes
    assert R.blinn(a, b).max() == 255 and R.blinn(a, b).min() == 0


@pytest.fixture(scope="module")
def native():
    srcs = [os.path.join(NATIVE, "cmyk_parse.cpp"), os.path.join(ROOT, "datago_amd", "csrc", "host", "jpeg_header.cpp")]
    deps = srcs + [os.path.join(ROOT, "datago_amd", "csrc", f) for f in ("dg_types.h", "host/jpeg_header.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"  # build beside it and rename (parallel test workers)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "datago_amd", "csrc"),
                        "-o", tmp] + srcs, check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    E.cmyk_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                             ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    return E


def _parse(E, data, cmyk, h1v2):
    why = ctypes.create_string_buffer(160)
    info = (ctypes.c_int * 4)()
    st = E.cmyk_parse(data, len(data), cmyk, h1v2, why, 160, info)
    return st, why.value, list(info)


def _small(name, t, **kw):
    samp = R.CMYK_LAYOUTS[name]
    comps, qtabs, tq = R.craft(samp, 37, 29, t, seed=3)
    return R.baseline(comps, samp, 37, 29, qtabs, tq, t, **kw)


def test_parser_accepts_with_the_flag(native):
    for name, samp in R.CMYK_LAYOUTS.items():
        need_h1v2 = name == "ycck_440"
        for t in (0, 2):
            data = _small(name, t)
            for h1v2 in (0, 1):
                assert _parse(native, data, 0, h1v2)[:2] == (J.UNSUPPORTED, OLD_WHY), name
            st, why, info = _parse(native, data, 1, 1)
            assert (st, why) == (J.OK, b""), (name, why)
            assert info == [4, 3 if t == 0 else 4, max(s[0] for s in samp), max(s[1] for s in samp)]
            st, why, _ = _parse(native, data, 1, 0)
            if need_h1v2:
                assert (st, why) == (J.UNSUPPORTED, b"chroma sampling other than 4:4:4/4:2:2/4:2:0")
            else:
                assert (st, why) == (J.OK, b"")
    samp = R.CMYK_LAYOUTS["ycck_420"]
    comps, qtabs, tq = R.craft(samp, 9, 17, 2)
    prog = R.progressive(comps, samp, 9, 17, qtabs, tq, 2)
    assert _parse(native, prog, 0, 0)[:2] == (J.UNSUPPORTED, OLD_WHY)
    assert _parse(native, prog, 1, 0)[:2] == (J.OK, b"")


def test_parser_refusals_with_the_flag(native):
    data = _small("cmyk_444", 0)
    adobe = data.index(b"Adobe")
    texts = set()
    # transform 1 with four components
    t1 = data[:adobe + 11] + b"\x01" + data[adobe + 12:]
    st, why, _ = _parse(native, t1, 1, 0)
    assert st == J.UNSUPPORTED and b"transform 1" in why
    texts.add(why)
    # no Adobe segment: the APP14 marker turned into a comment
    noadobe = data[:adobe - 3] + b"\xfe" + data[adobe - 2:]
    st, why, _ = _parse(native, noadobe, 1, 0)
    assert st == J.UNSUPPORTED and b"without an Adobe segment" in why
    texts.add(why)
    # two components
    samp2 = [(1, 1), (1, 1)]
    px = synth.synth_pixels(np.random.default_rng(1), 16, 16)
    qt = [np.full(64, 8), np.full(64, 8)]
    two = J.from_coefs(J.coefs_from_pixels(px, samp2, qt, [0, 1], ycc=False), samp2, 16, 16, qt, header="adobe")
    st, why, _ = _parse(native, two, 1, 0)
    assert st == J.UNSUPPORTED and why == b"2-component JPEG"
    assert _parse(native, two, 0, 0)[:2] == (J.UNSUPPORTED, OLD_WHY)
    texts.add(why)
    # more distinct Huffman tables than the entropy kernels' per-workgroup budget (6)
    many = _small("cmyk_444", 0, td=[0, 1, 2, 3], ta=[0, 1, 2, 3])
    st, why, _ = _parse(native, many, 1, 0)
    assert st == J.UNSUPPORTED and b"more distinct Huffman tables" in why
    texts.add(why)
    six = _small("cmyk_444", 0, td=[0, 1, 2, 0], ta=[0, 1, 2, 1])  # three DC + three AC: inside the budget
    assert _parse(native, six, 1, 0)[:2] == (J.OK, b"")
    assert len(texts) == 4 and OLD_WHY not in texts  # each refusal has a text of its own
    # 4:1:1-style ratios and too many blocks per MCU stay refused
    samp = [(4, 1), (1, 1), (1, 1), (4, 1)]
    comps, qtabs, tq = R.craft(samp, 37, 29, 2)
    st, why, _ = _parse(native, R.baseline(comps, samp, 37, 29, qtabs, tq, 2), 1, 1)
    assert st == J.UNSUPPORTED and why == b"chroma sampling other than 4:4:4/4:2:2/4:2:0"
    for samp in ([(2, 2)] * 4, [(2, 2), (2, 2), (2, 2), (1, 1)]):  # 16 and 13 blocks per MCU (T.81: at most 10)
        comps, qtabs, tq = R.craft(samp, 37, 29, 0)
        st, why, _ = _parse(native, R.baseline(comps, samp, 37, 29, qtabs, tq, 0), 1, 1)
        assert (st, why) == (J.CORRUPT, b"too many blocks per MCU")


def test_three_component_files_untouched_by_the_flag(native):
    for name in ("444", "420", "adobe_rgb_444", "gray"):
        if name not in J.LAYOUTS:
            continue
        d = J.layout_jpeg(name, 37, 29)
        assert _parse(native, d, 0, 0) == _parse(native, d, 1, 0), name


def test_probe_describes_the_default_options():
    from datago_amd import _lib as L
    for data in (_small("cmyk_444", 0), _small("ycck_420", 2), pillow_cmyk_file(40, 30, 1)):
        st, info = L.probe(data)
        assert st == L.DG_OK and info.components == 4 and info.gpu_supported == 0
