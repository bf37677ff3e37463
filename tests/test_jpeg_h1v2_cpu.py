"""4:4:0-style JPEGs (context option "jpeg_h1v2") without a GPU: the reference
module tests/ref_jpeg_h1v2.py is pinned against Pillow (libjpeg-turbo) in
decode_semantics 0, baseline and progressive, and against the oracle in both
semantics on layouts the oracle accepts; the header parser's allow_h1v2 flag;
the entropy emulator on 4:4:0 files."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_craft as J
import ref_jpeg_h1v2 as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SO = os.path.join(NATIVE, "libh1v2_emu.so")

SIZES = [(1, 1), (2, 33), (3, 5), (5, 2), (9, 17), (37, 29), (131, 67)]
RESTARTS = [0, 1, 3]
OLD_WHY = b"chroma sampling other than 4:4:4/4:2:2/4:2:0"


def _pil(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _case(samp, w, h, rst):
    comps, qtabs, tq = R.craft(samp, w, h, seed=w + rst, quality=(50, 90, 100)[rst % 3])
    data = R.baseline(comps, samp, w, h, qtabs, tq, restart=rst, tables="optimal" if rst == 1 else "std")
    return comps, qtabs, tq, data


@pytest.mark.parametrize("name", list(R.H1V2_LAYOUTS))
def test_baseline_reference_equals_pillow(name):
    samp = R.H1V2_LAYOUTS[name]
    n = 0
    for w, h in SIZES:
        for rst in RESTARTS:
            comps, qtabs, tq, data = _case(samp, w, h, rst)
            ref = R.decode(comps, samp, w, h, qtabs, tq, 0)
            pil = _pil(data)
            assert ref.shape == pil.shape == (h, w, 3), (w, h, rst)
            assert np.array_equal(ref, pil), (w, h, rst, int((ref != pil).sum()))
            n += 1
    assert n == len(SIZES) * len(RESTARTS)  # no case skipped


@pytest.mark.parametrize("w,h", [(9, 17), (131, 67)])
def test_progressive_reference_equals_pillow(w, h):
    samp = R.H1V2_LAYOUTS["440"]
    comps, qtabs, tq = R.craft(samp, w, h, seed=w, quality=90)
    data = R.progressive(comps, samp, w, h, qtabs, tq)
    ref = R.decode(R.visible_coefs(comps, samp, w, h), samp, w, h, qtabs, tq, 0)
    pil = _pil(data)
    assert np.array_equal(ref, pil), int((ref != pil).sum())


@pytest.mark.parametrize("sem", [0, 1], ids=["libjpeg", "zune"])
@pytest.mark.parametrize("name", ["mixed_cb_full", "422_wide"])
def test_reference_equals_oracle_on_supported_layouts(name, sem):
    """The plane trick and the h2v1 / h2v2 restatements, where an oracle exists."""
    samp = J.LAYOUTS[name][0]
    for w, h in [(1, 1), (3, 5), (5, 2), (9, 17), (37, 29), (131, 67)]:
        for rst in (0, 3):
            comps, qtabs, tq, data = _case(samp, w, h, rst)
            with O.semantics(sem):
                st, dec = O.jpeg_decode(data)
            assert st == 0
            ref = R.decode(comps, samp, w, h, qtabs, tq, sem)
            assert np.array_equal(ref, dec), (w, h, rst, int((ref != dec).sum()))


@pytest.fixture(scope="module")
def native():
    srcs = [os.path.join(NATIVE, "h1v2_emu.cpp"), os.path.join(ROOT, "datago_amd", "csrc", "host", "jpeg_header.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu.cpp")] + [os.path.join(ROOT, "datago_amd", "csrc", f)
                                                       for f in ("dg_entropy.h", "dg_types.h", "host/jpeg_header.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"  # build beside it and rename (parallel test workers)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "datago_amd", "csrc"), "-I" + NATIVE, "-o", tmp] + srcs, check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    E.h1v2_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    E.h1v2_set_allow.argtypes = [ctypes.c_int]
    E.emu_set_lead.argtypes = [ctypes.c_uint32]
    E.emu_decode_coefs.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int16),
                                   ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int64)]
    return E


def _parse(E, data, allow):
    why = ctypes.create_string_buffer(128)
    return E.h1v2_parse(data, len(data), allow, why, 128), why.value


def test_parser_flag(native):
    for name, samp in R.H1V2_LAYOUTS.items():
        for w, h in ((3, 5), (131, 67)):
            data = _case(samp, w, h, 0)[3]
            assert _parse(native, data, 0) == (J.UNSUPPORTED, OLD_WHY), name
            assert _parse(native, data, 1) == (J.OK, b""), name
    comps, qtabs, tq = R.craft(R.H1V2_LAYOUTS["440"], 9, 17)
    prog = R.progressive(comps, R.H1V2_LAYOUTS["440"], 9, 17, qtabs, tq)
    assert _parse(native, prog, 0) == (J.UNSUPPORTED, OLD_WHY)
    assert _parse(native, prog, 1) == (J.OK, b"")
    d411 = J.layout_jpeg("411", 37, 29)
    assert _parse(native, d411, 1) == (J.UNSUPPORTED, OLD_WHY)
    assert _parse(native, d411, 0) == (J.UNSUPPORTED, OLD_WHY)
    assert _parse(native, J.layout_jpeg("420_wide12", 37, 29), 1)[0] == J.CORRUPT
    ok = J.layout_jpeg("mixed_cb_full", 37, 29)  # untouched by the flag
    assert _parse(native, ok, 0) == _parse(native, ok, 1) == (J.OK, b"")


@pytest.mark.parametrize("rst", RESTARTS)
@pytest.mark.parametrize("sub_bits", [128, 1024])
def test_emulated_entropy_decode_of_440(native, sub_bits, rst):
    samp = R.H1V2_LAYOUTS["440"]
    comps, qtabs, tq, data = _case(samp, 131, 67, rst)
    want = np.zeros((sum(c.shape[0] * c.shape[1] for c in comps), 64), np.int16)
    n = 0
    for mcu in J._mcus(comps, samp):  # MCU order; zigzag -> natural
        for _, z in mcu:
            want[n, J.ZIGZAG] = z
            n += 1
    cap = 1 << 12
    out = np.zeros((cap, 64), np.int16)
    nb = ctypes.c_size_t()
    st = (ctypes.c_int64 * 8)()
    native.emu_set_lead(0)
    native.h1v2_set_allow(0)
    args = (data, len(data), sub_bits, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), cap, ctypes.byref(nb), st)
    assert native.emu_decode_coefs(*args) == J.UNSUPPORTED  # default options
    native.h1v2_set_allow(1)
    try:
        assert native.emu_decode_coefs(*args) == 0
    finally:
        native.h1v2_set_allow(0)
    assert nb.value == n == want.shape[0]
    assert np.array_equal(out[:n], want)
    assert st[5] == 0  # write pass exit == next subsequence's entry everywhere
    assert st[7] == n
