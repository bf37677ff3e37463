"""The 16-bit PNG re-encode (context option "penc16") pinned on the CPU:

  1. the reference (tests/ref_penc16.py) against readers that share nothing
     with it -- its own spec-level reader for every colour type, PIL (I;16)
     for gray -- and the properties the case set (tests/penc16_cases.py) is
     there for;
  2. the shared header the kernel runs (datago_amd/csrc/dg_penc16.h, built for
     the CPU through tests/native/penc16_emu.cpp) against the reference's
     filter types and filtered stream, for equality;
  3. the same sources as a program of their own under ASan + UBSan.
"""
import ctypes
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import penc16_cases as C
import ref_penc
import ref_penc16 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "penc16_emu.cpp")
SO = os.path.join(NATIVE, "libpenc16_emu.so")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "dg_penc16.h"), os.path.join(CSRC, "dg_types.h")]

CASES = C.all_cases()
BY_LABEL = dict(CASES)


# ------------------------------------------------------------------ 1. the reference and the set

@pytest.mark.parametrize("dynamic", [False, True], ids=["fixed", "dynamic"])
def test_reference_files_read_back(dynamic):
    for label, px in CASES:
        r = C.ref(label, px, dynamic)
        got = R.read(r.file)
        assert got.colour_type == R.COLOUR_TYPE[px.shape[2]], label
        np.testing.assert_array_equal(got.px, px, err_msg=label)
        np.testing.assert_array_equal(got.filters, r.filters, err_msg=label)
        assert got.stream.tobytes() == r.stream.tobytes(), label
        assert r.file[24] == 16, label  # IHDR bit depth
        if px.shape[2] == 1:
            im = Image.open(io.BytesIO(r.file))
            assert im.mode == "I;16", (label, im.mode)
            np.testing.assert_array_equal(np.array(im), px[:, :, 0], err_msg=label)
        if dynamic:  # the shorter of the two blocks
            assert len(r.file) <= len(C.ref(label, px).file), label
            assert r.dyn or r.file == C.ref(label, px).file, label


def _matches(stream):
    return [(p, k) for p, k in ref_penc.parse(stream) if k]


def test_set_properties():
    refs = {label: C.ref(label, px) for label, px in CASES}
    # filters: all five on rows after the first, Sub, Average and None on row 0
    assert {int(t) for r in refs.values() for t in r.filters[1:]} == {0, 1, 2, 3, 4}
    assert {int(r.filters[0]) for r in refs.values()} >= {0, 1, 3}
    assert int(refs[C.ROW0_NONE].filters[0]) == 0
    for spp in (1, 2, 3, 4):  # ... and per samples per pixel among the content cases
        own = [refs[l] for l, px in C.content_cases() if px.shape[2] == spp]
        assert {int(t) for r in own for t in r.filters[1:]} == {0, 1, 2, 3, 4}, spp
    # shapes: 1 x 1, one row, one column and width 2 for every spp
    shapes = {(px.shape[0], px.shape[1], px.shape[2]) for _, px in CASES}
    for spp in (1, 2, 3, 4):
        assert {(1, 1, spp), (1, 70, spp), (70, 1, spp)} <= shapes
        assert any(s[1] == 2 and s[2] == spp for s in shapes)
    # row bytes on both sides of and on 64, 128 and 256; more than one step of the wave (256 row bytes)
    rbs = {2 * px.shape[1] * px.shape[2] for _, px in CASES if px.shape[0] > 1}
    for edge in (64, 128, 256):
        assert {edge - 2, edge, edge + 2} <= rbs, edge
    assert any(rb > 512 for rb in rbs)
    assert any(rb % 4 == 2 for rb in rbs)  # a last quad of two bytes
    # rows that start 2 bytes off a dword: an odd number of samples per row, more than one row
    assert any(px.shape[0] > 1 and (px.shape[1] * px.shape[2]) % 2 == 1 and px.shape[2] == spp
               for _, px in CASES for spp in (1, 3))
    # 0x80 in the filtered rows
    s = refs[C.HIT80_LABEL]
    rows = s.stream.reshape(len(s.filters), -1)[:, 1:]
    assert (rows == 0x80).any()
    # stream lengths beside 1024 and 2048
    lens = {label: len(refs[label].stream) for label in C.STREAM_LENGTHS}
    assert sorted(lens.values()) == [1023, 1025, 2047, 2049], lens
    # a 258-long match, one that starts on a piece edge, one cut by an edge (the run goes on behind it)
    m = [(label, p, k, refs[label].stream) for label in refs for p, k in _matches(refs[label].stream)]
    assert any(k == 258 for _, _, k, _ in m)
    assert any(p % 1024 == 0 for _, p, _, _ in m)
    assert any((p + k) % 1024 == 0 and p + k < len(s) and s[p + k] == s[p + k - 1] and k < 258 for _, p, k, s in m)


def test_byte_order_and_neighbours_show():
    """The split-ramp cases tell the mistakes apart.  A neighbour taken 1 or bpp / 2 bytes back changes the
    filter choice and the bytes.  Swapped sample bytes change the bytes only: the filters work per byte lane
    of a pixel, so exchanging two lanes permutes every candidate row and leaves all five sums as they were."""
    px = BY_LABEL[C.ALT_LABEL]
    assert set(np.unique(px).tolist()) == {0x00FF, 0xFF00}
    for label in C.SPLIT_LABELS:
        px = BY_LABEL[label]
        rows = R.be_rows(px)
        h, w, bpp = rows.shape
        t0, s0 = ref_penc.filter_rows(rows)
        swapped = rows.reshape(h, w, bpp // 2, 2)[..., ::-1].reshape(h, w, bpp)
        t1, s1 = ref_penc.filter_rows(swapped)
        assert not np.array_equal(s0, s1), label
        back = s1[:, 1:].reshape(h, w, bpp // 2, 2)[..., ::-1].reshape(h, -1)
        assert np.array_equal(t0, t1) and np.array_equal(back, s0[:, 1:]), label  # (the permutation, as said)
        for wrong in {1, bpp // 2}:
            t2, s2 = ref_penc.filter_rows(rows.reshape(h, w * bpp // wrong, wrong))
            assert not np.array_equal(t0, t2) and not np.array_equal(s0, s2), (label, wrong)
    # and a swap shows in the alternation case's bytes too
    rows = R.be_rows(BY_LABEL[C.ALT_LABEL])
    assert not np.array_equal(rows, rows.reshape(8, 21, 2, 2)[..., ::-1].reshape(8, 21, 4))


# ------------------------------------------------------------------ 2. the shared header

def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in DEPS):
        tmp = f"{out}.{os.getpid()}.tmp"  # build beside it and rename: never a half-written file
        subprocess.run(["g++", "-O2", "-std=c++17", "-I" + CSRC, "-o", tmp, SRC] + extra, check=True)
        os.replace(tmp, out)


@pytest.fixture(scope="module")
def emu():
    _build(SO, ["-fPIC", "-shared"])
    lib = ctypes.CDLL(SO)
    p, u = ctypes.c_void_p, ctypes.c_uint32
    lib.p16e_filter.argtypes = [p, u, u, u, u, p, p]
    lib.p16e_filter.restype = None
    return lib


def _emu_filter(lib, px, shift):
    h, w, spp = px.shape
    px = np.ascontiguousarray(px)
    types, stream = np.zeros(h, np.uint8), np.full(h * (2 * w * spp + 1), 0xEE, np.uint8)
    lib.p16e_filter(px.ctypes.data, h, w, spp, shift, types.ctypes.data, stream.ctypes.data)
    return types, stream


def test_header_against_reference(emu):
    for label, px in CASES:
        r = C.ref(label, px)
        for shift in (0, 1):  # the encoder's own placement, and the rows' alignment classes exchanged
            types, stream = _emu_filter(emu, px, shift)
            np.testing.assert_array_equal(types, r.filters, err_msg=f"{label} shift {shift}: filter types")
            if not np.array_equal(stream, r.stream):
                p = int(np.flatnonzero(stream != r.stream)[0])
                rl = 2 * px.shape[1] * px.shape[2] + 1
                raise AssertionError(f"{label} shift {shift}: stream differs from position {p} (row {p // rl}, "
                                     f"byte {p % rl - 1}): {stream[p]:#x} against {r.stream[p]:#x}")


def test_header_on_random_images(emu):
    rng = np.random.default_rng(1670)
    for i in range(60):
        h, w, spp = int(rng.integers(1, 9)), int(rng.integers(1, 150)), int(rng.integers(1, 5))
        kind = i % 3
        if kind == 0:
            px = rng.integers(0, 65536, size=(h, w, spp), dtype=np.uint16)
        elif kind == 1:  # smooth with small noise: the depth-map shape
            px = (C.plane(h, w, spp).astype(np.int64) + rng.integers(-40, 41, size=(h, w, spp))).astype(np.uint16)
        else:  # few values: ties between filters
            px = rng.choice(np.array([0, 0x0100, 0x00FF, 0x8000, 0x7FFF], np.uint16), size=(h, w, spp))
        types, rows = ref_penc.filter_rows(R.be_rows(px))
        got_t, got_s = _emu_filter(emu, px, i & 1)
        np.testing.assert_array_equal(got_t, types, err_msg=f"random {i} {px.shape}")
        np.testing.assert_array_equal(got_s, rows.reshape(-1), err_msg=f"random {i} {px.shape}")


# ------------------------------------------------------------------ 3. under the sanitizers

def test_header_program_under_sanitizers(tmp_path):
    """The same sources as a program of their own under ASan + UBSan (alignment of every load included), every
    case at both placements; its answers are checked too."""
    san = str(tmp_path / "penc16_san")  # (not kept beside the sources: rebuilt per run, a few seconds)
    _build(san, ["-DP16_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    path = tmp_path / "cases.bin"
    want = []
    with open(path, "wb") as fh:
        for label, px in CASES:
            for shift in (0, 1):
                fh.write(struct.pack("<4I", *px.shape, shift) + np.ascontiguousarray(px).tobytes())
                want.append((label, C.ref(label, px)))
    res = subprocess.run([san, str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(want)
    for (label, r), line in zip(want, lines):
        types, stream = line.split(" ")
        assert types == "".join(str(int(t)) for t in r.filters), label
        assert stream == r.stream.tobytes().hex(), label
