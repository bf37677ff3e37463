"""The 16-bit resize's restatement (tests/ref_resize16.py) pinned on the CPU:
against Pillow's float Lanczos (same real-valued filter, its own tap window
and more precision: geometry, centre and normalisation), on cases with exact
answers, and against the shared header the kernels run
(datago_amd/csrc/dg_resize16.h through tests/native/resize16_emu.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import ref_resize16 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SO = os.path.join(NATIVE, "libresize16_emu.so")

# (W, H) -> (bw, bh)
SIZES = [((97, 61), (64, 48)), ((40, 30), (64, 48)), ((200, 64), (64, 48)), ((301, 299), (48, 64))]


def _noise(rng, w, h, c=1):
    return rng.integers(0, 65536, size=(h, w, c), dtype=np.uint16)


def _sine(w, h):
    y, x = np.mgrid[0:h, 0:w]
    v = 32767.5 + 32767.5 * np.sin(x / 7.3) * np.cos(y / 5.1)
    return np.clip(np.rint(v), 0, 65535).astype(np.uint16).reshape(h, w, 1)


@pytest.fixture(scope="module")
def images():
    """One noise and one sine field per source size, and their restated results (computed once)."""
    rng = np.random.default_rng(1610)
    out = []
    for (w, h), (bw, bh) in SIZES:
        for kind, px in (("noise", _noise(rng, w, h)), ("sine", _sine(w, h))):
            out.append((f"{kind}-{w}x{h}", px, bw, bh, R.resize_to_fill(px, bw, bh)))
    return out


def test_against_pillow(images):
    for cid, px, bw, bh, got in images:
        h, w, _ = px.shape
        w2, h2, x0, y0 = R.geometry(w, h, bw, bh)
        big = Image.fromarray(px[:, :, 0].astype(np.float32)).resize((w2, h2), Image.LANCZOS)
        t = np.clip(np.asarray(big, np.float64), 0.0, 65535.0)
        r = np.trunc(t)
        want = (r + ((t - r) >= 0.5)).astype(np.int64)[y0:y0 + bh, x0:x0 + bw]
        diff = np.abs(got[:, :, 0].astype(np.int64) - want)
        share = float((diff != 0).mean())
        print(f"{cid}: max {int(diff.max())} level(s), {100 * share:.2f}% of samples differ")
        # same real-valued filter, rounding errors far below half a level: never more than one level apart
        assert diff.max() <= 1, cid
        assert share <= 0.10, cid


def test_pure_crop_is_exact():
    rng = np.random.default_rng(1611)
    px = _noise(rng, 64, 50, 3)
    assert R.geometry(64, 50, 64, 48) == (64, 50, 0, 1)
    np.testing.assert_array_equal(R.resize_to_fill(px, 64, 48), px[1:49])
    px = _noise(rng, 71, 48, 2)  # a crop on x with an odd remainder: (71 - 64) // 2
    assert R.geometry(71, 48, 64, 48) == (71, 48, 3, 0)
    np.testing.assert_array_equal(R.resize_to_fill(px, 64, 48), px[:, 3:67])


def test_crop_branches():
    # wider than the target: crop on x; taller: crop on y; odd remainders floor
    assert R.geometry(200, 64, 64, 48) == (150, 48, 43, 0)
    assert R.geometry(97, 61, 64, 48) == (76, 48, 6, 0)
    assert R.geometry(60, 101, 64, 48) == (64, 108, 0, 30)
    assert R.geometry(64, 53, 64, 48) == (64, 53, 0, 2)
    w2, h2, x0, y0 = R.geometry(301, 299, 48, 64)
    assert (w2, h2, x0, y0) == (64, 64, 8, 0)
    # round half away from zero in the scaled size: 3 x 2 -> r = 2.5 gives 7.5 -> 8
    assert R.geometry(3, 2, 5, 5)[:2] == (8, 5)


def test_thin_sources():
    rng = np.random.default_rng(1612)
    # one pixel wide: every H output has left = 0, right = 1, weight exactly 1
    col = _noise(rng, 1, 40)
    for left, w in R.taps(1, 5):
        assert left == 0 and w.tolist() == [1.0]
    out = R.resize_to_fill(col, 4, 16)  # r = 4: 4 x 160, crop on y
    assert out.shape == (16, 4, 1)
    assert (out == out[:, :1]).all()  # the one source column, replicated
    # two rows: left is clamped to [0, 1], right to [left + 1, 2]
    tp = R.taps(2, 12)
    assert all(0 <= left <= 1 and 1 <= len(w) <= 2 - left for left, w in tp)
    assert tp[0][0] == 0 and tp[-1][0] + len(tp[-1][1]) == 2
    two = _noise(rng, 30, 2)
    assert R.resize_to_fill(two, 16, 8).shape == (8, 16, 1)
    # a constant image stays constant: the weights sum to 1 within rounding
    flat = np.full((2, 30, 1), 40000, np.uint16)
    assert np.abs(R.resize_to_fill(flat, 16, 8).astype(np.int64) - 40000).max() <= 1


ROUND_CASES = [(np.float32(0.5) - np.float32(2.0 ** -25), 0), (0.5, 1), (1.5, 2), (65534.5, 65535), (65535.0, 65535),
               (70000.0, 65535), (-3.0, 0), (0.49999, 0), (2.5, 3)]


def test_rounding():
    t = np.array([v for v, _ in ROUND_CASES], np.float32)
    assert float(t[0]) + 0.5 < 1.0 and np.float32(t[0] + np.float32(0.5)) == 1.0  # the floor(t + 0.5) trap
    assert R.round_sample(t).tolist() == [w for _, w in ROUND_CASES]


# ---- the shared header (what the kernels run) against the restatement

@pytest.fixture(scope="module")
def emu():
    src = os.path.join(NATIVE, "resize16_emu.cpp")
    deps = [src] + [os.path.join(ROOT, "datago_amd", "csrc", f) for f in ("dg_resize16.h", "dg_pixel.h", "dg_types.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"  # build beside it and rename: never a half-written library
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "datago_amd", "csrc"), "-o", tmp, src], check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    u32, pf = ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)
    pu16 = ctypes.POINTER(ctypes.c_uint16)
    E.r16e_geom.argtypes = [u32, u32, u32, u32, ctypes.POINTER(u32)]
    E.r16e_taps.argtypes = [u32, u32, u32, pf, ctypes.POINTER(ctypes.c_int32)]
    E.r16e_taps.restype = u32
    E.r16e_round.argtypes = [ctypes.c_float]
    E.r16e_round.restype = ctypes.c_uint16
    E.r16e_resize.argtypes = [pu16, u32, u32, u32, u32, u32, pu16]
    return E


def _emu_resize(E, px, bw, bh):
    h, w, c = px.shape
    src = np.ascontiguousarray(px)
    out = np.empty((bh, bw, c), np.uint16)
    pu16 = ctypes.POINTER(ctypes.c_uint16)
    assert E.r16e_resize(src.ctypes.data_as(pu16), w, h, c, bw, bh, out.ctypes.data_as(pu16)) == 1
    return out


# up and down scales: ratio 1, 16x down, 5x up, odd sizes, the thin sources
TAP_PAIRS = [(64, 64), (1024, 64), (13, 65), (97, 76), (61, 48), (40, 64), (30, 48), (200, 150), (301, 64),
             (299, 64), (1, 5), (2, 12), (333, 127), (7, 1)]


def test_header_taps_bit_identical(emu):
    for n_in, n_out in TAP_PAIRS:
        buf = np.empty(n_in, np.float32)
        left = ctypes.c_int32()
        for o, (rl, rw) in enumerate(R.taps(n_in, n_out)):
            n = emu.r16e_taps(n_in, n_out, o, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(left))
            assert (left.value, n) == (rl, len(rw)), (n_in, n_out, o)
            np.testing.assert_array_equal(buf[:n].view(np.uint32), rw.view(np.uint32), err_msg=f"{n_in}->{n_out} @{o}")


def test_header_geometry_and_rounding(emu):
    rng = np.random.default_rng(1613)
    cases = [(w, h, bw, bh) for (w, h), (bw, bh) in SIZES] + [(64, 50, 64, 48), (3, 2, 5, 5), (60, 101, 64, 48)]
    cases += [tuple(int(v) for v in rng.integers(1, 700, 4)) for _ in range(200)]
    for w, h, bw, bh in cases:
        g = (ctypes.c_uint32 * 4)()
        assert emu.r16e_geom(w, h, bw, bh, g) == 1
        assert tuple(g) == R.geometry(w, h, bw, bh), (w, h, bw, bh)
    for v, want in ROUND_CASES:
        assert emu.r16e_round(float(np.float32(v))) == want


def test_header_images_identical(emu, images):
    for cid, px, bw, bh, want in images:
        np.testing.assert_array_equal(_emu_resize(emu, px, bw, bh), want, err_msg=cid)
    rng = np.random.default_rng(1614)
    for c, (w, h, bw, bh) in [(3, (97, 61, 64, 48)), (4, (40, 30, 64, 48)), (2, (64, 50, 64, 48)), (1, (1, 40, 4, 16)),
                              (2, (30, 2, 16, 8))]:
        px = _noise(rng, w, h, c)
        np.testing.assert_array_equal(_emu_resize(emu, px, bw, bh), R.resize_to_fill(px, bw, bh))
