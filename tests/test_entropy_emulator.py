"""The GPU entropy decoder's algorithm (datago_amd/csrc/dg_entropy.h — the
product's own decode_range()) emulated sequentially on the CPU with the phase
structure of k_huff_sync / k_huff_fix / k_huff_scan / k_huff_write, checked
bit-exactly against the oracle's coefficients.  Catches logic errors in the
self-synchronising decode without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coef_patterns as P
import jpeg_craft as J
from datago_amd import synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SO = os.path.join(NATIVE, "libemu.so")


@pytest.fixture(scope="module")
def emu():
    srcs = [os.path.join(NATIVE, "emu.cpp"), os.path.join(ROOT, "datago_amd", "csrc", "host", "jpeg_header.cpp")]
    deps = srcs + [os.path.join(ROOT, "datago_amd", "csrc", f) for f in ("dg_entropy.h", "dg_types.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        # build beside it and rename: parallel test workers never load a half-written library
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "datago_amd", "csrc"), "-o", tmp] + srcs, check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    E.emu_set_lead.argtypes = [ctypes.c_uint32]
    E.emu_decode_coefs.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32,
                                   ctypes.POINTER(ctypes.c_int16), ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int64)]

    E.emu_multi_mismatch.restype = ctypes.c_int64
    E.emu_multi_checked.restype = ctypes.c_int64
    E.emu_two_mismatch.restype = ctypes.c_int64
    E.emu_two_checked.restype = ctypes.c_int64

    def run(data, sub_bits, lead=0):
        E.emu_set_lead(lead)
        run.multi0 = (E.emu_multi_mismatch(), E.emu_multi_checked())
        run.two0 = (E.emu_two_mismatch(), E.emu_two_checked())
        cap = 1 << 18
        out = np.zeros((cap, 64), np.int16)
        nb = ctypes.c_size_t()
        st = (ctypes.c_int64 * 8)()
        r = E.emu_decode_coefs(data, len(data), sub_bits, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                               cap, ctypes.byref(nb), st)
        run.multi = (E.emu_multi_mismatch() - run.multi0[0], E.emu_multi_checked() - run.multi0[1])
        run.two = (E.emu_two_mismatch() - run.two0[0], E.emu_two_checked() - run.two0[1])
        return r, out[: nb.value], list(st)
    return run


@pytest.mark.parametrize("seed", range(24))
@pytest.mark.parametrize("sub_bits,lead", [(128, 0), (1024, 0), (4096, 0), (512, 96), (1024, 2048), (4096, 6144)])
def test_emulated_parallel_decode_matches_oracle(emu, seed, sub_bits, lead):
    rng = np.random.default_rng(seed)
    w, h = int(rng.integers(1, 700)), int(rng.integers(1, 700))
    ss = ["4:2:0", "4:2:2", "4:4:4"][seed % 3]
    rst = [0, 0, 1, 3][seed % 4]
    data = synth.encode_jpeg(synth.synth_pixels(rng, w, h, seed % 7 == 0), int(rng.integers(30, 101)), ss,
                             restart_marker_rows=rst)
    st, ref = O.jpeg_coefs(data)
    r, co, stats = emu(data, sub_bits, lead)
    assert r == 0 and st == 0
    assert co.shape == ref.shape
    assert np.array_equal(co, ref)
    assert stats[5] == 0  # write pass exit == next subsequence's entry everywhere
    # k_huff_sync's multi-symbol lead-in (kMultiBits lookups) ends in the same state as single steps
    assert emu.multi[0] == 0, emu.multi
    # k_huff_sync2: two chains per lane in lockstep equal lead_in + decode_range per slot
    assert emu.two[0] == 0 and emu.two[1] > 0, emu.two


def _check(emu, data, sub_bits, lead):
    st, ref = O.jpeg_coefs(data)
    r, co, stats = emu(data, sub_bits, lead)
    assert r == 0 and st == 0
    assert co.shape == ref.shape
    assert np.array_equal(co, ref)
    assert stats[5] == 0
    assert emu.multi[0] == 0, emu.multi
    assert emu.two[0] == 0 and emu.two[1] > 0, emu.two


@pytest.fixture(scope="module")
def layout_files():
    """Every accepted layout of jpeg_craft.LAYOUTS: {(name, size, restart, q): bytes}."""
    return {(name, size, rst, q): J.layout_jpeg(name, *size, seed=7 + rst, quality=q, restart=rst)
            for name in J.OK_LAYOUTS for size in ((131, 67), (200, 150)) for rst in (0, 1, 3) for q in (50, 100)}


@pytest.mark.parametrize("sub_bits,lead", [(128, 0), (1024, 0), (512, 96)])
@pytest.mark.parametrize("name", J.OK_LAYOUTS)
def test_emulated_decode_of_crafted_layouts(emu, layout_files, name, sub_bits, lead):
    """Sampling layouts PIL does not write (general block order, gray with
    factors), with restart intervals of 0 / 1 / 3 MCUs at q 50 and 100; q 100
    with restart markers leaves empty trailing subsequences (the destuffed
    stream is more than a subsequence shorter than the raw scan)."""
    for key, data in layout_files.items():
        if key[0] == name:
            _check(emu, data, sub_bits, lead)


@pytest.mark.parametrize("sub_bits", [64, 128, 1024])
def test_emulated_decode_of_coefficient_patterns(emu, sub_bits):
    """All 256 part masks, all-64-nonzero blocks (spanning three or more
    64-bit subsequences) and all-zero blocks (tests/coef_patterns.py)."""
    for name, data in P.streams().items():
        _check(emu, data, sub_bits, 0)


def trigger_jpeg(sub_bits, seed=5):
    """mixed_cr_422, 131 x 67, q 100 (table of ones), restart interval 1: a
    raw scan just over 128 subsequences of sub_bits whose destuffed stream
    (81 markers and heavy 0xFF stuffing shorter) ends before subsequence 127.
    So slot 128 of the first workgroup -- the partner of live slot 0 in
    k_huff_sync2's chain pairs, and the first chain its lane ever sets up --
    is an empty trailing subsequence."""
    samp = J.LAYOUTS["mixed_cr_422"][0]
    geo = J.geometry(samp, 131, 67)
    nb = sum(a * b for a, b in geo)
    rng = np.random.default_rng(seed)
    order = rng.permutation(nb * 63)
    vals = rng.integers(1, 40, nb * 63) * rng.choice([-1, 1], nb * 63)
    dc = rng.integers(-100, 100, nb)

    def build(n):
        flat = np.zeros((nb, 64), np.int64)
        flat[:, 0] = dc
        flat[order[:n] // 63, 1 + order[:n] % 63] = vals[:n]
        offs = np.cumsum([0] + [a * b for a, b in geo])
        comps = [flat[offs[i]:offs[i + 1]].reshape(a, b, 64) for i, (a, b) in enumerate(geo)]
        return J.from_coefs(comps, samp, 131, 67, [np.ones(64, int)] * 2, restart=1)

    def scan_bits(d):
        i = d.index(b"\xff\xda")
        scan = d[i + 2 + int.from_bytes(d[i + 2:i + 4], "big"):-2]
        drop = scan.count(b"\xff\x00") + 2 * sum(scan.count(bytes([0xFF, 0xD0 + k])) for k in range(8))
        return len(scan) * 8, (len(scan) - drop) * 8
    lo, hi = 0, nb * 63
    while lo < hi:  # fewest nonzero coefficients whose raw scan exceeds 128 subsequences
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if scan_bits(build(mid))[0] > 128 * sub_bits else (mid + 1, hi)
    data = build(lo)
    raw, ds = scan_bits(data)
    assert raw > 128 * sub_bits and ds <= 127 * sub_bits
    return data


@pytest.fixture(scope="module")
def emu_san(tmp_path_factory):
    """tests/native/emu_main.cpp + the emulator + the header parser as one
    stand-alone program under AddressSanitizer and UBSan, run as a child
    process (nothing preloaded): f(data, sub_bits) -> CompletedProcess."""
    d = tmp_path_factory.mktemp("emu_san")
    exe = str(d / "emu_main")
    srcs = [os.path.join(NATIVE, "emu_main.cpp"), os.path.join(NATIVE, "emu.cpp"),
            os.path.join(ROOT, "datago_amd", "csrc", "host", "jpeg_header.cpp")]
    subprocess.run(["g++", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-static-libasan", "-ffp-contract=off", "-I" + os.path.join(ROOT, "datago_amd", "csrc"), "-o", exe] + srcs, check=True)
    count = [0]

    def run(data, sub_bits, lead=0):
        count[0] += 1
        path = str(d / ("f%d.jpg" % count[0]))
        with open(path, "wb") as f:
            f.write(data)
        return subprocess.run([exe, path, str(sub_bits), str(lead)], capture_output=True, text=True)
    return run


@pytest.mark.parametrize("sub_bits", [1024, 128])
def test_sanitized_empty_trailing_subsequence(emu_san, sub_bits):
    """schain_range's early return for an empty trailing subsequence left the
    chain's table pointers unset while schain_step2 went on reading them for
    its partner's steps: UBSan reported `dg_entropy.h: reference binding to
    null pointer` on these files before the fix."""
    for s in (1024, 128):
        r = emu_san(trigger_jpeg(s), sub_bits)
        assert r.returncode == 0, (s, r.stdout[-300:], r.stderr[-1500:])


def test_sanitized_crafted_layouts(emu_san):
    for name in J.OK_LAYOUTS:
        for sub_bits, lead in ((1024, 0), (128, 96)):
            r = emu_san(J.layout_jpeg(name, 131, 67, seed=2, quality=100, restart=3), sub_bits, lead)
            assert r.returncode == 0, (name, sub_bits, r.stdout[-300:], r.stderr[-1500:])


def test_truncated_stream_is_detected(emu):
    data = synth.make_jpeg(3, 300, 200, 90, "4:2:0")
    cut = data[: len(data) * 2 // 3]
    r, co, stats = emu(cut, 1024)
    assert stats[6] < stats[7]  # decoded blocks < total blocks -> CORRUPT on the GPU path
