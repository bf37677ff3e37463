"""The JPEG re-encoder's per-image Huffman tables (context option
"jenc_optimize") pinned on the CPU:

  1. the reference (tests/ref_jenc_opt.py) against readers that share nothing
     with it (PIL, the oracle's coefficient reader, a heapq Huffman build) and
     against the repository's other restatement of the rule (synth._huff_optimal);
  2. the set of cases reaches the rule's edges (one-symbol tables, the 16-bit
     limit binding, partial blocks, dense noise), and every twin is shorter;
  3. the shared header the kernel runs (datago_amd/csrc/dg_jenc_tree.h, built
     for the CPU through tests/native/jenc_tree_emu.cpp) against the reference:
     sizes, BITS, HUFFVAL, codes and DHT bytes, all for equality -- and the
     same sources as a program of their own under ASan + UBSan.
"""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

import jenc_opt_cases as C
import penc_dyn_cases as P
import ref_jenc_opt as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "jenc_tree_emu.cpp")
SO = os.path.join(NATIVE, "libjenc_tree_emu.so")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "dg_jenc_tree.h"), os.path.join(CSRC, "dg_types.h")]

PAIRS = C.pairs()
IDS = [f"{label}-q{q}" for label, _, q in PAIRS]


def _lengths(t):
    """Final code length per symbol 0..255 (0: no code)."""
    out = [0] * 256
    for s, (_, n) in R.canonical(t.bits, t.vals).items():
        out[s] = n
    return out


# ------------------------------------------------------------------ 1. the reference

@pytest.mark.parametrize("label,arr,quality", PAIRS, ids=IDS)
def test_reference_twin(label, arr, quality):
    from PIL import Image

    from datago_amd.synth import _huff_optimal
    from oracle import oracle as O
    std, tw = C.std_file(label, arr, quality), C.twin(label, arr, quality)
    assert not tw.fallback
    a, b = np.asarray(Image.open(io.BytesIO(std))), np.asarray(Image.open(io.BytesIO(tw.file)))
    assert a.shape == b.shape and np.array_equal(a, b)
    nb = -(-arr.shape[0] // 8) * -(-arr.shape[1] // 8) * arr.shape[2] + 8
    (s0, c0), (s1, c1) = O.jpeg_coefs(std, nb), O.jpeg_coefs(tw.file, nb)
    assert s0 == 0 and s1 == 0 and np.array_equal(c0, c1)
    for key, t in tw.tables.items():
        h, lens = tw.hist[key], _lengths(t)
        assert max(lens) <= 16
        assert sum(1 << (16 - n) for n in lens if n) < 1 << 16  # Kraft sum strictly below 1: all ones stays free
        assert all((n == 0) == (f == 0) for n, f in zip(lens, h))
        if max(t.sizes) <= 16:  # the limit does not bind: as short as plain Huffman with the reserved symbol
            _, cost = P.huffman_depth(h + [1])
            assert sum(f * n for f, n in zip(h, lens)) + t.sizes[256] == cost, key
        bits, vals = _huff_optimal(h[:12] if key[0] == 0 else h)
        assert (t.bits[1:], t.vals) == (bits[1:], vals), key
    # everything but the DHTs and the scan is the standard file's
    segs = [s for s in R.segments(std) if s[0] != 0xC4]
    twin_segs = [s for s in R.segments(tw.file) if s[0] != 0xC4]
    assert [std[a:b] for _, a, b in segs] == [tw.file[a:b] for _, a, b in twin_segs]
    assert [tw.file[s[1] + 4] for s in R.segments(tw.file) if s[0] == 0xC4] == [0x00, 0x10, 0x01, 0x11][:len(tw.tables)]
    assert tw.file.endswith(b"\xff\xd9") and R.segments(tw.file)[-1][2] == tw.header_len


# ------------------------------------------------------------------ 2. the set reaches its edges

@pytest.mark.parametrize("label,arr,qualities,prop", C.cases(), ids=[c[0] for c in C.cases()])
def test_case_property(label, arr, qualities, prop):
    for q in qualities:
        tw = C.twin(label, arr, q)
        assert prop(tw), (label, q)
        assert len(tw.file) < len(C.std_file(label, arr, q)), (label, q)
        assert tw.header_len <= tw.std_header_len, (label, q)  # the optimised DHTs list a subset of the symbols


def test_set_reaches_edges():
    labels = [c[0] for c in C.cases()]
    assert {"flat_8x8_gray", "block_8x8_rgb", "partial_13x9_gray", "partial_13x9_rgb", C.NOISE_LABEL,
            C.LIMIT_LABEL} <= set(labels)
    assert {"blocks_1023", "blocks_1024", "blocks_1025", "blocks_3075_rgb", "dc_alternate_gray", "b77_amp16_gray",
            "basis44_gray", "noise_8x8_whole_bytes_11", "noise_8x8_stuffed_end_2"} <= set(labels)
    tw = [C.twin(label, arr, q) for label, arr, q in PAIRS]
    over = [max(t.sizes) for w in tw for t in w.tables.values()]
    assert max(over) > 16 and min(over) == 1  # the limit binds somewhere; a one-symbol table exists
    assert any(len(w.tables) == 2 for w in tw) and any(len(w.tables) == 4 for w in tw)


# ------------------------------------------------------------------ 3. the shared header

def _build(out, extra):
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in DEPS):
        tmp = f"{out}.{os.getpid()}.tmp"  # build beside it and rename: never a half-written file
        subprocess.run(["g++", "-O2", "-std=c++17", "-I" + CSRC, "-o", tmp, SRC] + extra, check=True)
        os.replace(tmp, out)


@pytest.fixture(scope="module")
def emu():
    _build(SO, ["-fPIC", "-shared"])
    lib = ctypes.CDLL(SO)
    p = ctypes.c_void_p
    lib.jte_build.argtypes = [p, ctypes.c_uint32] + [p] * 7
    lib.jte_build.restype = ctypes.c_uint32
    return lib


GUARD = 0xA5


def _emu_build(lib, freq, cls):
    f = np.zeros(256, np.uint32)
    f[:len(freq)] = freq
    # each array is followed by guard bytes that must survive
    sizes, bits, vals, code, length, info, dht = (np.full(n + 16, GUARD, t) for n, t in (
        (257, np.uint8), (17, np.uint8), (256, np.uint8), (256, np.uint16), (256, np.uint8), (2, np.uint32),
        (277, np.uint8)))
    n = lib.jte_build(f.ctypes.data, cls, *[a.ctypes.data for a in (sizes, bits, vals, code, length, info, dht)])
    for a, used in ((sizes, 257), (bits, 17), (vals, 256), (code, 256), (length, 256), (info, 2), (dht, 277)):
        assert (a[used:] == GUARD).all()
    nvals, fallback = info[:2].tolist()
    if fallback:
        assert n == 0
        return dict(fallback=True)
    return dict(fallback=False, sizes=sizes[:257].tolist(), bits=bits[:17].tolist(), vals=vals[:nvals].tolist(),
                code=code[:256].tolist(), len=length[:256].tolist(), dht=dht[:n].tobytes())


def _expected_build(freq, cls):
    t = R.optimal_table(freq)
    if t.fallback:
        return dict(fallback=True)
    codes = R.canonical(t.bits, t.vals)
    return dict(fallback=False, sizes=t.sizes, bits=[0] + t.bits[1:], vals=t.vals,
                code=[codes.get(s, (0, 0))[0] for s in range(256)], len=[codes.get(s, (0, 0))[1] for s in range(256)],
                dht=R.dht_segment(cls, t))


def _same_build(lib, freq, what, cls=0x10):
    got, exp = _emu_build(lib, freq, cls), _expected_build(freq, cls)
    for key in exp:
        assert got[key] == exp[key], (what, key)
    return got


def test_header_on_case_histograms(emu):
    for label, arr, q in PAIRS:
        tw = C.twin(label, arr, q)
        for (kind, tid), h in tw.hist.items():
            got = _same_build(emu, h, (label, q, kind, tid), kind << 4 | tid)
            assert (got["bits"][1:], got["vals"]) == (tw.tables[(kind, tid)].bits[1:], tw.tables[(kind, tid)].vals)
    tw = C.twin(C.LIMIT_LABEL, dict((c[0], c[1]) for c in C.cases())[C.LIMIT_LABEL], 50)
    assert max(_emu_build(emu, tw.hist[(1, 0)], 0x10)["sizes"]) == 19


def _random_histograms(count, seed):
    """n = 1..256 used symbols: uniform, geometric, all equal, and scaled to a sum near 80 M."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(1, 257))
        used = rng.choice(256, n, replace=False)
        shape = i % 4
        if shape == 0:
            v = rng.integers(1, 1000, n)
        elif shape == 1:
            v = np.maximum(1, (2.0 ** rng.uniform(0, 24, n))).astype(np.int64)
        elif shape == 2:
            v = np.full(n, int(rng.integers(1, 100)))
        else:
            v = rng.integers(1, 1000, n).astype(np.float64)
            v = np.maximum(1, v / v.sum() * 80e6).astype(np.int64)
        f = np.zeros(256, np.int64)
        f[used] = v
        yield f.tolist()


def _fib(n):
    """1, 1, 3, 5, 9, ...: f(k) = f(k-1) + f(k-2) + 1.  With the reserved symbol's 1 every merge joins the one
    tree and the next leaf, the tree winning the tie: a chain, n deep."""
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2] + 1)
    return f[:n]


def _special_histograms():
    out = [("all 256 equal", [7] * 256), ("all 256 ones", [1] * 256)]
    for s in (0, 5, 255):
        f = [0] * 256
        f[s] = 12345
        out.append((f"one symbol {s}", f))
        f = [0] * 256
        f[s] = 80_000_000
        out.append((f"one symbol {s}, 80 M", f))
    out.append(("twenty symbols of 80 M", [80_000_000 if s % 13 == 0 else 0 for s in range(256)]))
    for n in (16, 20, 28, 32):  # K.2 sizes up to n: K.3's whole input range
        out.append((f"fibonacci {n}", [0] * 7 + _fib(n) + [0] * (249 - n)))
        out.append((f"fibonacci {n} descending", _fib(n)[::-1] + [0] * (256 - n)))
    return out


def _deep_histograms():
    """Fibonacci counts long enough that a K.2 size passes 32: the fallback."""
    return [_fib(n) + [0] * (256 - n) for n in (33, 40, 44)] + [[0] * 200 + _fib(43)[::-1] + [0] * 13]


def test_header_on_random_histograms(emu):
    for i, f in enumerate(_random_histograms(600, 7000)):
        _same_build(emu, f, f"random {i}", (0x00, 0x10, 0x01, 0x11)[i % 4])


def test_header_ties_limits_and_fallback(emu):
    deepest = 0
    for what, f in _special_histograms():
        got = _same_build(emu, f, what)
        assert not got["fallback"], what
        deepest = max(deepest, max(got["sizes"]))
    assert deepest == 32  # the last size K.3 takes
    one = _emu_build(emu, [0] * 5 + [9] + [0] * 250, 0x00)
    assert one["bits"][1:] == [1] + [0] * 15 and one["vals"] == [5] and (one["code"][5], one["len"][5]) == (0, 1)
    for f in _deep_histograms():
        assert max(R.optimal_table(f).sizes) > 32
        assert _same_build(emu, f, "deep")["fallback"]


def test_header_program_under_sanitizers(tmp_path):
    """The same sources as a program of their own under ASan + UBSan; its answers are checked too."""
    san = str(tmp_path / "jenc_tree_san")  # (not kept beside the sources: rebuilt per run, a few seconds)
    _build(san, ["-DJT_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    by = dict((c[0], c[1]) for c in C.cases())
    hists = []
    for label, q in ((C.LIMIT_LABEL, 50), (C.NOISE_LABEL, 100), ("flat_8x8_gray", 92), ("blocks_3075_rgb", 92)):
        for (kind, tid), h in C.twin(label, by[label], q).hist.items():
            hists.append((kind << 4 | tid, h))
    hists += [(0x10, f) for _, f in _special_histograms()] + [(0x11, f) for f in _deep_histograms()]
    hists += [(0x01, f) for f in _random_histograms(60, 7100)]
    path = tmp_path / "hists.txt"
    with open(path, "w") as fh:
        for cls, f in hists:
            fh.write(f"build {cls} " + " ".join(map(str, f)) + "\n")
    res = subprocess.run([san, str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(hists)
    for (cls, f), line in zip(hists, lines):
        v = line.split()
        assert v[0] == "build"
        v = list(map(int, v[1:]))
        exp = _expected_build(f, cls)
        if exp["fallback"]:
            assert v == [1, 0]
            continue
        want = [0, len(exp["vals"])] + exp["sizes"] + exp["bits"] + exp["vals"] + exp["code"] + exp["len"] \
            + list(exp["dht"])
        assert v == want
