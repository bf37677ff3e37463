"""The PNG re-encoder's per-image Huffman codes (context option "penc_dynamic")
pinned on the CPU:

  1. the reference (tests/ref_penc_dyn.py) against readers that share nothing
     with it, and against plain Huffman where the limit does not bind;
  2. the set of cases reaches the format's edges (both limiters, both block
     types, every run-length symbol, HLIT at both ends);
  3. the shared header the kernel runs (datago_amd/csrc/dg_penc_tree.h, built
     for the CPU through tests/native/penc_tree_emu.cpp) against the reference:
     lengths, codes, run-length tokens and header bits, all for equality --
     and the same sources as a program of their own under ASan + UBSan.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import enc_cases as E
import penc_dyn_cases as C
import ref_penc
import ref_penc_dyn as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "penc_tree_emu.cpp")
SO = os.path.join(NATIVE, "libpenc_tree_emu.so")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "dg_penc_tree.h"), os.path.join(CSRC, "dg_types.h")]

CASES = C.all_cases()


def _ref(label):
    return C.dyn_ref(label, dict(CASES)[label])


def _kraft(lens, limit):
    used = [n for n in lens if n]
    assert max(used) <= limit
    return sum(1 << (limit - n) for n in used), 1 << limit


# ------------------------------------------------------------------ 1. the reference

@pytest.mark.parametrize("label", [c[0] for c in CASES])
def test_reference_file(label):
    arr = dict(CASES)[label]
    r = _ref(label)
    E.png_independent_checks(r.file, arr)
    blk, data = D.read_block(D.idat_deflate(r.file))
    assert data == r.stream.tobytes()
    assert blk.tokens == ref_penc.parse(r.stream) == r.tokens
    assert blk.dyn == r.dyn
    if r.dyn:
        assert blk.litlen == r.litlen[:blk.hlit] and blk.distlen == [1] and blk.cllen == r.cllen
        assert blk.hdr_bits == r.hdr_bits and blk.bits == r.body_bits
    # both codes are complete and within their limits; unused symbols have no code
    assert _kraft(r.litlen, 15)[0] == _kraft(r.litlen, 15)[1]
    if sum(1 for n in r.cllen if n) > 1:
        assert _kraft(r.cllen, 7)[0] == _kraft(r.cllen, 7)[1]
    else:
        assert sorted(r.cllen)[-2:] == [0, 1]
    assert all((n == 0) == (f == 0) for n, f in zip(r.litlen, r.freq))
    clfreq = [0] * 19
    for s, _ in r.rle:
        clfreq[s] += 1
    assert all((n == 0) == (f == 0) for n, f in zip(r.cllen, clfreq))
    # optimal where the limit does not bind
    for freq, lens, limit in ((r.freq, r.litlen, 15), (clfreq, r.cllen, 7)):
        if sum(1 for f in freq if f) >= 2:
            depth, cost = C.huffman_depth(freq)
            if depth <= limit:
                assert sum(f * n for f, n in zip(freq, lens)) == cost, limit
    # the choice: never longer than the fixed file, and the fixed file itself when the block is fixed
    fixed = E.png_ref(label, arr).file
    assert len(r.file) <= len(fixed)
    assert r.dyn == (r.body_bits < r.fixed_bits)
    if not r.dyn:
        assert r.file == fixed


# ------------------------------------------------------------------ 2. the set reaches its edges

def _clfreq(r):
    f = [0] * 19
    for s, _ in r.rle:
        f[s] += 1
    return f


def test_set_reaches_edges():
    refs = {label: _ref(label) for label, _ in CASES}
    depth = C.huffman_depth(refs[C.FIB_LABEL].freq)[0]
    assert depth > 15, depth
    assert max(refs[C.FIB_LABEL].litlen) == 15 and refs[C.FIB_LABEL].dyn
    for label in C.CL_LIMITED:
        assert C.huffman_depth(_clfreq(refs[label]))[0] > 7, label
        assert max(refs[label].cllen) == 7, label
    assert any(refs[label].dyn for label in C.CL_LIMITED)
    kinds = {r.dyn for r in refs.values()}
    assert kinds == {False, True}
    assert {16, 17, 18} <= {s for r in refs.values() if r.dyn for s, _ in r.rle}
    hlit = {max(257, max(s for s in range(286) if r.litlen[s]) + 1) for r in refs.values() if r.dyn}
    assert {257, 286} <= hlit, sorted(hlit)
    for label in C.PHOTO_LABELS:
        arr = dict(CASES)[label]
        assert refs[label].dyn and len(refs[label].file) < arr.size, (label, len(refs[label].file), arr.size)


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
    lib.pte_lengths.argtypes = [p, ctypes.c_uint32, ctypes.c_uint32, p]
    lib.pte_lengths.restype = ctypes.c_int
    lib.pte_build.argtypes = [p] * 8
    lib.pte_build.restype = None
    return lib


def _emu_lengths(lib, freq, limit):
    f = np.asarray(freq, np.uint32)
    out = np.zeros(len(f), np.uint8)
    assert lib.pte_lengths(f.ctypes.data, len(f), limit, out.ctypes.data) == 1
    return out.tolist()


def _expected_build(freq):
    """What the header must give for a literal/length histogram, from the reference's functions."""
    litlen = D.package_merge(freq, 15)
    bits, cllen, toks, nlit = D.header(litlen)
    codes = D.canonical(litlen)
    table = [0] * 286
    for s, (c, n) in codes.items():
        table[s] = ref_penc._rev(c, n) | n << 16
    words = np.frombuffer(bits.tobytes() + b"\0" * 4, np.uint8)
    nw = (bits.nbits() + 31) // 32
    words = words[:4 * nw].view("<u4").tolist()
    last = max(i for i, s in enumerate(D.CL_ORDER) if cllen[s])
    extra = [0] * 257 + [ref_penc._LEN_EXTRA[i] for i in range(29)]
    dyn = bits.nbits() + sum(f * (n + (extra[s] + 1 if s > 256 else 0)) for s, (f, n) in enumerate(zip(freq, litlen)))
    fix = 3 + sum(f * (ref_penc._FIXED[s][1] + (extra[s] + 5 if s > 256 else 0)) for s, f in enumerate(freq))
    return dict(litlen=litlen, table=table, cllen=cllen, tok=[s | x << 5 for s, x in toks], hlit=nlit - 257,
                hclen=max(4, last + 1) - 4, hdr_bits=bits.nbits(), hdr=words, dyn=int(dyn < fix), dyn_bits=dyn,
                fixed_bits=fix)


def _emu_build(lib, freq):
    f = np.asarray(freq, np.uint32)
    assert len(f) == 286
    litlen, table, cllen = np.zeros(286, np.uint8), np.zeros(286, np.uint32), np.zeros(19, np.uint8)
    tok, info, hdr, bits = np.zeros(288, np.uint16), np.zeros(5, np.uint32), np.zeros(136, np.uint32), np.zeros(2, np.uint64)
    lib.pte_build(*[a.ctypes.data for a in (f, litlen, table, cllen, tok, info, hdr, bits)])
    ntok, hlit, hclen, hdr_bits, dyn = info.tolist()
    assert not hdr[(hdr_bits + 31) // 32:].any()
    return dict(litlen=litlen.tolist(), table=table.tolist(), cllen=cllen.tolist(), tok=tok[:ntok].tolist(), hlit=hlit,
                hclen=hclen, hdr_bits=hdr_bits, hdr=hdr[:(hdr_bits + 31) // 32].tolist(), dyn=dyn,
                dyn_bits=int(bits[0]), fixed_bits=int(bits[1]))


def _same_build(lib, freq, what):
    got, exp = _emu_build(lib, freq), _expected_build(freq)
    for key in exp:
        assert got[key] == exp[key], (what, key)


def test_header_on_case_histograms(emu):
    for label, arr in CASES:
        r = _ref(label)
        _same_build(emu, r.freq, label)
        got = _emu_build(emu, r.freq)
        assert (got["dyn"], got["hdr_bits"], got["dyn_bits"], got["fixed_bits"]) == \
            (int(r.dyn), r.hdr_bits, r.body_bits, r.fixed_bits), label


def _random_histograms(count, seed):
    """Literal/length histograms with n = 2..286 used symbols (256 always among them): flat, geometric, heavy tail."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(2, 287))
        used = rng.choice(np.delete(np.arange(286), 256), n - 1, replace=False)
        shape = i % 3
        if shape == 0:
            v = rng.integers(1, 40, n - 1)
        elif shape == 1:
            v = np.maximum(1, (2.0 ** rng.uniform(0, 28, n - 1))).astype(np.int64)
        else:
            v = np.maximum(1, rng.pareto(0.7, n - 1) * 3).astype(np.int64).clip(1, 1 << 28)
        f = np.zeros(286, np.int64)
        f[used] = v
        f[256] = 1
        yield f.tolist()


def test_header_on_random_histograms(emu):
    for i, f in enumerate(_random_histograms(2000, 5000)):
        _same_build(emu, f, f"random {i}")


def _fib(n):
    """Fibonacci frequencies with the ties taken out (1000 * F(k) + k): plain Huffman is one chain, n - 1 deep."""
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return [1000 * v + k for k, v in enumerate(f[:n])]


def test_header_ties_and_limits(emu):
    # all-equal frequencies: every comparison is a tie
    for n in (2, 3, 19, 20, 255, 286):
        for v in (1, 7):
            f = [0] * 286
            for s in list(range(n - 1)) + [256]:
                f[s] = v
            f[256] = 1 if v == 1 else v  # (the histogram's own 256 is 1; the header takes any frequency)
            _same_build(emu, f, f"equal {n} x {v}")
    # n = 2
    f = [0] * 286
    f[65], f[256] = 1000, 1
    _same_build(emu, f, "n = 2")
    # Fibonacci past the limiter for L = 15
    for n in (17, 24, 30):
        f = [0] * 286
        for s, v in zip(range(0, 3 * n, 3), _fib(n)):
            f[s] = v
        f[256] = 1
        assert C.huffman_depth(f)[0] > 15
        _same_build(emu, f, f"fibonacci {n}")
        assert max(_emu_build(emu, f)["litlen"]) == 15
    # ... and for L = 7, over the code-length alphabet, with the lengths alone
    for n in (9, 12, 19):
        for order in (1, -1):
            f = (_fib(n) + [0] * (19 - n))[::order]
            assert C.huffman_depth(f)[0] > 7
            got = _emu_lengths(emu, f, 7)
            assert got == D.package_merge(f, 7) and max(got) == 7, (n, order)
    # one used symbol: length 1
    f = [0] * 19
    f[8] = 5
    assert _emu_lengths(emu, f, 7) == D.package_merge(f, 7) == [0] * 8 + [1] + [0] * 10
    # every limit 1..15 at sizes that fit (2^L >= n)
    rng = np.random.default_rng(5100)
    for limit in range(1, 16):
        for _ in range(20):
            n = int(rng.integers(2, min(1 << limit, 286) + 1))
            f = rng.integers(1, 1000, n).tolist()
            assert _emu_lengths(emu, f, limit) == D.package_merge(f, limit), (limit, n)


def test_header_program_under_sanitizers(tmp_path):
    """The same sources as a program of their own under ASan + UBSan, on a subset; its answers are checked too."""
    san = str(tmp_path / "penc_tree_san")  # (not kept beside the sources: rebuilt per run, a few seconds)
    _build(san, ["-DPT_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    hists = [_ref(label).freq for label in (C.FIB_LABEL, "photo_rgb_128", "one_pixel_gray", "flat_zero") + C.CL_LIMITED]
    hists += list(_random_histograms(40, 5200))
    fibs = [(_fib(n) + [0] * (19 - n)) for n in (9, 19)]
    path = tmp_path / "hists.txt"
    with open(path, "w") as fh:
        for f in hists:
            fh.write("build " + " ".join(map(str, f)) + "\n")
        for f in fibs:
            fh.write("len 7 19 " + " ".join(map(str, f)) + "\n")
    res = subprocess.run([san, str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(hists) + len(fibs)
    for f, line in zip(hists, lines):
        v = line.split()
        assert v[0] == "build"
        v = list(map(int, v[1:]))
        exp = _expected_build(f)
        nw = (exp["hdr_bits"] + 31) // 32
        want = (exp["litlen"] + exp["table"] + exp["cllen"]
                + [len(exp["tok"]), exp["hlit"], exp["hclen"], exp["hdr_bits"], exp["dyn"]] + exp["tok"] + exp["hdr"][:nw]
                + [exp["dyn_bits"], exp["fixed_bits"]])
        assert v == want
    for f, line in zip(fibs, lines[len(hists):]):
        assert list(map(int, line.split()[1:])) == D.package_merge(f, 7)
