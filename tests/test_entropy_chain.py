"""Chained multi steps of the state-only Huffman decodes (option "sync_chain",
multi_chain in datago_amd/csrc/dg_entropy.h) on the CPU: tests/native/
emu_chain.cpp runs the product's lead_in and decode_range<false> over every
range with up to 1, 2 and 3 more multi entries per step, and every lead-in
state, range result (exit state, m, n, dc[3]) and checkpoint record must equal
the unchained decode's, word for word; the write pass's coefficients must equal
the oracle's.  A chain bug that stopped the position from advancing would hang
a GPU, so this runs before any GPU does."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from datago_amd import synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SO = os.path.join(NATIVE, "libemu_chain.so")

SUB_BITS = (256, 2048, 8192)
LEADS = (0, 512, 4096)


@pytest.fixture(scope="module")
def emu():
    srcs = [os.path.join(NATIVE, "emu_chain.cpp"), os.path.join(ROOT, "datago_amd", "csrc", "host", "jpeg_header.cpp")]
    deps = srcs + [os.path.join(ROOT, "datago_amd", "csrc", f) for f in ("dg_entropy.h", "dg_types.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        # build beside it and rename: parallel test workers never load a half-written library
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "datago_amd", "csrc"), "-o", tmp] + srcs, check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    E.emu_chain_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.POINTER(ctypes.c_int16), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                   ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                   ctypes.POINTER(ctypes.c_int64)]

    def run(data, sub_bits, lead, chain):
        """-> (coefficients, every state the decodes produced, stats)"""
        cap, cap_rec = 1 << 13, 1 << 21
        out = np.zeros((cap, 64), np.int16)
        rec = np.zeros(cap_rec, np.uint32)
        nb, nr = ctypes.c_size_t(), ctypes.c_size_t()
        st = (ctypes.c_int64 * 10)()
        r = E.emu_chain_decode(data, len(data), sub_bits, lead, chain, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                               cap, ctypes.byref(nb), rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap_rec,
                               ctypes.byref(nr), st)
        assert r == 0 and nb.value <= cap
        return out[: nb.value], rec[: nr.value].copy(), list(st)
    return run


def _pil(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _cases():
    """name -> (jpeg bytes factory, flat)"""
    c = {}
    for ss, gray in (("4:2:0", False), ("4:2:2", False), ("4:4:4", False), ("4:4:4", True)):
        for q in (10, 75, 95):
            name = ("gray" if gray else ss.replace(":", "")) + f"_q{q}"
            c[name] = (lambda ss=ss, gray=gray, q=q: synth.make_jpeg(700 + q, 157, 117, q, ss, gray), False)
    # 4-6 bit blocks: many block ends inside one peek, the chain must stop at each
    c["flat"] = (lambda: _pil(np.full((120, 160, 3), 131, np.uint8), quality=75), True)
    # blocks that run to zigzag 63 without EOB
    c["noise_q100"] = (lambda: _pil(np.random.default_rng(5).integers(0, 256, (48, 64, 3), dtype=np.uint8),
                                    quality=100, subsampling=0), False)
    # per-image tables: codes longer than kMultiBits
    c["optimized"] = (lambda: _pil(synth.synth_pixels(np.random.default_rng(6), 160, 120), quality=92, optimize=True),
                      False)
    px = synth.synth_pixels(np.random.default_rng(8), 150, 110)
    c["rst_mcu"] = (lambda: synth.encode_jpeg(px, 85, "4:2:0", restart_marker_blocks=1), False)
    c["rst_row"] = (lambda: synth.encode_jpeg(px, 85, "4:2:2", restart_marker_rows=1), False)
    # 8192-bit ranges with checkpoints and a half-way split
    c["large_q95"] = (lambda: synth.make_jpeg(9, 512, 384, 95, "4:2:0"), False)
    return c


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_chained_steps_equal_unchained(emu, name):
    make, flat = CASES[name]
    data = make()
    st, ref = O.jpeg_coefs(data)
    assert st == 0
    for sub_bits in SUB_BITS:
        for lead in LEADS:
            base = None
            for chain in range(4):
                co, rec, stats = emu(data, sub_bits, lead, chain)
                key = (name, sub_bits, lead, chain)
                assert stats[4] == 0, key  # no step consumed more than the 32 bits one bw_shift covers
                assert stats[5] == 0, key  # write pass exit == the state-only decode's exit everywhere
                assert stats[6] >= stats[7], key  # every block decoded (the padding bits may read as one more)
                assert co.shape == ref.shape and np.array_equal(co, ref), key
                if chain == 0:
                    base = (rec, stats)
                    assert stats[3] == 0, key
                    continue
                # lead-in states, range results and checkpoint records, before and after the re-decodes
                assert rec.shape == base[0].shape and np.array_equal(rec, base[0]), key
                assert stats[8] == base[1][8], key  # the same ranges were re-decoded
                assert stats[1] <= base[1][1] and stats[2] <= base[1][2], key
                if not flat:
                    assert stats[3] > 0, key  # the chain was taken
                    assert stats[2] < base[1][2], key  # ... and saved steps
