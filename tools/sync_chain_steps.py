#!/usr/bin/env python3
"""Steps per range of k_huff_sync's state-only decodes with 0..3 chained
multi entries per step (option sync_chain), counted on the CPU by
tests/native/emu_chain.cpp over images of the benchmark pool.

    python tools/sync_chain_steps.py [--images 32] [--sub-bits 8192] [--cxxflags=-DDG_CHAIN_DC=1]

Lead-in as the library's auto setting: 4096 bits for MCUs of >= 4 blocks, else 2048.
"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from datago_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--sub-bits", type=int, default=8192)
    ap.add_argument("--cxxflags", default="")
    a = ap.parse_args()
    idx = list(range(a.images))
    synth.generate_pool_images(a.seed, a.pool, idx, workers=min(8, os.cpu_count() or 1))
    datas = synth.load_pool_images(a.seed, a.pool, idx)
    spec = synth.mixed_spec(a.seed, a.pool)
    so = os.path.join(tempfile.mkdtemp(), "libemu_chain.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off"] + a.cxxflags.split() +
                   ["-I" + os.path.join(ROOT, "datago_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "emu_chain.cpp"),
                    os.path.join(ROOT, "datago_amd", "csrc", "host", "jpeg_header.cpp")], check=True)
    E = ctypes.CDLL(so)
    P = ctypes.POINTER
    E.emu_chain_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                   P(ctypes.c_int16), ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_uint32),
                                   ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_int64)]
    cap, cap_rec = 1 << 17, 1 << 22
    out = np.zeros((cap, 64), np.int16)
    rec = np.zeros(cap_rec, np.uint32)
    tot = np.zeros((4, 10), np.int64)
    base = None
    for i, d in enumerate(datas):
        w, h, q, ss, gray = spec[i]
        lead = 4096 if (ss == "4:2:0" and not gray) else 2048
        for chain in range(4):
            nb, nr = ctypes.c_size_t(), ctypes.c_size_t()
            st = (ctypes.c_int64 * 10)()
            r = E.emu_chain_decode(d, len(d), a.sub_bits, lead, chain, out.ctypes.data_as(P(ctypes.c_int16)), cap,
                                   ctypes.byref(nb), rec.ctypes.data_as(P(ctypes.c_uint32)), cap_rec, ctypes.byref(nr),
                                   st)
            assert r == 0 and st[4] == 0 and st[5] == 0, (i, chain, r, list(st))
            cur = rec[: nr.value].copy()
            if chain == 0:
                base = cur
            assert np.array_equal(cur, base), (i, chain)
            tot[chain] += np.array(list(st))
    bits = sum(len(d) for d in datas) * 8
    print(f"{a.images} pool images (seed {a.seed}), sub_bits {a.sub_bits}, {tot[0][0]} ranges, "
          f"{bits / tot[0][7]:.1f} coded bits per block {a.cxxflags}")
    print("chain  lead-in steps/range  range steps/range  total/range  vs chain 0  chained entries/range")
    for c in range(4):
        n = tot[c][0]
        t = (tot[c][1] + tot[c][2]) / n
        t0 = (tot[0][1] + tot[0][2]) / n
        print(f"{c:5d}  {tot[c][1] / n:19.1f}  {tot[c][2] / n:17.1f}  {t:11.1f}  {t / t0:10.3f}  {tot[c][3] / n:21.1f}")


if __name__ == "__main__":
    main()
