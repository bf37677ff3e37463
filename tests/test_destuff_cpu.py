"""The lane routines of the destuff count and write passes
(datago_amd/csrc/dg_destuff.h) on the CPU.

tests/native/destuff_emu.cpp is a program of its own: it runs the routines the
kernels run (window shift, classification of a 64-byte span, staging on the
output's dword grid) lane by lane over scans at every address mod 16, of
lengths 0 .. 5 * 4096 + 7, filled with random bytes, a dense FF / 00 / Dn
alphabet, all FF 00, and FF 00 / FF FF Dn / FF Dn / FF xx sequences laid
across the last byte of a lane, a wave (= chunk) and the scan at every phase,
and compares kept bytes, marker bit positions and per-chunk counts with a byte
loop built on destuff_keep.  It is built plain and under ASan + UBSan (the
scan ends where its allocation ends) and run directly.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "destuff_emu.cpp")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")


@pytest.mark.parametrize("name,extra", [
    ("plain", ["-O2"]),
    ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
])
def test_lane_routines(tmp_path, name, extra):
    exe = str(tmp_path / f"destuff_emu_{name}")
    subprocess.run(["g++", "-std=c++17", "-I" + CSRC, "-o", exe, SRC] + extra, check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.startswith("ok ") and int(res.stdout.split()[1]) >= 2704
