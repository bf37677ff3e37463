"""The 16-bit TIFF path without a GPU: the header walk with deep = true and the tiff16_* lane routines of dg_tiff.h as
the stand-alone program tests/native/tiff16_emu.cpp over the files of tiff16_craft, against the arrays they were made
from (test_gpu_tiff16.py holds Pillow to them); the same program under AddressSanitizer and UBSan, also over
truncations; the option row."""
import os
import subprocess

import pytest

import tiff16_craft as S
from test_tiff_cpu import CSRC, ROOT, _run

SAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")  # host code with its own main
FILES = [c for c in S.forms() if "deflate" not in c[0]] + [
    S.tiff16("pred %dx3x%d %s" % (w, c, "MM" if be else "II"), S.noise16(3, w, c, w + c), be=be, comp=5, pred=2)
    for w in (1, 5, 65) for c in (1, 2, 3, 4) for be in (False, True)]


@pytest.mark.parametrize("flags", [("-O2",), SAN], ids=["plain", "sanitized"])
def test_files_refusals_and_truncations(tmp_path, flags):
    exe = str(tmp_path / "tiff16_emu")
    subprocess.run(["g++", "-std=c++17", "-I" + CSRC, "-o", exe, *flags, os.path.join(ROOT, "tests", "native", "tiff16_emu.cpp"),
                    os.path.join(CSRC, "host", "tiff_header.cpp")], check=True)
    for label, data, pix in FILES[::1 if flags == ("-O2",) else 4]:
        assert _run(exe, tmp_path, data) == (0, "", pix.astype("=u2").tobytes()), label
    for label, data, corrupt in S.refusals():
        st, why, raw = _run(exe, tmp_path, data)
        assert st == (2 if corrupt else 1) and why.startswith("TIFF: ") and raw is None, (label, st, why)
    small = S.tiff16("", S.noise16(3, 16, 3, 4), be=True, comp=5, pred=2, rps=2)[1]
    for data in [small[:k] for k in range(0, len(small), 3)] + [small[:8] + small[8:][::-1]]:
        _run(exe, tmp_path, data)  # (asserts a clean exit)


def test_option_row():
    """The row "tiff16" stands in options.cpp's second table and takes 0 and 1 only."""
    import test_options_cpu as TO
    out = subprocess.run([TO.build_options_main(), "apply", "tiff16", "0", "tiff16", "1", "tiff16", "2"],
                         check=True, capture_output=True, text=True).stdout.split("\n")
    assert [ln.split("\t")[:3] for ln in out[:3]] == [["0", "0", "1"], ["0", "1", "0"], ["1", "0", "1"]]  # status, stored, unchanged
