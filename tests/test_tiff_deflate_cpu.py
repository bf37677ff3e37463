"""The TIFF Deflate path without a GPU: the admitting header walk and the lane routines of dg_tiff_inflate.h as the
stand-alone program tests/native/tiff_inflate_emu.cpp over the files of tiff_deflate_craft, against Pillow; the same
program under AddressSanitizer and UBSan, also over truncations; the option row."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import tiff_craft as T
import tiff_deflate_craft as D
from test_tiff_cpu import CSRC, ROOT, _run

SRCS = [os.path.join(ROOT, "tests", "native", "tiff_inflate_emu.cpp"), os.path.join(CSRC, "host", "tiff_header.cpp")]


def _build(exe, *flags):
    subprocess.run(["g++", "-std=c++17", "-I" + CSRC, "-o", exe] + list(flags) + SRCS, check=True)
    return exe


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tinf") / "tiff_inflate_emu"), "-O2")


def test_every_file_decodes_as_pillow_does(emu, tmp_path):
    for group, label, data, pix in D.cases():
        ref = np.asarray(Image.open(io.BytesIO(data)))
        assert np.array_equal(ref, pix), label
        assert _run(emu, tmp_path, data) == (0, "", ref.tobytes()), label


def test_refusals(emu, tmp_path):
    for label, data in D.refusals():
        st, why, raw = _run(emu, tmp_path, data)
        assert st == 2 and "fail" in why and raw is None, (label, st, why)
        with pytest.raises(OSError):
            Image.open(io.BytesIO(data)).load()


def test_sanitized_program_over_files_and_truncations(tmp_path):
    """Host code with its own main, built with AddressSanitizer and UBSan."""
    exe = _build(str(tmp_path / "tiff_inflate_emu_san"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    small = T.tiff(D.mix()[:6, :40], comp=8, pred=2, rps=2, pack=D.z(9))
    files = [c[2] for c in D.cases()] + [r[1] for r in D.refusals()] + [small[:k] for k in range(0, len(small), 3)]
    for data in files + [small[:8] + small[8:][::-1]]:
        _run(exe, tmp_path, data)  # (asserts a clean exit)


def test_option_row():
    """The row "tiff_deflate" stands in options.cpp's second table and takes 0 and 1 only."""
    import test_options_cpu as TO
    out = subprocess.run([TO.build_options_main(), "apply", "tiff_deflate", "0", "tiff_deflate", "1", "tiff_deflate", "2"],
                         check=True, capture_output=True, text=True).stdout.split("\n")
    assert [ln.split("\t")[:3] for ln in out[:3]] == [["0", "0", "1"], ["0", "1", "0"], ["1", "0", "1"]]  # status, stored, unchanged
