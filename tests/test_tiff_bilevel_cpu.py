"""The bilevel TIFF path without a GPU: the header walk with bilevel = true and the lane routines of dg_tiff_g4.h as the
stand-alone program tests/native/tiff_g4_emu.cpp over the case list, against Pillow and the arrays the files were made
from; the same program under AddressSanitizer and UBSan; the two broken streams; the option row."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import tiff_bilevel_cases as B
from test_tiff_cpu import CSRC, ROOT, _run

SAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")  # host code with its own main


@pytest.mark.parametrize("flags", [("-O2",), SAN], ids=["plain", "sanitized"])
def test_case_list_and_broken_streams(tmp_path, flags):
    exe = str(tmp_path / "tiff_g4_emu")
    subprocess.run(["g++", "-std=c++17", "-I" + CSRC, "-o", exe, *flags, os.path.join(ROOT, "tests", "native", "tiff_g4_emu.cpp"),
                    os.path.join(CSRC, "host", "tiff_header.cpp")], check=True)
    for label, arr, rps in B.cases():
        pix = np.asarray(arr, np.uint8) * 255
        for data in [B.written(arr, "g4", rps), B.crafted(1 - arr, True, photo=0, be=True)] + [B.written(arr, "lzw", rps)] * (rps == 3):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("L")), pix), label
            assert _run(exe, tmp_path, data) == (0, "", pix.tobytes()), label
    page = B.cases()[-1][1]
    strip = B.g4_strip(1 - page)
    for pack in (lambda d: strip[:len(strip) // 2], lambda d: b"\x02" + strip[1:]):  # cut short; 0000001x, the extension code
        assert _run(exe, tmp_path, B.crafted(page, True, pack=pack)) == (1, "TIFF: irregular Group 4 stream", None)


def test_option_row():
    """The row "tiff_bilevel" stands in options.cpp's second table and takes 0 and 1 only."""
    import test_options_cpu as TO
    out = subprocess.run([TO.build_options_main(), "apply", "tiff_bilevel", "0", "tiff_bilevel", "1", "tiff_bilevel", "2"],
                         check=True, capture_output=True, text=True).stdout.split("\n")
    assert [ln.split("\t")[:3] for ln in out[:3]] == [["0", "0", "1"], ["0", "1", "0"], ["1", "0", "1"]]  # status, stored, unchanged
