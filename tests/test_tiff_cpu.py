"""The TIFF path without a GPU: host/tiff_header.cpp and the lane routines of dg_tiff.h as the stand-alone program
tests/native/tiff_emu.cpp over the crafted files and refusals of tiff_craft, against Pillow; the same program under
AddressSanitizer and UBSan, also over truncations; the option row; dg_probe."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import tiff_craft as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "native", "tiff_emu.cpp"), os.path.join(CSRC, "host", "tiff_header.cpp")]


def _build(exe, *flags):
    subprocess.run(["g++", "-std=c++17", "-I" + CSRC, "-o", exe] + list(flags) + SRCS, check=True)
    return exe


def _run(exe, tmp_path, data):
    """(status, why, pixels or None) of one file through the program."""
    src, dst = tmp_path / "in.tif", tmp_path / "out.raw"
    src.write_bytes(data)
    dst.unlink(missing_ok=True)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    head, why = r.stdout.strip().split(" |")
    return int(head.split()[0]), why.strip(), dst.read_bytes() if dst.exists() else None


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tiff") / "tiff_emu"), "-O2")


def test_every_file_decodes_as_pillow_does(emu, tmp_path):
    for label, data, pix in T.cases():
        ref = np.asarray(Image.open(io.BytesIO(data)))
        assert np.array_equal(ref, pix), label
        assert _run(emu, tmp_path, data) == (0, "", ref.tobytes()), label


def test_refusals(emu, tmp_path):
    for label, data, corrupt in T.refusals():
        st, why, raw = _run(emu, tmp_path, data)
        assert st == (2 if corrupt else 1) and why and raw is None, (label, st, why)
    with pytest.raises(OSError):  # libtiff gives up on a table that stays full, a little later than the library
        Image.open(io.BytesIO(dict((r[0], r[1]) for r in T.refusals())["stream: LZW table stays full"])).load()


def test_sanitized_program_over_files_and_truncations(tmp_path):
    """Host code with its own main, built with AddressSanitizer and UBSan."""
    exe = _build(str(tmp_path / "tiff_emu_san"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    small = T.tiff(T.noise(3, 16, 3, 4), comp=5, pred=2, rps=2)
    files = [c[1] for c in T.cases()[::3]] + [r[1] for r in T.refusals()] + [small[:k] for k in range(0, len(small), 3)]
    for data in files + [small[:8] + small[8:][::-1]]:
        _run(exe, tmp_path, data)  # (asserts a clean exit)


def test_option_row_and_probe():
    """The row "tiff" stands in options.cpp's second table and takes 0 and 1 only; dg_probe names a TIFF."""
    import test_options_cpu as TO
    out = subprocess.run([TO.build_options_main(), "apply", "tiff", "0", "tiff", "1", "tiff", "2"], check=True,
                         capture_output=True, text=True).stdout.split("\n")
    assert [ln.split("\t")[:3] for ln in out[:3]] == [["0", "0", "1"], ["0", "1", "0"], ["1", "0", "1"]]  # status, stored, unchanged
    from datago_amd import _lib as L
    data = T.tiff(T.noise(70, 97, 4, 3), comp=5, tile=(32, 32))
    st, info = L.probe(data)
    assert st == L.DG_OK and (info.format, info.width, info.height, info.components, info.bit_depth) == (L.DG_FMT_TIFF, 97, 70, 4, 8)
    assert L.DG_FMT_TIFF == 6 and info.gpu_supported == 0
    st, info = L.probe(data[:-20])
    assert st == L.DG_ERR_CORRUPT and info.format == L.DG_FMT_TIFF and "IFD" in L.last_error()
