"""The match parse of the PNG re-encoder (context option "penc_match") without a GPU: the reference
(ref_penc_match.py) over penc_match_cases reads back through zlib, PIL and the oracle, is never longer than the
parent's file and equals it where no match block won; the crafted cases hold the tokens they were crafted for; the
header arithmetic of dg_penc_tree.h (pm_build), as the program tests/native/penc_match_emu.cpp, plain and under
AddressSanitizer and UBSan, gives the reference's lengths, bit counts and header bits; the option row."""
import os
import subprocess

import numpy as np
import pytest

import enc_cases as E
import penc_match_cases as C
import ref_penc16
import ref_penc_match as R
from test_tiff_cpu import CSRC, ROOT

CASES = C.cases()


@pytest.mark.parametrize("dynamic", [False, True], ids=["fixed", "dynamic"])
def test_reference_files(dynamic):
    wins = []
    for label, arr, want, never in CASES:
        r = C.ref(label, arr, dynamic)
        parent = R.parent(arr, dynamic)
        assert bytes(E.png_independent_checks(r.file, arr)) == r.stream.tobytes(), label
        assert len(r.file) <= len(parent) and (r.which >= R.MATCH_FIXED or r.file == parent), label
        assert set(want) <= set(r.tokens) and not set(never) & set(r.tokens), label
        wins.append(r.which >= R.MATCH_FIXED)
        if label in ("checker_gray", "tile_rgb"):
            assert 4 * len(r.file) < len(parent), (label, len(r.file), len(parent))
    assert 2 * sum(wins) >= len(wins) and len(wins) - sum(wins) >= 5, (sum(wins), len(wins))


def test_the_set_meets_its_edges():
    refs = {label: C.ref(label, arr, True) for label, arr, _, _ in CASES}
    used = {label: {R.distance_symbol(d)[0] for _, k, d in r.tokens if k} for label, r in refs.items()}
    assert used["every_distance_symbol"] == set(range(26))
    assert used["one_distance_symbol"] == {1} and refs["one_distance_symbol"].which >= R.MATCH_FIXED
    assert not used["d3_inside_group"] and not used["far_before_window"] and not used["far_5_refused"]
    assert {len(r.stream) for r in refs.values()} >= {2, 3, 4, 5, 1023, 1024, 1025, 2049}
    assert {r.which for r in refs.values()} == {0, 1, 2, 3}
    assert any(k == 258 for r in refs.values() for _, k, _ in r.tokens)
    assert any(k > d > 1 for r in refs.values() for _, k, d in r.tokens)  # a match that overlaps its source
    label, px = C.GRAY16
    r16 = R.encode_rows(ref_penc16.be_rows(px), 16, True)
    assert r16.which == R.MATCH_DYN and r16.file[24] == 16 and len(r16.file) < len(ref_penc16.encode(px, True).file)
    assert np.array_equal(ref_penc16.read(r16.file).px, px)


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitized"])
def test_header_program(tmp_path, flags):
    exe, src = str(tmp_path / "penc_match_emu"), str(tmp_path / "hist.txt")
    subprocess.run(["g++", "-std=c++17", "-I" + CSRC, "-o", exe, *flags,
                    os.path.join(ROOT, "tests", "native", "penc_match_emu.cpp")], check=True)
    refs = [(label, C.ref(label, arr, True)) for label, arr, _, _ in CASES]
    refs = [(label, r) for label, r in refs if r.litlen is not None]
    assert len(refs) >= 30
    with open(src, "w") as f:
        for _, r in refs:
            f.write(" ".join(map(str, r.lit_freq + r.dist_freq)) + "\n")
    out = subprocess.run([exe, src], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert len(out) == len(refs)
    for (label, r), line in zip(refs, out):
        v = [int(x) for x in line.split()]
        assert v[:286] == r.litlen and v[286:316] == r.distlen, label
        assert v[316:319] == [r.hdr_bits, r.bits[R.MATCH_DYN], r.bits[R.MATCH_FIXED]], label
        hdr = np.asarray(v[319:], "<u4").tobytes()
        exp = R.header(r.litlen, r.distlen)[0].tobytes()
        assert hdr[:len(exp)] == exp and not any(hdr[len(exp):]), label


def test_option_row():
    """The row "penc_match" stands in options.cpp's second table and takes 0 and 1 only."""
    import test_options_cpu as TO
    out = subprocess.run([TO.build_options_main(), "apply", "penc_match", "0", "penc_match", "1", "penc_match", "2"],
                         check=True, capture_output=True, text=True).stdout.split("\n")
    assert [ln.split("\t")[:3] for ln in out[:3]] == [["0", "0", "1"], ["0", "1", "0"], ["1", "0", "1"]]  # status, stored, unchanged
