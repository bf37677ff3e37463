"""The corpus of all_formats_cases.py, checked without a GPU: every family holds its stated members, the labels are
unique, no file is over 128 px a side, Pillow's decode of every file made from an array is that array, the failing
files cover five formats, and the 8-bit TIFF members go through tests/native/tiff_emu.cpp as test_tiff_cpu.py builds
it."""
import io

import numpy as np
from PIL import Image

import all_formats_cases as A
from test_tiff_cpu import _run, emu  # noqa: F401  (the fixture that builds the emulator, and its runner)

# family -> words each of which some member's label must hold
MEMBERS = {
    "jpeg": ["gray", "4:4:4", "4:2:0 restart", "4:2:2", "progressive", "4:4:0", "cmyk", "ycck", "multiscan"],
    "png": ["RGB", "palette", "RGBA Adam7", "noise chunked", "gray16", "rgb16"],
    "gif": ["global table", "local table", "interlaced", "transparent index"],
    "webp": ["lossless index", "lossless predictor", "lossless cache", "lossy seg_delta", "alpha raw_f", "alpha vp8l"],
    "bmp": ["24-bit", "RLE8", "32-bit masks alpha", "8-bit palette bottom-up"],
    "tiff": ["raw gray MM", "WhiteIsZero lzw", "La8 packbits", "Rgb8 lzw pred rps 7", "Rgba8 lzw pred tiles", "over LDS"],
    "tiff_deflate": ["dynamic", "stored pred"],
    "tiff16": ["gray16 II", "La16", "Rgb16 MM lzw pred", "Rgba16 tiles"],
}


def _format(data):
    for magic, name in ((b"\xff\xd8", "jpeg"), (b"\x89PNG", "png"), (b"GIF8", "gif"), (b"RIFF", "webp"), (b"BM", "bmp"),
                        (b"II", "tiff"), (b"MM", "tiff")):
        if data.startswith(magic):
            return name
    return "unknown"


def test_families_and_labels():
    corpus = A.corpus()
    assert len(corpus) >= 40
    labels = [m[1] for m in corpus] + [b[0] for b in A.bad()]
    assert len(set(labels)) == len(labels)
    assert [f for f in A.FAMILIES if f not in MEMBERS] == [] and {m[0] for m in corpus} == set(A.FAMILIES)
    for fam, words in MEMBERS.items():
        have = [m[1] for m in corpus if m[0] == fam]
        for w in words:
            assert any(w in label for label in have), (fam, w, have)
        shapes = [m[3].shape[:2] for m in corpus if m[0] == fam]
        assert len(set(shapes)) >= 2, fam
    assert A.BMP_NO_INDEX in labels


def test_sizes_types_and_neighbours():
    corpus = A.corpus()
    for fam, label, data, ref, bits in corpus:
        assert ref.ndim == 3 and max(ref.shape[:2]) <= A.MAX_SIDE, label
        assert ref.dtype == (np.uint16 if bits == 16 else np.uint8), label
        assert _format(data) == {"tiff_deflate": "tiff", "tiff16": "tiff"}.get(fam, fam), label
    for (_, a, _, ra, _), (_, b, _, rb, _) in zip(corpus, corpus[1:]):
        assert ra.shape[:2] != rb.shape[:2], (a, b)
    lds = 65536  # kTiffLdsOut: both forms of a segment that decodes to more
    by = {m[1]: m for m in corpus}
    assert 144 * 128 * 4 > lds and by["tiff Rgba8 lzw pred segment over LDS"][3].shape == (128, 121, 4)
    assert by["tiff16 Rgba16 deflate pred strip over LDS"][3].size * 2 > lds


def test_pillow_references_equal_their_sources():
    src = A.sources()
    assert len(src) >= 8
    for fam, label, data, ref, bits in A.corpus():
        if label in src:
            assert np.array_equal(ref, src[label]), label
        if fam == "tiff16" and ref.shape[2] != 2:  # Pillow holds 16-bit gray, and 8 bits of 16-bit colour
            pil = np.asarray(Image.open(io.BytesIO(data)))
            assert np.array_equal(pil.reshape(pil.shape[0], pil.shape[1], -1), ref if ref.shape[2] == 1 else ref >> 8), label


def test_bad_files_and_the_order():
    bad = A.bad()
    assert len(bad) >= 8 and len({_format(b[1]) for b in bad}) >= 5
    assert {b[2] for b in bad} == {A.CORRUPT, A.UNSUPPORTED}
    order = A.order()
    assert order[0][2] is None and any(m[2] is None for m in order[-4:-1]) and order[-1][2] is not None
    for label, _, _, fam in bad:  # a stream-level refusal stands between two good files of its own format
        if fam:
            k = next(i for i, m in enumerate(order) if m[0] == label)
            assert order[k - 1][2] == fam == order[k + 1][2], label
    rots = A.rotations()
    assert len(rots) == 1 + len(A.FAMILIES)
    for (name, batch), fam in zip(rots[1:], A.FAMILIES):
        assert batch[0][2] == fam and sorted(m[0] for m in batch) == sorted(m[0] for m in order), name
    assert A.rotated(order, A.BMP_NO_INDEX)[0][0] == A.BMP_NO_INDEX


def test_tiff_members_through_the_emulator(emu, tmp_path):
    members = [m for m in A.corpus() if m[0] == "tiff"]
    assert len(members) >= 6
    for fam, label, data, ref, bits in members:
        assert _run(emu, tmp_path, data) == (0, "", ref.tobytes()), label
    short = next(b for b in A.bad() if b[0] == "bad tiff stream: short LZW")
    st, why, raw = _run(emu, tmp_path, short[1])
    assert st == 2 and why and raw is None


def test_large_members_for_the_budget():
    large = A.large()
    assert {m[0] for m in large} == set(A.FAMILIES) and len({m[1] for m in large}) == len(large)
    for fam, label, data in large:
        w, h = Image.open(io.BytesIO(data)).size
        assert 400 <= min(w, h) and max(w, h) <= 700, (label, w, h)
