"""Windows bitmaps (context option "bmp") without a GPU.

tests/ref_bmp.py restates the decode; here it is pinned to Pillow byte for byte
on every decodable crafted file except the few that run into one of Pillow's two
RLE quirks (each flagged with its reason in bmp_cases.py; their share is
capped).  For the stream irregularities the library refuses, the test shows
that Pillow's result differs from the reading that continues a run onto the
next row and leaves skipped pixels zero, which is why they go to the CPU.

The native parser (host/bmp_header.cpp) is built with g++ as test_gif_cpu.py
builds its own: fields on every crafted layout, every truncation length of two
files, the refusal texts.  The step logic of dg_bmp.h runs as
tests/native/bmp_emu.cpp and must equal ref_bmp on every case and refusal; the
same sources run as a stand-alone program under AddressSanitizer and UBSan over
the crafted files and their truncations.  dg_probe and dg_sample_align take a
BMP through the C ABI."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import bmp_cases as C
import bmp_craft as G
import ref_bmp as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
SO = os.path.join(NATIVE, "libbmp_emu.so")
SRCS = [os.path.join(NATIVE, "bmp_emu.cpp"), os.path.join(CSRC, "host", "bmp_header.cpp")]
FIELDS = ["status", "header_size", "width", "height", "top_down", "bits", "compression", "stride", "data_off",
          "data_len", "out_c", "pos_r", "pos_g", "pos_b", "pos_a", "npal"]

PIXELS = C.pixel_cases()
RLES = C.rle_cases()
REFUSALS = C.refusals()


@pytest.fixture(scope="module")
def emu():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("dg_types.h", "dg_bmp.h", "host/bmp_header.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"  # build beside it and rename (parallel test workers)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", tmp] + SRCS, check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    E.bmp_parse.restype = ctypes.c_int
    E.bmp_decode.restype = ctypes.c_int
    return E


def _parse(E, data):
    f = (ctypes.c_int64 * 16)()
    pal = (ctypes.c_uint8 * 1024)()
    why = ctypes.c_char_p()
    st = E.bmp_parse(data, ctypes.c_size_t(len(data)), f, pal, ctypes.byref(why))
    return st, (why.value or b"").decode(), dict(zip(FIELDS, list(f))), np.frombuffer(pal, np.uint8).reshape(256, 4)


def _decode(E, data, w, h, c):
    cap = w * h * c
    buf = (ctypes.c_uint8 * max(cap, 1))()
    why, steps, hops = ctypes.c_char_p(), ctypes.c_uint64(), ctypes.c_uint64()
    st = E.bmp_decode(data, ctypes.c_size_t(len(data)), buf, ctypes.c_size_t(cap), ctypes.byref(why),
                      ctypes.byref(steps), ctypes.byref(hops))
    return st, (why.value or b"").decode(), np.frombuffer(buf, np.uint8, cap).reshape(h, w, c), steps.value, hops.value


def _pillow(data, c):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im.convert("RGBA" if c == 4 else "RGB"))  # (Pillow reports 1 / L / P for palette files)


def test_ref_bmp_equals_pillow_on_every_unflagged_case():
    n = flagged = rgba = 0
    for label, data, pillow, reason in PIXELS + RLES:
        st, why, ref, h = R.decode(data)
        assert st == R.OK, (label, why)
        assert ref.shape == (h.height, h.width, h.out_c), label
        n += 1
        rgba += h.out_c == 4
        if not pillow:  # only the two quirks, each with its reason; Pillow really is off there
            assert reason in (C.QUIRK_PARITY, C.QUIRK_ODD4), label
            if reason == C.QUIRK_PARITY:
                assert h.data_off % 2 == 1 and h.compression == R.RLE8, label
            else:
                assert h.compression == R.RLE4, label
            assert not np.array_equal(_pillow(data, h.out_c), ref), label
            flagged += 1
            continue
        got = _pillow(data, h.out_c)
        assert got.shape == ref.shape and np.array_equal(got, ref), label
        if h.out_c == 4:
            assert Image.open(io.BytesIO(data)).mode == "RGBA", label
    assert n >= 300 and rgba >= 30
    assert 0 < flagged * 10 <= n, (flagged, n)  # the Pillow pin does not thin out


def _other_reading(data):
    """An RLE stream read the other way: a run that passes its row's end continues on the next row, a delta, an
    early end-of-line or an early end of the stream leaves zero bytes (not colour 0)."""
    st, why, h = R.parse(data)
    assert st == R.OK
    W, H, rle4 = h.width, h.height, h.compression == R.RLE4
    out = np.zeros((H * W, 3), np.uint8)
    s = data[h.data_off:]
    pos = x = y = 0

    def put(v):
        nonlocal x, y
        if x >= W:
            x, y = 0, y + 1
        if y < H and v < h.npal:
            out[y * W + x] = h.pal[v][:3]
        x += 1
    while pos + 2 <= len(s) and y < H:
        a, b = s[pos], s[pos + 1]
        pos += 2
        if a:
            for t in range(a):
                put(b if not rle4 else (b >> 4 if t % 2 == 0 else b & 15))
        elif b == 0:
            x, y = 0, y + 1
        elif b == 1:
            break
        elif b == 2:
            if pos + 2 > len(s):
                break
            x, y = x + s[pos], y + s[pos + 1]
            pos += 2
        else:
            nb = (b + 1) // 2 if rle4 else b
            raw = s[pos:pos + nb]
            pos += (nb + 1) & ~1
            px = [v for byte in raw for v in (byte >> 4, byte & 15)] if rle4 else list(raw)
            for v in px[:b]:
                put(v)
    return out.reshape(H, W, 3)[::-1]


def test_pillow_differs_from_the_other_reading_on_every_stream_irregularity():
    """Why these go to the CPU: the two readings of such a stream give different pixels."""
    n = 0
    for label, data, status, text in REFUSALS:
        if text not in (R.WHY_ROW, R.WHY_DELTA, R.WHY_SHORT):
            continue
        assert status == R.UNSUPPORTED, label
        try:
            pil = _pillow(data, 3)
        except (OSError, ValueError):  # Pillow clips, comes up short and gives up ("not enough image data")
            n += 1
            continue
        other = _other_reading(data)
        assert pil.shape == other.shape and not np.array_equal(pil, other), label
        n += 1
    assert n >= 20


def test_sixteen_bit_files_are_refused_for_pillows_truncating_expansion():
    """Pillow expands a 5-bit field as v * 255 // 31 (3 -> 24, 4 -> 32); a rounded table gives 25 and 33.  Nothing
    here can pin either, so 16-bit files stay with the CPU."""
    px = np.array([[3 << 10 | 4 << 5 | 31, 0]], np.uint16)
    data = G.bmp(2, 1, 16, px)
    got = _pillow(data, 3)
    assert tuple(got[0, 0]) == (3 * 255 // 31, 4 * 255 // 31, 255) == (24, 32, 255)
    assert (round(3 * 255 / 31), round(4 * 255 / 31)) == (25, 33)
    assert R.decode(data)[:2] == (R.UNSUPPORTED, "BMP: 16 bits per pixel")


def test_native_parser_fields_on_every_layout(emu):
    for label, data, _, _ in PIXELS + RLES:
        rs, rw, h = R.parse(data)
        st, why, f, pal = _parse(emu, data)
        assert (st, why) == (rs, rw) == (R.OK, ""), label
        want = dict(status=0, header_size=h.header_size, width=h.width, height=h.height, top_down=h.top_down,
                    bits=h.bits, compression=h.compression, stride=h.stride, data_off=h.data_off,
                    data_len=h.data_len, out_c=h.out_c, pos_r=h.pos[0], pos_g=h.pos[1], pos_b=h.pos[2],
                    pos_a=h.pos[3], npal=h.npal)
        assert f == want, (label, f, want)
        assert np.array_equal(pal, h.pal), label
    sizes = {_parse(emu, d)[2]["header_size"] for _, d, _, _ in PIXELS}
    assert sizes == {12, 40, 108, 124}
    assert {_parse(emu, d)[2]["data_off"] % 4 for _, d, _, _ in PIXELS} == {0, 1, 2, 3}


def test_every_truncation_of_two_files_returns_a_status(emu):
    ph = C.photo(7, 13, 16, 41)
    files = [G.bmp(13, 7, 4, data=G.rle_bytes(G.rle_commands(ph, True, "mixed"), True), compression=G.RLE4,
                   pal=G.palette(16, 42), gap=3),
             G.bmp(11, 5, 32, C.rgb(5, 11, 43, 4), compression=G.BITFIELDS, masks=G.MASKS32[5][:3]),
             G.bmp(9, 4, 8, C.noise(4, 9, 200, 44), pal=G.palette(200, 45), header=124)]
    for data in files:
        seen = set()
        for n in range(len(data) + 1):
            cut = data[:n]
            rs, rw, _ = R.parse(cut)
            st, why, _, _ = _parse(emu, cut)
            assert (st, why) == (rs, rw), (n, st, why, rs, rw)
            assert st in (R.OK, R.UNSUPPORTED, R.CORRUPT)
            seen.add(why)
            if st == R.OK:  # the headers are whole: the decode gives a status too
                ds, dw, ref, h = R.decode(cut)
                es, ew, got, _, _ = _decode(emu, cut, h.width, h.height, h.out_c)
                assert (es, ew) == (ds, dw), (n, es, ew, ds, dw)
                if ds == R.OK:
                    assert np.array_equal(got, ref), n
        assert {"not a BMP", "BMP: truncated file header", "BMP: truncated info header", ""} <= seen, seen
    texts = [{R.parse(f[:n])[1] for n in range(len(f))} for f in files]
    assert "BMP: truncated colour table" in texts[0] and "BMP: truncated colour table" in texts[2]
    assert "BMP: pixel data offset inside the headers or past the file" in texts[0]
    assert "BMP: truncated bit masks" in texts[1] and "BMP: pixel data truncated" in texts[1]
    assert R.WHY_SHORT in {R.decode(files[0][:n])[1] for n in range(len(files[0]))}


def test_refusal_statuses_and_texts(emu):
    for label, data, status, text in REFUSALS:
        rs, rw, _, h = R.decode(data)
        assert (rs, rw) == (status, text), label
        ps, pw, f, _ = _parse(emu, data)
        if text in R.STREAM_TEXTS:  # the stream's, not the header's
            assert ps == R.OK, label
            es, ew, _, _, _ = _decode(emu, data, h.width, h.height, h.out_c)
        else:
            assert (ps, pw) == (status, text), label
            es, ew, _, _, _ = _decode(emu, data, 1, 1, 4)
        assert (es, ew) == (status, text), (label, es, ew)
    texts = {t for _, _, _, t in REFUSALS}
    assert set(R.STREAM_TEXTS) <= texts and len(texts) >= 24


@pytest.mark.parametrize("which", ["pixels", "rle"])
def test_lane_routines_equal_ref_bmp(emu, which):
    for label, data, _, _ in (PIXELS if which == "pixels" else RLES):
        st, why, ref, h = R.decode(data)
        es, ew, got, steps, hops = _decode(emu, data, h.width, h.height, h.out_c)
        assert (es, ew) == (st, why) == (R.OK, ""), (label, es, ew)
        assert np.array_equal(got, ref), (label, int((got != ref).sum()))
        if which == "rle":
            assert 0 < steps <= h.data_len // 128 + 2, label  # the device loop's bound
    if which == "rle":
        by = {label: d for label, d, _, _ in RLES}
        # several absolute blocks in one window: the hop loop runs more than once per step, never 64 times
        _, _, _, steps, hops = _decode(emu, by["RLE8 131x3 absolute even"], 131, 3, 3)
        assert hops > 2 * steps and hops <= 16 * steps
        # runs only: no hop at all
        assert _decode(emu, by["RLE8 131x3 runs of 1"], 131, 3, 3)[4] == 0
        # a 255-pixel absolute block spans more than one window
        d = by["RLE8 510x2 run 255 and absolute 255"]
        assert _decode(emu, d, 510, 2, 3)[3] >= 4
        # fewer than 64 commands in the whole file: one step
        assert _decode(emu, by["RLE8 9x3 runs"], 9, 3, 3)[3] == 1


def test_standalone_program_under_the_sanitizers(tmp_path):
    """Host code with its own main, built with AddressSanitizer and UBSan: the parser and the emulator over the
    crafted files, the refusals and every truncation of the small ones."""
    exe = str(tmp_path / "bmp_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DBMP_MAIN", "-I" + CSRC, "-o", exe] + SRCS, check=True)
    paths = []
    for k, data in enumerate([d for _, d, _, _ in PIXELS + RLES] + [d for _, d, _, _ in REFUSALS]):
        paths.append(str(tmp_path / ("f%d.bmp" % k)))
        with open(paths[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[2]) > 20000 and int(words[4]) >= len(PIXELS) + len(RLES), r.stdout
    assert int(words[6]) > 0 and int(words[8]) > 0, r.stdout


def test_option_row_takes_0_and_1_only():
    """The row "bmp" through apply_option on a fresh Options (tests/native/options_main.cpp), held to what
    test_options_cpu.py holds every STRICT row to.  It stands in options.cpp's second table, which find_option
    reads after the first."""
    import test_options_cpu as TO
    exe = TO.build_options_main()
    names = [ln.split("\t")[0] for ln in subprocess.run([exe, "list"], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert "bmp" not in names and "gif" in names  # one row per key across the two tables
    case = TO.strict()
    values = list(case["stored"]) + list(case["rejected"])
    out = subprocess.run([exe, "apply"] + [s for v in values for s in ("bmp", str(v))], check=True, capture_output=True,
                         text=True).stdout.split("\n")[:-1]
    assert len(out) == len(values)
    for v, ln in zip(values, out):
        st, field, same, text = ln.split("\t")
        if v in case["stored"]:
            assert (int(st), field, text) == (0, str(case["stored"][v]), ""), (v, ln)
            assert int(same) == (v == 0), v  # off by default: storing 0 changes nothing, storing 1 does
        else:
            assert int(st) == 1 and int(same) == 1, (v, ln)
            assert text == 'dg_ctx_set_option("bmp", %d): %s' % (v, case["rejected"][v]), (v, ln)


def test_probe_and_sample_align_take_a_bmp():
    from datago_amd import _lib as L
    from datago_amd import synth
    data = G.bmp(200, 120, 24, C.rgb(120, 200, 51), top_down=True)
    st, info = L.probe(data)
    assert st == L.DG_OK and info.format == L.DG_FMT_BMP == 5
    assert (info.width, info.height, info.components, info.bit_depth) == (200, 120, 3, 8)
    assert info.gpu_supported == 0
    st, info = L.probe(dict((c[0], c[1]) for c in PIXELS)["bf32:5 131x67"])
    assert st == L.DG_OK and (info.format, info.width, info.height, info.components) == (5, 131, 67, 4)
    st, info = L.probe(dict((c[0], c[1]) for c in REFUSALS)["16-bit 555"])  # named, though no option decodes it
    assert st == L.DG_OK and (info.format, info.width, info.height, info.gpu_supported) == (5, 5, 3, 0)
    st, info = L.probe(data[:20])
    assert st == L.DG_ERR_CORRUPT and info.format == L.DG_FMT_BMP and "truncated info header" in L.last_error()
    st, info = L.probe(data[:-8])
    assert st == L.DG_ERR_CORRUPT and "pixel data truncated" in L.last_error()
    # the reference payload of a sample: a BMP first member decides the others' bucket, as a PNG twin does
    table = L.BucketTable(224, 16, 0.5, 2.0)
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    twin = io.BytesIO()
    Image.fromarray(np.zeros((120, 200, 3), np.uint8)).save(twin, "PNG")
    got = L.sample_align(table, [data, jpg, jpg])
    assert got == L.sample_align(table, [twin.getvalue(), jpg, jpg])
    assert got[0] == -1 and got[1] == got[2] >= 0
    assert got != L.sample_align(table, [jpg, jpg, jpg])  # (the BMP's 200x120, not the JPEG's 64x48, chose the bucket)
    # a broken BMP is skipped like any payload that fails to load: the JPEG behind it is the reference
    assert L.sample_align(table, [data[:20], jpg, jpg]) == L.sample_align(table, [b"junk", jpg, jpg])
