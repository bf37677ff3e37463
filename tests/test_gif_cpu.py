"""GIF first frames (context option "gif") without a GPU.

tests/ref_gif.py restates image 0.25's GifDecoder; here it is pinned to Pillow
wherever the two agree: the indices in mode P and the RGBA conversion byte for
byte on every full-screen crafted file, a transparent index included.  For a
frame smaller than the screen Pillow and image agree inside the frame's
rectangle only: image leaves (0,0,0,0) outside it, Pillow paints the
background palette colour there (under alpha 0 only where the background index
is the transparent one) and grows the canvas for a frame that reaches past the
screen.  The test asserts that this is the whole difference.

The native parser (host/gif_header.cpp) is built with g++ as
test_jpeg_multiscan_cpu.py builds its own: fields on every crafted layout,
every truncation length of two files, the refusal texts.  The step logic of
dg_gif.h runs as tests/native/gif_emu.cpp and must equal ref_gif on every
stream, frame and refusal case; the same sources run as a stand-alone program
under AddressSanitizer and UBSan over the crafted files and their truncations.
dg_probe and dg_sample_align take a GIF through the C ABI."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import gif_cases as C
import gif_craft as G
import ref_gif as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
SO = os.path.join(NATIVE, "libgif_emu.so")
SRCS = [os.path.join(NATIVE, "gif_emu.cpp"), os.path.join(CSRC, "host", "gif_header.cpp")]
FIELDS = ["status", "version", "width", "height", "left", "top", "fw", "fh", "interlace", "has_global", "has_local",
          "npal", "transparent", "min_code_size", "data_off", "nbytes", "closed", "nruns"]


@pytest.fixture(scope="module")
def emu():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("dg_types.h", "dg_gif.h", "host/gif_header.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"  # build beside it and rename (parallel test workers)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", tmp] + SRCS, check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    E.gif_parse.restype = ctypes.c_int
    E.gif_decode.restype = ctypes.c_int
    return E


def _parse(E, data):
    f = (ctypes.c_int64 * 18)()
    pal = (ctypes.c_uint8 * 1024)()
    why = ctypes.c_char_p()
    st = E.gif_parse(data, ctypes.c_size_t(len(data)), f, pal, ctypes.byref(why))
    return st, (why.value or b"").decode(), dict(zip(FIELDS, list(f))), np.frombuffer(pal, np.uint8).reshape(256, 4)


def _decode(E, data, w, h):
    cap = w * h * 4
    buf = (ctypes.c_uint8 * max(cap, 1))()
    why, steps = ctypes.c_char_p(), ctypes.c_uint64()
    st = E.gif_decode(data, ctypes.c_size_t(len(data)), buf, ctypes.c_size_t(cap), ctypes.byref(why), ctypes.byref(steps))
    return st, (why.value or b"").decode(), np.frombuffer(buf, np.uint8, cap).reshape(h, w, 4), steps.value


STREAMS = C.stream_cases()
FRAMES = C.frame_cases()
REFUSALS = C.refusals()


def test_ref_gif_equals_pillow_on_full_screen_files():
    n = 0
    for label, data in STREAMS + FRAMES:
        st, why, ref, h = R.decode(data)
        assert st == R.OK, (label, why)
        if (h.left, h.top, h.fw, h.fh) != (0, 0, h.width, h.height):
            continue
        im = Image.open(io.BytesIO(data))
        assert im.mode == "P" and im.size == (h.width, h.height), label
        assert np.array_equal(np.asarray(im), h.indices), label
        if "past the table" in label:  # Pillow ignores such an index too; the pixels compare as any others
            assert h.transparent >= h.npal
        assert np.array_equal(np.asarray(im.convert("RGBA")), ref), label
        n += 1
    assert n >= 40
    assert any(R.decode(d)[3].transparent >= 0 and (R.decode(d)[2][..., 3] == 0).any() for _, d in FRAMES)


def test_ref_gif_and_pillow_differ_outside_a_sub_frame_only():
    n = 0
    for label, data in FRAMES:
        st, why, ref, h = R.decode(data)
        assert st == R.OK, (label, why)
        if (h.left, h.top, h.fw, h.fh) == (0, 0, h.width, h.height):
            continue
        im = Image.open(io.BytesIO(data))
        pil = np.asarray(im.convert("RGBA"))
        assert pil.shape[0] >= h.height and pil.shape[1] >= h.width, label  # (Pillow grows the canvas)
        pil = pil[:h.height, :h.width]
        inside = np.zeros((h.height, h.width), bool)
        inside[h.top:h.top + h.fh, h.left:h.left + h.fw] = True
        assert np.array_equal(pil[inside], ref[inside]), label
        assert (ref[~inside] == 0).all(), label
        bg = h.pal[im.info.get("background", 0)]
        want_a = 0 if im.info.get("transparency") == im.info.get("background", 0) else 255
        assert (pil[~inside][:, :3] == bg[:3]).all() and (pil[~inside][:, 3] == want_a).all(), label
        n += 1
    assert n >= 7


def test_native_parser_fields_on_every_layout(emu):
    for label, data in STREAMS + FRAMES:
        rs, rw, h = R.parse(data)
        st, why, f, pal = _parse(emu, data)
        assert (st, why) == (rs, rw) == (R.OK, ""), label
        want = dict(status=0, version=h.version, width=h.width, height=h.height, left=h.left, top=h.top, fw=h.fw,
                    fh=h.fh, interlace=h.interlace, has_global=h.has_global, has_local=h.has_local, npal=h.npal,
                    transparent=h.transparent, min_code_size=h.min_code_size, data_off=h.data_off, nbytes=h.nbytes,
                    closed=int(h.closed), nruns=0 if h.closed else len(h.runs))
        assert f == want, (label, f, want)
        assert np.array_equal(pal, h.pal), label
    closed = {label: _parse(emu, data)[2]["closed"] for label, data in STREAMS}
    assert closed["sub-blocks 255"] == 1 and closed["sub-blocks 1"] == 0 and closed["sub-blocks mixed"] == 0
    assert closed["sub-blocks 100"] == 0 and closed["sub-blocks 255 then 254s"] == 0 and closed["photo 1x1"] == 1


def test_every_truncation_of_two_files_returns_a_status(emu):
    pal = G.palette(8, 41)
    files = [G.gif(13, 11, C.photo(11, 13, 8, 42), 3, gct=pal, lct=G.palette(8, 43), sub=[9, 4],
                   before=[G.comment(), G.gce(transparent=1), G.netscape()]),
             G.gif(40, 30, C.noise(30, 40, 256, 44), 8, gct=G.palette(256, 45), version=b"87a", interlace=True)]
    for data in files:
        seen = set()
        for n in range(len(data) + 1):
            cut = data[:n]
            rs, rw, _ = R.parse(cut)
            st, why, _, _ = _parse(emu, cut)
            assert (st, why) == (rs, rw), (n, st, why, rs, rw)
            assert st in (R.OK, R.UNSUPPORTED, R.CORRUPT)
            seen.add(why)
            if st == R.OK:  # the chain is whole: the decode gives a status too, and the whole file's pixels
                ds, dw, ref, h = R.decode(cut)
                es, ew, got, _ = _decode(emu, cut, h.width, h.height)
                assert (es, ew) == (ds, dw) == (R.OK, ""), n
                assert np.array_equal(got, ref), n
        assert {"not a GIF", "GIF: truncated logical screen descriptor", "GIF: truncated global colour table",
                "GIF: no image descriptor", "GIF: truncated image descriptor", "GIF: truncated image data",
                "GIF: truncated sub-block chain", ""} <= seen, seen
    assert "GIF: truncated extension" in {R.parse(files[0][:n])[1] for n in range(len(files[0]))}
    assert "GIF: truncated local colour table" in {R.parse(files[0][:n])[1] for n in range(len(files[0]))}


def test_refusal_statuses_and_texts(emu):
    for label, data, status, text in REFUSALS:
        rs, rw, _, h = R.decode(data)
        assert (rs, rw) == (status, text), label
        ps, pw, f, _ = _parse(emu, data)
        if text.startswith("GIF: LZW code") or text in (R.WHY_SHORT, R.WHY_PALETTE):  # the stream's, not the header's
            assert ps == R.OK, label
            es, ew, _, _ = _decode(emu, data, h.width, h.height)
        else:
            assert (ps, pw) == (status, text), label
            es, ew, _, _ = _decode(emu, data, 1, 1)
        assert (es, ew) == (status, text), (label, es, ew)


@pytest.mark.parametrize("which", ["streams", "frames"])
def test_step_logic_equals_ref_gif(emu, which):
    for label, data in (STREAMS if which == "streams" else FRAMES):
        st, why, ref, h = R.decode(data)
        es, ew, got, steps = _decode(emu, data, h.width, h.height)
        assert (es, ew) == (st, why) == (R.OK, ""), label
        assert np.array_equal(got, ref), (label, int((got != ref).sum()))
        assert 0 < steps <= h.nbytes * 8 // (h.min_code_size + 1) + 2, label  # the device loop's bound
    if which == "streams":  # 64 codes per step where nothing cuts it short
        d = dict(STREAMS)["noise 128x64 full clears"]
        h = R.decode(d)[3]
        assert _decode(emu, d, h.width, h.height)[3] < h.nbytes * 8 / 9 / 50


def test_standalone_program_under_the_sanitizers(tmp_path):
    """Host code with its own main, built with AddressSanitizer and UBSan: the parser and the emulator over the
    crafted files, the refusals and every truncation of the small ones."""
    exe = str(tmp_path / "gif_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DGIF_MAIN", "-I" + CSRC, "-o", exe] + SRCS, check=True)
    paths = []
    for k, data in enumerate([d for _, d in STREAMS + FRAMES] + [d for _, d, _, _ in REFUSALS]):
        paths.append(str(tmp_path / ("f%d.gif" % k)))
        with open(paths[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[2]) > 5000 and int(words[4]) >= len(STREAMS) + len(FRAMES), r.stdout
    assert int(words[6]) > 0 and int(words[8]) > 0, r.stdout


def test_probe_and_sample_align_take_a_gif():
    from datago_amd import _lib as L
    from datago_amd import synth
    data = G.gif(200, 120, C.photo(120, 200, 8, 51), 3, gct=G.palette(8, 52), interlace=True)
    st, info = L.probe(data)
    assert st == L.DG_OK and info.format == L.DG_FMT_GIF == 3
    assert (info.width, info.height, info.components, info.bit_depth) == (200, 120, 4, 8)
    assert info.progressive == 1 and info.gpu_supported == 0
    st, info = L.probe(dict(FRAMES)["offset inside"])
    assert st == L.DG_OK and (info.width, info.height, info.progressive) == (30, 20, 0)  # the screen, not the frame
    st, info = L.probe(data[:10])
    assert st == L.DG_ERR_CORRUPT and info.format == L.DG_FMT_GIF and "truncated logical screen" in L.last_error()
    st, info = L.probe(data[:-8])
    assert st == L.DG_ERR_CORRUPT and "truncated sub-block chain" in L.last_error()
    st, info = L.probe(b"RIFF\x00\x00\x00\x00WEBPVP8 ")
    assert st == L.DG_ERR_CORRUPT and "unknown image format" in L.last_error()
    # the reference payload of a sample: a GIF first member decides the others' bucket, as a PNG twin does
    table = L.BucketTable(224, 16, 0.5, 2.0)
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    twin = io.BytesIO()
    Image.fromarray(np.zeros((120, 200, 4), np.uint8)).save(twin, "PNG")
    got = L.sample_align(table, [data, jpg, jpg])
    assert got == L.sample_align(table, [twin.getvalue(), jpg, jpg])
    assert got[0] == -1 and got[1] == got[2] >= 0
    assert got != L.sample_align(table, [jpg, jpg, jpg])  # (the GIF's 200x120, not the JPEG's 64x48, chose the bucket)
    # a broken GIF is skipped like any payload that fails to load: the JPEG behind it is the reference
    assert L.sample_align(table, [data[:10], jpg, jpg]) == L.sample_align(table, [b"junk", jpg, jpg])
