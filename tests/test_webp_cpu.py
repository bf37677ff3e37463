"""Lossless WebP (context option "webp") without a GPU.

tests/ref_webp.py restates the container walk and the VP8L decode; here it is
pinned to Pillow (libwebp) byte for byte, mode and pixels, on every Pillow-made
file and on every crafted file Pillow opens.  Two crafted files are the one place
where the library's rule is not Pillow's: in an extended file the library takes
the VP8X alpha flag (image-webp's rule, as recalled), Pillow the VP8L header's
bit; there the RGB channels are compared and the difference is asserted.

The native parser (host/webp_header.cpp) and the walk and lane routines of
dg_vp8l.h run as tests/native/vp8l_emu.cpp, built with g++ on demand, and must
equal ref_webp on every case, wave-wide steps included; the same sources run as a
stand-alone program under AddressSanitizer and UBSan over all cases and their
truncations.  dg_probe and dg_sample_align take a lossless WebP through the C ABI
(the option's values need a context: tests/test_gpu_webp.py)."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import ref_webp as R
import webp_cases as K
import webp_craft as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
SO = os.path.join(NATIVE, "libvp8l_emu.so")
SRCS = [os.path.join(NATIVE, "vp8l_emu.cpp"), os.path.join(CSRC, "host", "webp_header.cpp")]
FIELDS = ["status", "extended", "alpha", "canvas_w", "canvas_h", "width", "height", "data_off", "nbytes"]
STATUS = {"OK": 0, "UNSUPPORTED": 1, "CORRUPT": 2}
ALPHA_RULE_DIFFERS = {"extended_no_alpha", "extended_alpha_flag_header_clear"}

PILLOW = K.pillow_cases()
CRAFTED = K.crafted_cases()
REFUSALS = K.refusals()


@pytest.fixture(scope="module")
def emu():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("dg_types.h", "dg_vp8l.h", "host/webp_header.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"  # build beside it and rename (parallel test workers)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", tmp] + SRCS, check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    E.webp_parse.restype = ctypes.c_int
    E.webp_decode.restype = ctypes.c_int
    return E


@pytest.fixture(scope="module")
def refs():
    """ref_webp's result per file, computed once."""
    return {name: R.decode(data) for name, data in PILLOW + CRAFTED}


def _parse(E, data):
    f = (ctypes.c_int64 * 9)()
    why = ctypes.c_char_p()
    st = E.webp_parse(data, ctypes.c_size_t(len(data)), f, ctypes.byref(why))
    return st, (why.value or b"").decode(), dict(zip(FIELDS, list(f)))


def _decode(E, data, cap=1 << 18):
    buf = (ctypes.c_uint8 * cap)()
    why, ch = ctypes.c_char_p(), ctypes.c_int()
    st = E.webp_decode(data, ctypes.c_size_t(len(data)), buf, ctypes.c_size_t(cap), ctypes.byref(why), ctypes.byref(ch))
    return st, (why.value or b"").decode(), ch.value, np.frombuffer(buf, np.uint8)


def test_ref_webp_equals_pillow(refs):
    opened = 0
    for name, data in PILLOW + CRAFTED:
        r = refs[name]
        assert r.status == "OK", (name, r.why)
        im = Image.open(io.BytesIO(data))  # (Pillow opens every file of the set; a refusal would raise here)
        pil = np.asarray(im)
        if name in ALPHA_RULE_DIFFERS:
            assert im.mode != r.mode and np.array_equal(pil[..., :3], r.pixels[..., :3]), name
        else:
            assert im.mode == r.mode, (name, im.mode, r.mode)
            assert np.array_equal(pil, r.pixels), (name, int((pil != r.pixels).sum()))
        opened += 1
    assert opened == len(PILLOW) + len(CRAFTED)
    assert R.decode(dict(CRAFTED)["index_past_table_used"]).pixels[0, 8:12].max() == 0  # an index past the table: 0x00000000
    a = R.decode(dict(CRAFTED)["alpha_bit_clear_alpha_data"])
    assert a.mode == "RGB" and a.pixels.shape[2] == 3


def test_the_pillow_made_set_covers_the_format(refs):
    rep = [refs[name].report for name, _ in PILLOW]
    for t in R.TRANSFORM_NAMES:
        assert any(t in r["transforms"] for r in rep), t
    assert any(r["cache_bits"] > 0 for r in rep)
    assert any(r["prefix_bits"] > 0 and r["groups"] > 1 for r in rep)
    assert any(r["copies"] > 0 for r in rep) and any(r["cache_hits"] > 0 for r in rep)
    packings = {b for r in rep for b in r["index_bits"]}
    assert packings == {0, 1, 2, 3}, packings  # 8 / 4 / 2 / 1 indices per packed pixel, as the files have them
    assert max(r["groups"] for r in rep) * 2 <= R.MAX_GROUPS


def test_native_walk_equals_ref_webp_on_every_case(emu, refs):
    for name, data in PILLOW + CRAFTED:
        r = refs[name]
        st, why, ch, got = _decode(emu, data)
        assert (st, why) == (0, ""), (name, st, why)
        assert ch == r.pixels.shape[2], name
        assert np.array_equal(got[:r.pixels.size], r.pixels.ravel()), name


def test_native_parser_fields_on_every_layout(emu):
    for name, data in PILLOW + CRAFTED:
        want = R.parse(data)
        st, why, f = _parse(emu, data)
        assert (st, why) == (0, ""), name
        assert f == dict(status=0, **want), (name, f, want)
    ext = _parse(emu, dict(CRAFTED)["extended_alpha"])[2]
    assert ext["extended"] == 1 and ext["alpha"] == 1 and (ext["canvas_w"], ext["canvas_h"]) == (9, 9)
    assert (ext["data_off"] - 5) % 2 == 0 and ext["data_off"] > 12 + 18 + 12  # behind VP8X and the padded odd ICCP chunk


def _with_sizes(data, n):
    """data[:n] with the RIFF and VP8L chunk sizes made to fit, so the bitstream itself ends early."""
    f = R.parse(data)
    cut = bytearray(data[:n])
    cut[4:8] = (n - 8).to_bytes(4, "little")
    cut[f["data_off"] - 9:f["data_off"] - 5] = (n - f["data_off"] + 5).to_bytes(4, "little")
    return bytes(cut)


def _truncation_files(refs):
    most = max(len(refs[name].report["transforms"]) for name, _ in PILLOW)
    return [min((d for name, d in PILLOW if len(refs[name].report["transforms"]) == most), key=len),
            dict(CRAFTED)["extended_alpha"]]


def test_every_truncation_of_two_files_returns_a_status(emu, refs):
    """Every length through the parser; with the sizes made to fit, the bitstream's own cuts through the decode
    (about 150 of them here, compared with ref_webp, which is Python; the sanitizer program below takes every
    one of these two files)."""
    # the Pillow-made file with the most transforms (libwebp writes two at most here), the smallest of those
    most = max(len(refs[name].report["transforms"]) for name, _ in PILLOW)
    assert most >= 2
    files = _truncation_files(refs)
    for data in files:
        seen = set()
        whole = R.decode(data)
        off = R.parse(data)["data_off"]
        fitted = set(range(off, len(data), max(1, (len(data) - off) // 150)))
        for n in range(len(data) + 1):
            cut = data[:n]
            try:
                R.parse(cut)
                rs, rw = 0, ""
            except R.Fail as e:
                rs, rw = STATUS[e.status], e.why
            st, why, _ = _parse(emu, cut)
            assert (st, why) == (rs, rw), (n, st, why, rs, rw)
            seen.add(why)
            if n in fitted:
                fit = _with_sizes(data, n)
                r = R.decode(fit)
                es, ew, _, _ = _decode(emu, fit)
                assert (es, ew) == (STATUS[r.status], r.why), (n, es, ew, r.status, r.why)
                assert es in (0, 1, 2)
                seen.add(ew)
        assert {"not a WebP", "WebP: truncated chunk", R.E_BITS, ""} <= seen, seen
        st, why, ch, got = _decode(emu, data)
        assert st == 0 and np.array_equal(got[:whole.pixels.size], whole.pixels.ravel())


def test_refusal_statuses_and_texts(emu):
    for name, data, status, text in REFUSALS:
        r = R.decode(data)
        assert (r.status, r.why) == (status, text), name
        es, ew, _, _ = _decode(emu, data)
        assert (es, ew) == (STATUS[status], text), (name, es, ew)
        ps, pw, _ = _parse(emu, data)
        if text in (R.E_BITS, R.E_CODE, R.E_COPY, R.E_CACHE, R.E_TRANSFORM, R.E_GROUPS):  # the stream's, not the header's
            assert ps == 0, name
        else:
            assert (ps, pw) == (STATUS[status], text), name
    assert not R.is_webp(K.SIMPLE_LOSSY) and _parse(emu, K.SIMPLE_LOSSY)[:2] == (2, "not a WebP")
    assert {t for _, _, _, t in REFUSALS} >= {"WebP: animated WebP", "WebP: lossy WebP", "WebP: truncated chunk",
                                             "WebP: bad VP8L signature", "WebP: bad VP8L version", "WebP: no image chunk",
                                             "WebP: VP8X canvas size differs from the VP8L size", R.E_BITS, R.E_CODE,
                                             R.E_COPY, R.E_CACHE, R.E_TRANSFORM, R.E_GROUPS}


DENSE_BYTES = 3000


def test_standalone_program_under_the_sanitizers(tmp_path, refs):
    """Host code with its own main, built with AddressSanitizer and UBSan: the parser and the emulator over
    every case and refusal at every length.  A plain cut is refused by the file's own RIFF size, so the cuts
    that reach the bitstream walk are those with the sizes made to fit: every such length of the two files of
    the truncation test above and of every crafted file and refusal of at most DENSE_BYTES bytes, 64 evenly
    spaced ones of each larger file (the Pillow-made ones: 2 to 40 KB, where every length would take minutes)."""
    exe = str(tmp_path / "vp8l_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DVP8L_MAIN", "-I" + CSRC, "-o", exe] + SRCS, check=True)
    named = _truncation_files(refs)
    dense = named + [d for _, d in CRAFTED if len(d) <= DENSE_BYTES] + [d for _, d, _, _ in REFUSALS if len(d) <= DENSE_BYTES]
    sampled = [d for _, d in PILLOW + CRAFTED if d not in dense] + [d for _, d, _, _ in REFUSALS if d not in dense]
    assert len(dense) >= len(CRAFTED) - 1 + 2 and len(dense) + len(sampled) >= len(PILLOW) + len(CRAFTED) + len(REFUSALS)
    args = []
    for flag, files in (("--dense", dense), ("--sampled", sampled)):
        args.append(flag)
        for data in files:
            args.append(str(tmp_path / ("f%d.webp" % len(args))))
            with open(args[-1], "wb") as f:
                f.write(data)
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    every_length = sum(len(d) + 1 for d in dense + sampled)
    every_fitted = sum(len(d) - R.parse(d)["data_off"] for d in dense if R.decode(d).status != "UNSUPPORTED" and _parses(d))
    assert words[0] == "ok" and int(words[2]) >= every_length + every_fitted, (r.stdout, every_length, every_fitted)
    assert int(words[4]) >= len(PILLOW) + len(CRAFTED) and int(words[6]) > 0 and int(words[8]) > 1000, r.stdout
    assert int(words[10]) >= every_fitted >= sum(len(d) - R.parse(d)["data_off"] for d in named), r.stdout


def _parses(data):
    try:
        R.parse(data)
        return True
    except R.Fail:
        return False


def test_probe_and_sample_align_take_a_lossless_webp():
    from datago_amd import _lib as L
    from datago_amd import synth
    data = dict(PILLOW)["mixed_200x150_m3_q0"]
    st, info = L.probe(data)
    assert st == L.DG_OK and info.format == L.DG_FMT_WEBP == 4
    assert (info.width, info.height, info.components, info.bit_depth) == (200, 150, 3, 8)
    assert info.gpu_supported == 0
    st, info = L.probe(dict(PILLOW)["rgba_130x64"])
    assert st == L.DG_OK and (info.width, info.height, info.components) == (130, 64, 4)
    st, info = L.probe(dict(CRAFTED)["extended_no_alpha"])
    assert st == L.DG_OK and info.format == L.DG_FMT_WEBP and info.components == 3
    st, info = L.probe(data[:40])
    assert st == L.DG_ERR_CORRUPT and info.format == L.DG_FMT_WEBP and "truncated chunk" in L.last_error()
    refused = dict((n, d) for n, d, _, _ in REFUSALS)
    for name in ("animated_flag", "animated_chunks", "extended_lossy", "extended_lossy_alpha"):
        st, info = L.probe(refused[name])  # no VP8L header is reached: the VP8X canvas is the size
        assert st == L.DG_OK and info.format == L.DG_FMT_WEBP and info.gpu_supported == 0, name
        assert (info.width, info.height) == (4, 4) and info.components == (4 if "alpha" in name or "animated" in name else 3), name
    st, info = L.probe(K.SIMPLE_LOSSY)  # a simple lossy file stays an unknown format
    assert st == L.DG_ERR_CORRUPT and "unknown image format" in L.last_error()
    table = L.BucketTable(224, 16, 0.5, 2.0)
    jpg = synth.make_jpeg(5, 64, 48, 85, "4:2:0")
    twin = io.BytesIO()
    data = dict(PILLOW)["rgba_130x64"]  # (not the JPEG's aspect ratio)
    Image.fromarray(np.zeros((64, 130, 4), np.uint8)).save(twin, "PNG")
    got = L.sample_align(table, [data, jpg, jpg])
    assert got == L.sample_align(table, [twin.getvalue(), jpg, jpg])
    assert got[0] == -1 and got[1] == got[2] >= 0
    assert got != L.sample_align(table, [jpg, jpg, jpg])  # (the WebP's 130x64, not the JPEG's 64x48, chose the bucket)
    assert L.sample_align(table, [data[:40], jpg, jpg]) == L.sample_align(table, [b"junk", jpg, jpg])
    # an extended lossy file is the reference payload too (the CPU path loads it): its canvas decides
    lossy = C.riff([C.vp8x(130, 64, 0), C.chunk(b"VP8 ", b"\x30\x01\x00\x9d\x01\x2a\x04\x00\x04\x00")])
    assert L.probe(lossy)[1].width == 130 and L.sample_align(table, [lossy, jpg, jpg]) == got
