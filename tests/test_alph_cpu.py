"""Lossy WebP with alpha (context option "webp_alpha" beside "webp_lossy") without a GPU.

tests/ref_alph.py, ref_vp8's frame decode plus the ALPH rules, is pinned to Pillow (libwebp,
MODE_RGBA) byte for byte, all four channels, on every accepted file of alph_cases.py; the case
set has to reach every pair of compression and filter and both strip cases of the gradient
walk.  Pillow refuses every file that comes back DG_ERR_CORRUPT; what it does with the two
structural DG_ERR_UNSUPPORTED forms is written down in the cases.  The statements of
datago_amd/csrc/dg_alph.h with the host parser run as tests/native/alph_emu.cpp, a stand-alone
program built with g++ on demand, once plain and once with -fsanitize=address,undefined, and
must equal ref_alph on pixels and on status over every case and its cuts.
"""
import io
import os
import subprocess

import pytest
from PIL import Image

import alph_cases as K
import alph_craft as A
import ref_alph as R
import ref_vp8 as RV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
SRCS = [os.path.join(NATIVE, "alph_emu.cpp"), os.path.join(CSRC, "host", "webp_header.cpp")]
DEPS = SRCS + [os.path.join(NATIVE, f) for f in ("vp8_emu.cpp", "vp8l_emu.cpp")] + \
    [os.path.join(CSRC, f) for f in ("dg_alph.h", "dg_vp8.h", "dg_vp8l.h", "dg_vp8_tables.h", "dg_types.h", "host/webp_header.h")]
STATUS = {"UNSUPPORTED": R.UNSUPPORTED, "CORRUPT": R.CORRUPT}


def build_emu(sanitized):
    exe = os.path.join(NATIVE, "alph_emu_san" if sanitized else "alph_emu")
    if not os.path.exists(exe) or any(os.path.getmtime(p) > os.path.getmtime(exe) for p in DEPS):
        tmp = f"{exe}.{os.getpid()}.tmp"
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", tmp] + flags + SRCS, check=True)
        os.replace(tmp, exe)
    return exe


def pillow(data):
    """(mode, bytes) or None when Pillow refuses the file."""
    try:
        im = Image.open(io.BytesIO(data))
        im.load()
        return im.mode, im.tobytes()
    except Exception:
        return None


def accepted():
    return K.pillow_cases() + K.crafted_cases()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Every case, plain file and refusal as a file, with what ref_alph says about it and what it touched."""
    d = tmp_path_factory.mktemp("alph")
    out = []
    for i, (label, data) in enumerate(accepted() + K.plain_cases() + [(r[0], r[1]) for r in K.refusals()]):
        p = d / ("%03d.webp" % i)
        p.write_bytes(data)
        cover = set()
        out.append((label, data, str(p), R.decode(data, cover), cover))
    return out


def test_ref_equals_pillow_on_every_accepted_case(files):
    n = 0
    for label, data, _, r, _ in files[:len(accepted())]:
        assert (r.status, r.channels) == (R.OK, 4), (label, r.why)
        assert pillow(data) == ("RGBA", r.pixels), label
        n += 1
    assert n >= 110


def test_rgb_is_what_the_vp8_chunk_gives_alone(files):
    """The colour channels are those of the same `VP8 ` chunk under webp_lossy alone (ref_vp8), and a file that is
    not this option's (no ALPH chunk before the image chunk) is ref_vp8's answer whole."""
    for label, data, _, r, _ in files[:len(accepted())]:
        alone = RV.decode(A.without_alph(data))
        assert alone.status == RV.OK and (alone.width, alone.height) == (r.width, r.height), label
        assert bytes(r.pixels[i] for i in range(len(r.pixels)) if i % 4 != 3) == alone.rgb, label
        off = RV.decode(data)  # webp_alpha off: the refusal of today
        assert (off.status, off.why) == (RV.UNSUPPORTED, "WebP: lossy WebP with alpha"), label
    for label, data, _, r, _ in files[len(accepted()):len(accepted()) + len(K.plain_cases())]:
        alone = RV.decode(data)
        assert (r.status, r.why, r.width, r.height, r.channels, r.pixels) == (alone.status, alone.why, alone.width, alone.height, 3, alone.rgb), label
    by = {f[0]: f for f in files}
    # what Pillow does with them is not the pin here: it gives the flag its fourth channel, and refuses an ALPH chunk behind the image
    assert pillow(by["flag_without_chunk"][1])[0] == "RGBA" and pillow(by["alph_after_the_image"][1]) is None
    assert pillow(by["simple_file"][1]) == ("RGB", by["simple_file"][3].pixels)


def test_refusals_have_their_status_and_text(files):
    by = {f[0]: f for f in files}
    texts = set()
    for label, data, status, text, stream, pil in K.refusals():
        r = by[label][3]
        assert (r.status, r.why) == (STATUS[status], text), label
        assert R.parse(data)["status"] == (R.OK if stream else STATUS[status]), label
        got = pillow(data)
        assert (got is None) == (pil == "refuses") and (got is None or got[0] == pil), (label, pil)
        if status == "CORRUPT":
            assert got is None, label  # Pillow refuses what comes back corrupt
        texts.add(text)
        off = RV.decode(data)  # with webp_alpha off every one of them is the refusal of today
        assert (off.status, off.why) == (RV.UNSUPPORTED, "WebP: lossy WebP with alpha"), label
    assert texts == {R.E_HEADER, R.E_RAW, R.E_SHORT_CHUNK, R.E_STREAM, R.E_TWO, R.E_FLAG}
    assert len(texts) == 6  # each case of broken data has a text of its own


def test_case_set_reaches_every_pair_and_both_strip_cases(files):
    cover = set().union(*(f[4] for f in files[:len(accepted())]))
    want = {("alph", c, f) for c in (R.RAW, R.VP8L) for f in range(4)} | {("grad", "first strip"), ("grad", "row above from the plane")}
    assert cover == want, sorted(want ^ cover, key=str)
    for made, label in ((K.pillow_cases(), "pillow"), (K.crafted_cases(), "crafted")):
        own = set().union(*(f[4] for f in files if f[0] in dict(made)))
        assert {c for _, c, _ in (k for k in own if k[0] == "alph")} == {R.RAW, R.VP8L}, label
    # the crafted streams: packed colour indexing with copies, predictor and subtract-green transforms, a cache with hits and copies
    import ref_webp as RW
    seen = {}
    for label, data in K.crafted_cases():
        if label.startswith("vp8l_"):
            rep, h = {}, R.parse(data)
            RW.decode_vp8l(A.alph_of(data)[1:], h["width"], h["height"], rep)
            seen.setdefault(label.split("_")[1], []).append(rep)
    assert any(r["transforms"] == ["index"] and r["index_bits"][0] > 0 and r["copies"] for r in seen["index"])
    assert all(r["transforms"] == ["green", "predictor"] for r in seen["transforms"])
    assert any(r["cache_bits"] == 4 and r["cache_hits"] and r["copies"] for r in seen["cache"])


def test_alpha_stream_cuts_agree_with_pillow():
    """One raw and two VP8L-coded files (one of few levels, which libwebp reads by its own path and rule, one not)
    with their ALPH payload cut short: accept / refuse is Pillow's at every sampled cut, and so are the pixels."""
    cases = dict(accepted())
    kept = refused = 0
    for label in ("noise", "blob_aq50", "blob", "vp8l_index_f3_65x65", "vp8l_transforms_f2_17x33"):
        data = cases[label]
        n = len(A.alph_of(data))
        for k in sorted(set(list(range(1, 13)) + list(range(13, n, max(1, n // 12))) + [n - 1, n])):
            cut = K.cut_stream(data, k)
            r, p = R.decode(cut), pillow(cut)
            assert (r.status == R.OK) == (p is not None), (label, k, r.why)
            if r.status == R.OK:
                assert p == ("RGBA", r.pixels), (label, k)
                kept += 1
            else:
                assert r.status == R.CORRUPT and r.why in (R.E_STREAM, R.E_RAW, R.E_SHORT_CHUNK), (label, k, r.why)
                refused += 1
    assert kept >= 2 and refused >= 80  # a few-levels stream cut by one byte still decodes


def test_option_row_takes_0_and_1_only():
    """The row "webp_alpha" through apply_option on a fresh Options (tests/native/options_main.cpp), held to what
    test_options_cpu.py holds every STRICT row to.  It stands in options.cpp's second table."""
    import test_options_cpu as TO
    exe = TO.build_options_main()
    names = [ln.split("\t")[0] for ln in subprocess.run([exe, "list"], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert "webp_alpha" not in names and "webp" in names  # one row per key across the two tables
    case = TO.strict()
    values = list(case["stored"]) + list(case["rejected"])
    out = subprocess.run([exe, "apply"] + [s for v in values for s in ("webp_alpha", str(v))], check=True, capture_output=True,
                         text=True).stdout.split("\n")[:-1]
    assert len(out) == len(values)
    for v, ln in zip(values, out):
        st, field, same, text = ln.split("\t")
        if v in case["stored"]:
            assert (int(st), field, text) == (0, str(case["stored"][v]), ""), (v, ln)
            assert int(same) == (v == 0), v  # off by default: storing 0 changes nothing, storing 1 does
        else:
            assert int(st) == 1 and int(same) == 1, (v, ln)
            assert text == 'dg_ctx_set_option("webp_alpha", %d): %s' % (v, case["rejected"][v]), (v, ln)


def _emu_decode(exe, files, outdir):
    subprocess.run([exe, "--decode", str(outdir)] + [f[2] for f in files], check=True)
    res = []
    for i in range(len(files)):
        raw = open(os.path.join(str(outdir), "%d.out" % i), "rb").read()
        line, px = raw.split(b"\n", 1)
        st, w, h, c, why = (line.decode().split(" ", 4) + [""])[:5]
        res.append((int(st), int(w), int(h), int(c), why, px))
    return res


def _same(files, results):
    for (label, data, _, r, _), (st, w, h, c, why, px) in zip(files, results):
        assert (st, why) == (r.status, r.why), label
        if r.status == R.OK:
            assert (w, h, c) == (r.width, r.height, r.channels) and px == r.pixels, label


def test_emulation_equals_ref_on_pixels_and_status(files, tmp_path):
    _same(files, _emu_decode(build_emu(False), files, tmp_path))


def test_sanitized_emulation_over_every_case_and_its_cuts(files, tmp_path):
    exe = build_emu(True)
    _same(files, _emu_decode(exe, files, tmp_path))
    run = subprocess.run([exe, "--cuts"] + [f[2] for f in files], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.splitlines()
    assert lines[-1].startswith("ok runs "), lines[-1]
    tot = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert tot["runs"] > 15000 and tot["alph_cuts"] > 6000 and tot["corrupt"] > tot["alph_cuts"]
    # an ALPH cut that still decodes: the same answer from ref_alph, pixels included
    by_path = {f[2]: f for f in files}
    okcuts = [ln.split() for ln in lines if ln.startswith("okcut ")]
    assert okcuts
    cuts = []
    for i, (_, path, k) in enumerate(okcuts[:: max(1, len(okcuts) // 40)]):
        p = tmp_path / ("cut%d.webp" % i)
        p.write_bytes(K.cut_stream(by_path[path][1], int(k)))
        cut = p.read_bytes()
        cuts.append(("%s cut %s" % (by_path[path][0], k), cut, str(p), R.decode(cut), None))
    assert all(c[3].status == R.OK for c in cuts), [c[0] for c in cuts if c[3].status != R.OK]
    out = tmp_path / "cuts"
    out.mkdir()
    _same(cuts, _emu_decode(exe, cuts, out))
