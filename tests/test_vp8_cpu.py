"""Lossy WebP (context option "webp_lossy") without a GPU.

tests/ref_vp8.py, the plain restatement of the container rules and the VP8 key-frame
decode, is pinned to Pillow (libwebp) byte for byte on every accepted file of
vp8_cases.py, and the case set has to reach every mode by position, token, band,
context, filter kind and hev threshold that ref_vp8 records.  The walk of
datago_amd/csrc/dg_vp8.h with the host parser runs as tests/native/vp8_emu.cpp, a
stand-alone program built with g++ on demand, and must equal ref_vp8 on pixels and
on status; built with -fsanitize=address,undefined it runs every case and its
truncations.
"""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import ref_vp8 as R
import vp8_cases as K
import vp8_craft as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
SRCS = [os.path.join(NATIVE, "vp8_emu.cpp"), os.path.join(CSRC, "host", "webp_header.cpp")]
DEPS = SRCS + [os.path.join(CSRC, f) for f in ("dg_vp8.h", "dg_vp8_tables.h", "dg_types.h", "host/webp_header.h")]
STATUS = {"UNSUPPORTED": R.UNSUPPORTED, "CORRUPT": R.CORRUPT}


def build_emu(sanitized):
    exe = os.path.join(NATIVE, "vp8_emu_san" if sanitized else "vp8_emu")
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


def _pillow_agrees(cut, rgb):
    """Pillow's pixels for an accepted cut.  The one known difference ("Lossy WebP"): a last chunk of odd
    length without its pad byte, which libwebp's demuxer refuses and the walker here takes, as parse_webp_header does."""
    p = pillow(cut)
    if p is None:
        h = R.parse(cut)
        return h["len"] & 1 == 1 and h["off"] + h["len"] == len(cut)
    return p == ("RGB", rgb)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Every case and refusal as a file, with what ref_vp8 says about it and what it touched."""
    d = tmp_path_factory.mktemp("vp8")
    out = []
    cases = K.pillow_cases() + K.crafted_cases() + [(r[0], r[1]) for r in K.refusals()] + [("lossless", K.lossless_file())]
    for i, (label, data) in enumerate(cases):
        p = d / ("%03d.webp" % i)
        p.write_bytes(data)
        cover = set()
        out.append((label, data, str(p), R.decode(data, cover), cover))
    return out


def test_ref_equals_pillow_on_every_accepted_case(files):
    n = 0
    for label, data, _, r, _ in files[:len(K.pillow_cases()) + len(K.crafted_cases())]:
        assert r.status == R.OK, (label, r.why)
        assert pillow(data) == ("RGB", r.rgb), label
        n += 1
    assert n >= 110


def test_refusals_have_their_status_and_text(files):
    by = {f[0]: f for f in files}
    for label, data, status, text, stream in K.refusals():
        r = by[label][3]
        assert (r.status, r.why) == (STATUS[status], text), label
        assert R.parse(data)["status"] == (R.OK if stream else STATUS[status]), label
        if label != "alpha":  # Pillow decodes the alpha plane, which is the follow-up here
            assert pillow(data) is None, label
    assert R.decode(K.lossless_file()) == R.Result(R.CORRUPT, "", 0, 0, None)  # not the lossy path's file
    assert not R.parse(b"RIFF\x04\0\0\0WEBP")["claim"]


def test_case_set_reaches_everything(files):
    cover = set().union(*(f[4] for f in files))
    assert not (R.universe() - cover), sorted(R.universe() - cover, key=str)
    crafted = set().union(*(f[4] for f in files if f[0] in dict(K.crafted_cases())))
    for key in (("filter", "simple"), ("parts", 8), ("hdr", "sharp"), ("hdr", "lfdelta"), ("hdr", "segnomap"), ("token", "cat6")):
        assert key in crafted, key


def test_what_pillow_never_writes():
    """The reason for vp8_craft: one partition, the normal filter, sharpness 0, no deltas, version 0."""
    rng = np.random.default_rng(4)
    a = K._photo(rng, 40, 56)
    maps = set()
    for q in range(0, 101):
        for m in (0, 4, 6):
            i = C.frame_info(K.save(a, q, m))
            assert (i["parts"], i["simple"], i["sharp"], i["lf_delta"], i["version"]) == (1, 0, 0, 0, 0), (q, m)
            assert i["seg"] == i["seg_map"] == (0 if q == 100 else 1), (q, m)
            maps.add(i["seg_map"])
    assert maps == {0, 1}
    assert C.frame_info(K.save(a[:1, :1], 75, 4))["seg"] == 0  # a tiny image


def test_bool_encoder_round_trips():
    rng = np.random.default_rng(5)
    seq = [(int(rng.integers(0, 2)), int(rng.integers(1, 256))) for _ in range(4000)]
    e = C.BoolEnc()
    for bit, p in seq:
        e.put(bit, p)
    data = e.finish()
    d = R.BoolDec(data, 0, len(data))
    assert [d.bit(p) for _, p in seq] == [b for b, _ in seq] and not d.eof


def test_option_row_takes_0_and_1_only():
    """The row "webp_lossy" through apply_option on a fresh Options (tests/native/options_main.cpp), held to what
    test_options_cpu.py holds every STRICT row to.  It stands in options.cpp's second table, which find_option
    reads after the first."""
    import test_options_cpu as TO
    exe = TO.build_options_main()
    names = [ln.split("\t")[0] for ln in subprocess.run([exe, "list"], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert "webp_lossy" not in names and "webp" in names  # one row per key across the two tables
    case = TO.strict()
    values = list(case["stored"]) + list(case["rejected"])
    out = subprocess.run([exe, "apply"] + [s for v in values for s in ("webp_lossy", str(v))], check=True, capture_output=True,
                         text=True).stdout.split("\n")[:-1]
    assert len(out) == len(values)
    for v, ln in zip(values, out):
        st, field, same, text = ln.split("\t")
        if v in case["stored"]:
            assert (int(st), field, text) == (0, str(case["stored"][v]), ""), (v, ln)
            assert int(same) == (v == 0), v  # off by default: storing 0 changes nothing, storing 1 does
        else:
            assert int(st) == 1 and int(same) == 1, (v, ln)
            assert text == 'dg_ctx_set_option("webp_lossy", %d): %s' % (v, case["rejected"][v]), (v, ln)


def _emu_decode(exe, files, outdir):
    subprocess.run([exe, "--decode", str(outdir)] + [f[2] for f in files], check=True)
    res = []
    for i in range(len(files)):
        raw = open(os.path.join(str(outdir), "%d.out" % i), "rb").read()
        line, px = raw.split(b"\n", 1)
        st, w, h, why = (line.decode().split(" ", 3) + [""])[:4]
        res.append((int(st), int(w), int(h), why, px))
    return res


def test_emulation_equals_ref_on_pixels_and_status(files, tmp_path):
    for (label, data, _, r, _), (st, w, h, why, px) in zip(files, _emu_decode(build_emu(False), files, tmp_path)):
        assert (st, why) == (r.status, r.why), label
        if r.status == R.OK:
            assert (w, h) == (r.width, r.height) and px == r.rgb, label


def test_sanitized_emulation_over_every_case_and_its_truncations(files, tmp_path):
    exe = build_emu(True)
    for (label, data, _, r, _), (st, w, h, why, px) in zip(files, _emu_decode(exe, files, tmp_path)):
        assert (st, why) == (r.status, r.why) and (r.status != R.OK or px == r.rgb), label
    dense = [f[2] for f in files if len(f[1]) <= 3000]
    sampled = [f[2] for f in files if len(f[1]) > 3000]
    assert dense and sampled
    run = subprocess.run([exe, "--cuts", "--dense"] + dense + ["--sampled"] + sampled, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.splitlines()
    assert lines[-1].startswith("ok runs "), lines[-1]
    tot = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert tot["runs"] > 30000 and tot["fitted"] > 10000 and tot["corrupt"] > tot["fitted"]
    # a cut that still decodes lost only bytes no reader needed: ref_vp8 and Pillow give the whole file's pixels
    by_path = {f[2]: f for f in files}
    okcuts = [ln.split() for ln in lines if ln.startswith("okcut ")]
    for _, path, n, fit in okcuts[:: max(1, len(okcuts) // 40)]:
        label, data, _, r, _ = by_path[path]
        cut = K.fitted_cut(data, int(n)) if fit == "1" else data[:int(n)]
        rc = R.decode(cut)
        assert rc.status == R.OK and rc.rgb == r.rgb, (label, n, fit)
        assert _pillow_agrees(cut, r.rgb), (label, n, fit)


def test_a_cut_stream_is_pillows_answer_or_corrupt(files):
    """ref_vp8 on 24 fitted cuts of a Pillow-made and a crafted file: never anything but Pillow's pixels or CORRUPT."""
    corrupt = 0
    for label in ("photo_40x36", "parts4_20x77", "bpred_mixed"):
        data = dict(K.pillow_cases() + K.crafted_cases())[label]
        off = R.parse(data)["off"]
        for k in range(24):
            n = off + 10 + 1 + k * (len(data) - off - 12) // 23
            cut = K.fitted_cut(data, n)
            r = R.decode(cut)
            if r.status == R.OK:
                assert _pillow_agrees(cut, r.rgb), (label, n)
            else:
                assert r.status == R.CORRUPT and r.why in (R.FAIL_BITS, R.FAIL_PARTS), (label, n, r.why)
                corrupt += 1
    assert corrupt >= 60
