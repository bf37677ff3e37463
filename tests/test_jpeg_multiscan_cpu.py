"""Non-interleaved baseline JPEGs (context option "jpeg_multiscan") without a
GPU: Pillow (libjpeg-turbo) on the crafted multiscan files of
tests/ref_jpeg_multiscan.py equals the oracle on their single-scan twins byte
for byte (decode_semantics 0's reference); the header parser's allow_multiscan
flag, its refusals and every truncation of a file (also as a stand-alone
program under AddressSanitizer and UBSan); the scan -> parent block map of
dg_types.h against jpeg_craft's MCU order; every scan through the product's
lead_in + decode_range and that map against the oracle's coefficients of the
zeroed twin; dg_probe unchanged."""
import ctypes
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_craft as J
import ref_jpeg_multiscan as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "datago_amd", "csrc")
SO = os.path.join(NATIVE, "libmultiscan.so")
SRCS = [os.path.join(NATIVE, "multiscan.cpp"), os.path.join(CSRC, "host", "jpeg_header.cpp")]

SIZES = [(1, 1), (8, 8), (9, 17), (17, 9), (33, 17), (33, 31), (100, 75)]
RESTARTS = [0, 1, 7]
OLD_WHY = b"non-interleaved multi-scan JPEG"


def _craft(name, w, h, rst=0):
    return R.craft(R.LAYOUTS[name], w, h, seed=w + 3 * h + rst, quality=(50, 90, 100)[rst % 3])


def _variant(rst):
    """Standard tables once / optimal tables once / every scan's own optimal tables under id 0."""
    return {0: dict(tables="std"), 1: dict(tables="optimal"), 7: dict(tables="optimal", per_scan_dht=True)}[rst]


@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_pillow_on_the_multiscan_file_is_the_oracle_on_the_twin(name):
    samp = R.LAYOUTS[name]
    for w, h in SIZES:
        for rst in RESTARTS:
            comps, qtabs = _craft(name, w, h, rst)
            ref = R.decode(comps, samp, w, h, qtabs, 0)
            assert ref.shape == (h, w, 3)
            for script in R.SCRIPTS:
                data = R.multiscan(comps, samp, w, h, qtabs, script, restart=rst, **_variant(rst))
                got = np.asarray(Image.open(io.BytesIO(data)))
                assert np.array_equal(got, ref), (name, w, h, rst, script)
        if (w, h) in ((33, 31), (100, 75)):  # a DRI between the scans, Annex K tables re-sent before every scan
            comps, qtabs = _craft(name, w, h)
            ref = R.decode(comps, samp, w, h, qtabs, 0)
            for script in R.SCRIPTS:
                data = R.multiscan(comps, samp, w, h, qtabs, script, restart=[7, 1, 0][:len(script)], per_scan_dht=True)
                assert data.count(b"\xff\xdd\x00\x04") == len(script)
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), ref), (name, w, h, script)


def test_blocks_outside_the_own_grid_do_not_reach_libjpeg_pixels():
    """The twin's padding blocks may hold anything in decode_semantics 0 (the module docstring's claim)."""
    samp = R.LAYOUTS["420"]
    comps, qtabs = _craft("420", 9, 17)
    with O.semantics(O.SEM_LIBJPEG):
        a = O.jpeg_decode(R.twin(comps, samp, 9, 17, qtabs))[1]
        b = O.jpeg_decode(R.twin(comps, samp, 9, 17, qtabs, zeroed=True))[1]
    assert any(not np.array_equal(c, z) for c, z in zip(comps, R.zero_outside(comps, samp, 9, 17)))
    assert np.array_equal(a, b)


@pytest.fixture(scope="module")
def native():
    deps = SRCS + [os.path.join(CSRC, f) for f in ("dg_types.h", "dg_entropy.h", "host/jpeg_header.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(p) > os.path.getmtime(SO) for p in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"  # build beside it and rename (parallel test workers)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + CSRC, "-o", tmp] + SRCS,
                       check=True)
        os.replace(tmp, SO)
    E = ctypes.CDLL(SO)
    E.ms_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                           ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64), ctypes.c_size_t]
    E.ms_map.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                         ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                         ctypes.POINTER(ctypes.c_uint32)]
    E.ms_map.restype = ctypes.c_int64
    E.ms_div_errors.restype = ctypes.c_int64
    E.ms_emu.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                         ctypes.POINTER(ctypes.c_int16), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                         ctypes.POINTER(ctypes.c_int64)]
    return E


def _parse(E, data, ms=1, h1v2=0, cmyk=0):
    why = ctypes.create_string_buffer(200)
    info = (ctypes.c_int64 * 82)()
    st = E.ms_parse(data, len(data), ms, h1v2, cmyk, why, 200, info, 82)
    scans = [list(info[2 + 10 * j:12 + 10 * j]) for j in range(info[0])] if st == 0 else []
    return st, why.value, (info[1], scans)


def _fnv(bits, vals):
    x = 2166136261
    for b in list(bits) + list(vals):
        x = ((x ^ b) * 16777619) & 0xFFFFFFFF
    return x


def _walk(data):
    """Per scan of a crafted file: (components, restart interval in force, {(class, id): table hash} in force,
    table ids per component, entropy offset) from its marker segments."""
    i, tabs, rst, out = 2, {}, 0, []
    while data[i + 1] != 0xD9:
        m, n = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        s = data[i + 4:i + 2 + n]
        if m == 0xC4:
            while s:
                cnt = sum(s[1:17])
                tabs[(s[0] >> 4, s[0] & 15)] = _fnv(s[1:17], s[17:17 + cnt])
                s = s[17 + cnt:]
        elif m == 0xDD:
            rst = struct.unpack(">H", s)[0]
        i += 2 + n
        if m == 0xDA:
            comps = [(s[1 + 2 * k] - 1, s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15) for k in range(s[0])]
            out.append((comps, rst, dict(tabs), i))
            while not (data[i] == 0xFF and data[i + 1] not in (0, 0xFF) and not 0xD0 <= data[i + 1] <= 0xD7):
                i += 1
            out[-1] += (i,)
    return out


def test_parser_walks_the_scans_with_the_flag(native):
    for name, samp in R.LAYOUTS.items():
        comps, qtabs = _craft(name, 33, 17)
        for script in R.SCRIPTS:
            for kw in (dict(restart=0), dict(restart=3, tables="optimal"),
                       dict(restart=[5, 0, 2][:len(script)], tables="optimal", per_scan_dht=True)):
                data = R.multiscan(comps, samp, 33, 17, qtabs, script, **kw)
                assert _parse(native, data, ms=0)[:2] == (J.UNSUPPORTED, OLD_WHY)
                st, why, (multi, scans) = _parse(native, data)
                assert (st, why, multi, len(scans)) == (J.OK, b"", 1, len(script)), (name, script, why)
                for got, members, (wc, rst, tabs, off, end) in zip(scans, script, _walk(data)):
                    assert [c for c, _, _ in wc] == members
                    assert got[:6] == [len(members), members[0], members[1] if len(members) > 1 else -1, rst, off, end]
                    want = []
                    for q in range(2):
                        want += [tabs[(0, wc[q][1])], tabs[(1, wc[q][2])]] if q < len(members) else [-1, -1]
                    assert got[6:] == want, (name, script, kw)
    # per-scan tables under one id really differ from scan to scan: the snapshots are needed
    st, _, (_, scans) = _parse(native, data)
    assert len({s[6] for s in scans}) > 1 or len({s[7] for s in scans}) > 1


def test_single_scan_and_gray_files_untouched_by_the_flag(native):
    for name in ("444_h2", "mixed_12", "gray_22", "adobe_rgb_420"):
        d = J.layout_jpeg(name, 37, 29)
        assert _parse(native, d, ms=0) == _parse(native, d, ms=1), name
        assert _parse(native, d)[2] == (0, [])


def _small(script, **kw):
    comps, qtabs = _craft("420", 33, 17)
    return R.multiscan(comps, R.LAYOUTS["420"], 33, 17, qtabs, script, **kw)


def test_parser_refusals_with_the_flag(native):
    texts = set()
    for data, status, text in R.refusal_files():
        st, why, _ = _parse(native, data, cmyk=1)
        assert st == status and text in why and why != OLD_WHY, (text, st, why)
        texts.add(why)
        assert _parse(native, data, ms=0, cmyk=1)[:2] == (J.UNSUPPORTED, OLD_WHY), text
    assert len(texts) == 8  # each refusal has a text of its own (the spectral and the frame-header cases share theirs)
    # the four-component file without jpeg_cmyk keeps that option's text
    assert _parse(native, R.refusal_files()[2][0], cmyk=0)[:2] == (J.UNSUPPORTED, b"CMYK/2-component JPEG")
    # a table re-sent unchanged, or one no component uses, between the scans is no refusal
    comps, qtabs = _craft("420", 33, 17)
    same = J._seg(0xDB, bytes([1]) + bytes(int(qtabs[1][z]) for z in J.ZIGZAG))
    unused = J._seg(0xDB, bytes([3]) + bytes([7] * 64))
    assert _parse(native, _small([[0], [1], [2]], extra={1: same, 2: unused}))[:2] == (J.OK, b"")


def test_every_truncation_returns_a_status(native):
    data = _small([[0], [1, 2]], restart=2, tables="optimal", per_scan_dht=True)
    seen = set()
    for cut in range(len(data) + 1):
        for ms in (0, 1):
            st, why, _ = _parse(native, bytes(data[:cut]), ms=ms)
            assert st in (J.OK, J.UNSUPPORTED, J.CORRUPT)
            seen.add((ms, st))
    assert (1, J.OK) in seen and (1, J.CORRUPT) in seen and (0, J.OK) not in seen


def test_standalone_program_under_the_sanitizers(tmp_path):
    """Host code with its own main, built with AddressSanitizer and UBSan: the parser over a file and all its
    truncations, the emulator and the division check."""
    exe = str(tmp_path / "multiscan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DMS_MAIN", "-I" + CSRC, "-o", exe] + SRCS, check=True)
    path = tmp_path / "ms.jpg"
    path.write_bytes(_small([[2], [0], [1]], restart=[3, 0, 1], tables="optimal", per_scan_dht=True))
    refused = []
    for k, (data, _, _) in enumerate(R.refusal_files()):
        refused.append(str(tmp_path / ("refused%d.jpg" % k)))
        with open(refused[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([exe, str(path)] + refused, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 0 and words[6:8] == ["scans", "3"], r.stdout
    assert words[8:10] == ["emu", "0"] and words[12:] == ["mismatch", "0", "div_errors", "0"], r.stdout


def _parent_order(samp, w, h):
    """{(component, by, bx): index in the single-scan file's decode order}, from jpeg_craft's own _mcus."""
    comps = []
    for bh, bw in J.geometry(samp, w, h):
        c = np.zeros((bh, bw, 64), np.int64)
        c[:, :, 0] = np.arange(bh * bw).reshape(bh, bw)
        comps.append(c)
    pos, n = {}, 0
    for mcu in J._mcus(comps, samp):
        for ci, z in mcu:
            bw = comps[ci].shape[1]
            pos[(ci, int(z[0]) // bw, int(z[0]) % bw)] = n
            n += 1
    return comps, pos, n


def test_block_map_is_the_parents_order(native):
    assert native.ms_div_errors() == 0
    for name, samp in R.LAYOUTS.items():
        hs = (ctypes.c_int * 3)(*[s[0] for s in samp])
        vs = (ctypes.c_int * 3)(*[s[1] for s in samp])
        for w, h in SIZES + [(131, 67), (640, 9)]:
            comps, pos, total = _parent_order(samp, w, h)
            grids = R.own_grid(samp, w, h)
            for script in R.SCRIPTS:
                hit = np.zeros(total, np.int64)
                for members in script:
                    out = (ctypes.c_uint32 * total)()
                    ptotal = ctypes.c_uint32()
                    n = native.ms_map(w, h, hs, vs, len(members), (ctypes.c_int * 2)(*(members + [0])[:2]), out, total,
                                      ctypes.byref(ptotal))
                    blocks = R.scan_blocks(comps, samp, w, h, members)
                    assert ptotal.value == total and n == len(blocks), (name, w, h, members)
                    assert list(out[:n]) == [pos[b] for b in blocks], (name, w, h, members)
                    hit[list(out[:n])] += 1
                # together: every block of a component's own grid (one-component scans) or padded grid once
                assert hit.max() == 1
                for c, (gh, gw) in enumerate(grids):
                    alone = [c] in script
                    for (ci, by, bx), p in pos.items():
                        if ci == c:
                            assert hit[p] == (1 if (not alone or (by < gh and bx < gw)) else 0), (name, w, h, script, c)


@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_each_scan_through_the_entropy_emulator(native, name):
    samp = R.LAYOUTS[name]
    cap = 1 << 14
    for k, (w, h) in enumerate([(1, 1), (9, 17), (33, 31), (100, 75), (131, 67)]):
        for rst in (0, 1, 3):
            comps, qtabs = _craft(name, w, h, rst)
            for j, script in enumerate(R.SCRIPTS):
                # zeroed: the blocks this script leaves uncoded; with one scan per component that is every block
                # outside a component's own grid
                st, ref = O.jpeg_coefs(R.twin(comps, samp, w, h, qtabs, zeroed=True if j < 2 else script))
                assert st == 0
                data = R.multiscan(comps, samp, w, h, qtabs, script, restart=rst, **_variant({3: 7}.get(rst, rst)))
                sub_bits, lead = [(128, 0), (256, 96), (1024, 2048), (2048, 4096)][(k + j + rst) % 4]
                out = np.zeros((cap, 64), np.int16)
                nb = ctypes.c_size_t()
                stats = (ctypes.c_int64 * 5)()
                r = native.ms_emu(data, len(data), sub_bits, lead, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
                                  cap, ctypes.byref(nb), stats)
                label = (name, w, h, rst, script, sub_bits)
                assert r == 0 and nb.value == len(ref), label
                assert np.array_equal(out[:nb.value], ref), label
                assert stats[2] == 0 and stats[3] >= stats[4], (label, list(stats))  # (pad bits may start a block more)


def test_probe_describes_the_default_options():
    from datago_amd import _lib as L
    st, info = L.probe(_small([[0], [1], [2]]))
    assert st == L.DG_OK and info.components == 3 and info.gpu_supported == 0
