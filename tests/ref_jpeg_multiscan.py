"""Non-interleaved baseline JPEGs (context option "jpeg_multiscan"): SOF0 files
whose scans carry one or two of the frame's three components each, written
from the crafted coefficient arrays of tests/jpeg_craft.py, and the
single-scan twins that hold the same coefficients.

A plain helper module (no tests).  A one-component scan codes the component's
own grid ceil(cdsw / 8) x ceil(cdsh / 8) row by row (T.81 A.2.2), so the
blocks between that grid and the MCU-padded grid of the coefficient arrays
appear in no scan; an interleaved scan codes the frame's MCU grid with the MCU
cut down to its components (A.2.3).

The reference decode of such a file is the oracle's decode of its twin:

  decode_semantics 0 (libjpeg-turbo): the twin as it is.  libjpeg never reads
    a block outside a component's own grid (test_jpeg_multiscan_cpu.py pins
    Pillow on the multiscan file to the oracle on the twin).
  decode_semantics 1 (zune-jpeg): the twin with every block that no scan
    codes zeroed (sample 128): the blocks outside the own grid of every
    component that has a scan to itself.  zune-jpeg keeps zero-initialised
    coefficient storage for multi-scan files and finishes them over the
    MCU-padded grid; its vertical upsampling reads padded rows.  A component
    coded in an interleaved scan has its MCU-padded blocks in the file, and
    that storage keeps what was decoded into it.  Recalled from the crate's
    source, parity-unpinned like the rest of that mode.
"""
import struct

import numpy as np

import jpeg_craft as J
import ref_jpeg_cmyk as RC
import ref_jpeg_h1v2 as RH
from datago_amd.synth import _STD_CHROMA_Q, _STD_LUMA_Q, _BitWriter, _huff_codes, _huff_optimal, _scaled_q, synth_pixels
from oracle import oracle as O

LAYOUTS = {
    "444": [(1, 1)] * 3,
    "422": [(2, 1), (1, 1), (1, 1)],
    "420": [(2, 2), (1, 1), (1, 1)],
    "422_wide": J.LAYOUTS["422_wide"][0],
    "luma_sub_420": J.LAYOUTS["luma_sub_420"][0],
    "mixed_12": J.LAYOUTS["mixed_12"][0],
}
SCRIPTS = [[[0], [1], [2]], [[2], [0], [1]], [[0], [1, 2]], [[0, 1], [2]]]


def craft(samp, width, height, seed=0, quality=75):
    """Coefficients of a seeded synthetic image in the factors `samp`: (comps, qtabs)."""
    px = synth_pixels(np.random.default_rng(seed), width, height)
    qtabs = [_scaled_q(_STD_LUMA_Q, quality), _scaled_q(_STD_CHROMA_Q, quality)]
    return J.coefs_from_pixels(px, samp, qtabs, [0, 1, 1]), qtabs


def own_grid(samp, width, height):
    """[(gh, gw)] per component: the blocks a one-component scan codes."""
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    return [(-(-(-(-height * v // vmax)) // 8), -(-(-(-width * h // hmax)) // 8)) for h, v in samp]


def zero_outside(comps, samp, width, height, script=None):
    """The coefficient arrays with the blocks outside a component's own grid zeroed, for every component
    (script None) or for the components `script` codes in a scan of their own: the blocks it leaves uncoded."""
    out = []
    for k, (c, (gh, gw)) in enumerate(zip(comps, own_grid(samp, width, height))):
        z = np.array(c)
        if script is None or [k] in script:
            z[:] = 0
            z[:gh, :gw] = np.asarray(c)[:gh, :gw]
        out.append(z)
    return out


def scan_blocks(comps, samp, width, height, members):
    """The blocks of one scan in decode order: [(component, by, bx)]."""
    if len(members) == 1:
        c = members[0]
        gh, gw = own_grid(samp, width, height)[c]
        return [(c, by, bx) for by in range(gh) for bx in range(gw)]
    my, mx = comps[0].shape[0] // samp[0][1], comps[0].shape[1] // samp[0][0]
    return [(c, y * samp[c][1] + by, x * samp[c][0] + bx) for y in range(my) for x in range(mx) for c in members
            for by in range(samp[c][1]) for bx in range(samp[c][0])]


def _scan_symbols(comps, samp, width, height, members, restart, ids):
    """(table key, symbol, value, bits) of one scan; restart in the scan's own MCUs."""
    per_mcu = 1 if len(members) == 1 else sum(samp[c][0] * samp[c][1] for c in members)
    seq, pred = [], {c: 0 for c in members}
    for n, (c, by, bx) in enumerate(scan_blocks(comps, samp, width, height, members)):
        if restart and n and n % (restart * per_mcu) == 0:
            seq.append(("rst", (n // (restart * per_mcu) - 1) & 7, 0, 0))
            pred = {k: 0 for k in members}
        z = comps[c][by, bx]
        J._block_symbols(z, pred[c], (0, ids[c]), (1, ids[c]), seq)
        pred[c] = int(z[0])
    return seq


def _specs(seqs, keys, tables):
    if tables == "std":
        return {k: J.std_tables()[(k[0], min(k[1], 1))] for k in keys}
    freq = {k: [0] * 256 for k in keys}
    for seq in seqs:
        for e in seq:
            if e[0] != "rst":
                freq[e[0]][e[1]] += 1
    return {k: _huff_optimal(f[:12] if k[0] == 0 else f) for k, f in freq.items()}


def _dht(specs):
    out = b""
    for k in sorted(specs):
        bits, vals = specs[k]
        out += J._seg(0xC4, bytes([(k[0] << 4) | k[1]]) + bytes(bits[1:17]) + bytes(vals))
    return out


def _entropy(seq, specs):
    codes = {k: _huff_codes(*s) for k, s in specs.items()}
    bw = _BitWriter()
    for key, sym, v, nb in seq:
        if key == "rst":
            bw.pad()
            bw.out += bytes([0xFF, 0xD0 + sym])
            continue
        bw.put(*codes[key][sym])
        if nb:
            bw.put(v if v >= 0 else v + (1 << nb) - 1, nb)
    bw.pad()
    return bytes(bw.out)


def multiscan(comps, samp, width, height, qtabs, script, restart=0, tables="std", per_scan_dht=False, parts=False,
              ss_se=(0, 63), extra=None):
    """SOF0 file with one scan per entry of `script` (lists of component indices).

    restart: one interval for the file, or one per scan (a DRI is then written
    before every scan whose interval differs from the one in force), in the
    scan's own MCUs.  per_scan_dht: every scan's tables -- Annex K ("std") or
    the scan's own optimal ones ("optimal") -- are sent right before its SOS,
    under id 0 for its first component and 1 for its second; otherwise all
    tables come once before the first scan, id 0 for component 0 and 1 for the
    rest.  parts: also return the byte range (start, end) of every scan's entropy data.
    extra: {scan index: bytes} written before that scan's SOS (tests)."""
    comps = [np.asarray(c) for c in comps]
    assert [c.shape[:2] for c in comps] == J.geometry(samp, width, height)
    rst = list(restart) if isinstance(restart, (list, tuple)) else [restart] * len(script)
    tq = [0, 1, 1]
    out = bytearray(b"\xff\xd8")
    out += J._seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in (0, 1):
        out += J._seg(0xDB, bytes([t]) + bytes(int(qtabs[t][z]) for z in J.ZIGZAG))
    sof = struct.pack(">BHHB", 8, height, width, 3)
    for ci, (h, v) in enumerate(samp):
        sof += bytes([ci + 1, (h << 4) | v, tq[ci]])
    out += J._seg(0xC0, sof)
    if per_scan_dht:
        ids = [{c: k for k, c in enumerate(m)} for m in script]
    else:
        ids = [{0: 0, 1: 1, 2: 1}] * len(script)
    seqs = [_scan_symbols(comps, samp, width, height, m, r, i) for m, r, i in zip(script, rst, ids)]
    if not per_scan_dht:
        keys = sorted({e[0] for s in seqs for e in s if e[0] != "rst"} | {(0, 0), (1, 0), (0, 1), (1, 1)})
        shared = _specs(seqs, keys, tables)
        out += _dht(shared)
    in_force, offs = 0, []
    for k, (members, seq) in enumerate(zip(script, seqs)):
        if extra and k in extra:
            out += extra[k]
        if per_scan_dht:
            keys = sorted({(cls, ids[k][c]) for c in members for cls in (0, 1)})
            if tables == "std":  # Annex K luminance for component 0, chrominance for the others, under the scan's ids
                specs = {(cls, ids[k][c]): J.std_tables()[(cls, min(c, 1))] for c in members for cls in (0, 1)}
            else:
                specs = _specs([seq], keys, tables)
            out += _dht(specs)
        else:
            specs = shared
        if rst[k] != in_force:
            out += J._seg(0xDD, struct.pack(">H", rst[k]))
            in_force = rst[k]
        sos = bytes([len(members)])
        for c in members:
            sos += bytes([c + 1, (ids[k][c] << 4) | ids[k][c]])
        out += J._seg(0xDA, sos + bytes([ss_se[0], ss_se[1], 0]))
        ecs = _entropy(seq, specs)
        offs.append((len(out), len(out) + len(ecs)))
        out += ecs
    out += b"\xff\xd9"
    return (bytes(out), offs) if parts else bytes(out)


def twin(comps, samp, width, height, qtabs, zeroed=False, restart=0, tables="std"):
    """The single-scan file of the same coefficients (jpeg_craft.from_coefs);
    zeroed: True = with the blocks outside every component's own grid set to zero, a scan script = with the
    blocks that script leaves uncoded set to zero (zero_outside)."""
    if zeroed:
        comps = zero_outside(comps, samp, width, height, None if zeroed is True else zeroed)
    return J.from_coefs(comps, samp, width, height, qtabs, restart=restart, tq=[0, 1, 1], tables=tables)


def decode(comps, samp, width, height, qtabs, sem, script=None):
    """The reference pixels of a multiscan file of these coefficients written with `script` (module docstring;
    script None: one scan per component)."""
    script = script or [[0], [1], [2]]
    if any((hv[0], hv[1]) == (1, 2) and max(s[1] for s in samp) == 2 and max(s[0] for s in samp) == 1 for hv in samp):
        # 4:4:0 (option "jpeg_h1v2"): the oracle refuses the twin; tests/ref_jpeg_h1v2.py decodes the coefficients
        src = zero_outside(comps, samp, width, height, script) if sem else comps
        return RH.decode(src, samp, width, height, qtabs, [0, 1, 1], sem)
    data = twin(comps, samp, width, height, qtabs, zeroed=script if sem else False)
    with O.semantics(O.SEM_ZUNE if sem else O.SEM_LIBJPEG):
        st, dec = O.jpeg_decode(data)
    assert st == 0, st
    return dec


def refusal_files():
    """(file, status, its text) of every refusal with the flag on."""
    comps, qtabs = craft(LAYOUTS["420"], 33, 17, seed=84)
    small = lambda script, **kw: multiscan(comps, LAYOUTS["420"], 33, 17, qtabs, script, **kw)
    dqt = lambda t, v: J._seg(0xDB, bytes([t]) + bytes([v] * 64))
    cm_samp = RC.CMYK_LAYOUTS["cmyk_444"]
    cm_comps, cm_q, cm_tq = RC.craft(cm_samp, 16, 16, 0, seed=1)
    cmyk = RC.baseline(cm_comps, cm_samp, 16, 16, cm_q, cm_tq, 0)
    sos = cmyk.index(b"\xff\xda")
    n = struct.unpack(">H", cmyk[sos + 2:sos + 4])[0]
    cmyk1 = cmyk[:sos] + b"\xff\xda\x00\x08\x01" + cmyk[sos + 5:sos + 7] + b"\x00\x3f\x00" + cmyk[sos + 2 + n:]
    samp3 = [(3, 1)] * 3
    c3, q3 = craft(samp3, 33, 17, seed=2)
    return [
        (small([[0], [1]]), J.UNSUPPORTED, b"a component that no scan codes"),
        (small([[0], [1], [2]], extra={1: dqt(1, 9)}), J.UNSUPPORTED, b"quantisation table redefined"),
        (cmyk1, J.UNSUPPORTED, b"non-interleaved four-component JPEG"),
        (small([[0], [1], [2], [0]]), J.UNSUPPORTED, b"more scans than components"),
        (multiscan(c3, samp3, 33, 17, q3, [[0], [1], [2]]), J.UNSUPPORTED, b"sampling factor of 3"),
        (small([[0], [0], [1, 2]]), J.CORRUPT, b"component coded twice"),
        (small([[0], [1, 2]], ss_se=(0, 62)), J.CORRUPT, b"spectral selection or successive approximation"),
        (small([[0], [1, 2]], ss_se=(1, 63)), J.CORRUPT, b"spectral selection or successive approximation"),
    ] + [(d, J.CORRUPT, b"frame header after a scan") for d in second_frame_files()]


def second_frame_files():
    """Files that send another frame header once scans have been read: after three one-component scans of a
    three-component SOF0 frame, (a) an Adobe segment, a four-component SOF2 frame and an interleaved DC scan,
    (b) an Adobe segment and a four-component SOF0 frame, (c) after the first scan, a three-component SOF2
    frame with other factors.  The walk must not let them swap the components under the recorded scans."""
    comps, qtabs = craft(LAYOUTS["420"], 33, 17, seed=84)
    adobe = J._seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00")

    def sof(marker, factors):
        body = struct.pack(">BHHB", 8, 17, 33, len(factors))
        for ci, (h, v) in enumerate(factors):
            body += bytes([ci + 1, (h << 4) | v, min(ci, 1)])
        return J._seg(marker, body)
    dc_scan = J._seg(0xDA, bytes([4, 1, 0x00, 2, 0x10, 3, 0x10, 4, 0x10, 0, 0, 0])) + b"\x00" * 8
    one = multiscan(comps, LAYOUTS["420"], 33, 17, qtabs, [[0], [1], [2]])[:-2]
    return [one + adobe + sof(0xC2, [(1, 1)] * 4) + dc_scan + b"\xff\xd9",
            one + adobe + sof(0xC0, [(1, 1)] * 4) + b"\xff\xd9",
            multiscan(comps, LAYOUTS["420"], 33, 17, qtabs, [[0], [1], [2]], extra={1: sof(0xC2, [(1, 1)] * 3)})]
