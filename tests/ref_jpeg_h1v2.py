"""Reference decode of colour JPEGs with an h1v2 component (4:4:0 and its
mixed layouts; context option "jpeg_h1v2"), which the oracle refuses
(supported_sampling), from the crafted coefficient arrays of tests/jpeg_craft.py.

A plain helper module (no tests).  Each component's MCU-padded plane comes
from the oracle itself: the component alone, written as a 1x1 gray JPEG of
cbw*8 x cbh*8 with its own table, decoded in the wanted semantics.  The
upsampling and the colour conversion are restated here in numpy:

  decode_semantics 0 (libjpeg-turbo): h2v1 / h2v2 fancy as the oracle's
    upsample_row; h1v2 as h1v2_fancy_upsample: (3 near + far + bias) >> 2 with
    bias 1 on even rows and 2 on odd rows, far row clamped to the component's
    rows, no box filter for narrow images.  Pinned against Pillow
    (test_jpeg_h1v2_cpu.py).
  decode_semantics 1 (zune-jpeg 0.5.12): as the oracle's upsample_row_zune;
    h1v2 is its vertical half alone, (3 near + far + 2) >> 2, far row clamped
    to the MCU-padded rows.  Recalled from the crate's source, parity-unpinned
    like the rest of that mode.

Also a small progressive (SOF2) writer over the same coefficient arrays.
"""
import struct

import numpy as np

import jpeg_craft as J
from datago_amd.synth import _STD_CHROMA_Q, _STD_LUMA_Q, _BitWriter, _huff_codes, _scaled_q, synth_pixels
from oracle import oracle as O

# the layouts of the tests: 4:4:0 and four mixed ones with an h1v2 component
H1V2_LAYOUTS = {
    "440": [(1, 2), (1, 1), (1, 1)],
    "420_cb_h2v1": [(2, 2), (2, 1), (1, 1)],
    "luma_sub_v2": [(1, 1), (1, 2), (1, 2)],
    "420_cr_h2v1": [(2, 2), (1, 1), (2, 1)],
    "440_cr_full": [(1, 2), (1, 1), (1, 2)],
}


def craft(samp, width, height, seed=0, quality=75):
    """Coefficients of a seeded synthetic image in the factors `samp`:
    (comps, qtabs, tq) as jpeg_craft.from_coefs takes them."""
    px = synth_pixels(np.random.default_rng(seed), width, height)
    qtabs = [_scaled_q(_STD_LUMA_Q, quality), _scaled_q(_STD_CHROMA_Q, quality)]
    tq = [0] + [1] * (len(samp) - 1)
    return J.coefs_from_pixels(px, samp, qtabs, tq), qtabs, tq


def baseline(comps, samp, width, height, qtabs, tq, restart=0, tables="std"):
    return J.from_coefs(comps, samp, width, height, qtabs, restart=restart, tq=tq, tables=tables)


def planes(comps, qtabs, tq, sem):
    """Each component's MCU-padded plane [cbh*8, cbw*8] as the oracle's IDCT of
    semantics `sem` makes it."""
    out = []
    for c, t in zip(comps, tq):
        bh, bw = c.shape[:2]
        data = J.from_coefs([c], [(1, 1)], bw * 8, bh * 8, qtabs, tq=[t])
        with O.semantics(sem):
            st, dec = O.jpeg_decode(data)
        assert st == 0 and dec.shape == (bh * 8, bw * 8, 1)
        out.append(dec[:, :, 0].astype(np.int32))
    return out


def _zune_up_h(row):
    """oracle zune_up_h over every row of `row` [H, n], n >= 2."""
    n = row.shape[1]
    out = np.empty((row.shape[0], 2 * n), np.int32)
    s = 3 * row[:, 1:n - 1] + 2
    out[:, 2:2 * n - 2:2] = (s + row[:, 0:n - 2]) >> 2
    out[:, 3:2 * n - 2:2] = (s + row[:, 2:n]) >> 2
    out[:, 0] = row[:, 0]
    out[:, 1] = (row[:, 0] * 3 + row[:, 1] + 2) >> 2
    out[:, 2 * n - 2] = (3 * row[:, n - 2] + row[:, n - 1] + 2) >> 2
    out[:, 2 * n - 1] = row[:, n - 1]
    return out


def upsample(pl, hr, vr, width, height, dsw, dsh, sem):
    """Component plane -> [height, width] int32 samples at full resolution."""
    ph = pl.shape[0]
    ys, xs = np.arange(height), np.arange(width)
    if vr == 1:
        near = far = pl[ys]
    else:
        r = ys >> 1
        rn = np.where(ys & 1, r + 1, r - 1).clip(0, (ph if sem else dsh) - 1)
        near, far = pl[r], pl[rn]
    if sem:  # zune-jpeg: vertical (3 near + far + 2) >> 2, then upsample_horizontal over the padded row
        row = near if vr == 1 else (3 * near + 2 + far) >> 2
        return (row if hr == 1 else _zune_up_h(row))[:, :width]
    if hr == 1:
        if vr == 1:
            return near[:, :width]
        bias = np.where(ys & 1, 2, 1)[:, None]  # h1v2_fancy_upsample
        return ((3 * near + far + bias) >> 2)[:, :width]
    c = xs >> 1
    if dsw <= 2:  # libjpeg's box filter for the h2 cases
        return near[:, c]
    cn = np.where(xs & 1, c + 1, c - 1).clip(0, dsw - 1)
    if vr == 1:  # h2v1 fancy
        return (3 * near[:, c] + near[:, cn] + np.where(xs & 1, 2, 1)[None, :]) >> 2
    cs = 3 * near + far  # h2v2 fancy
    return (3 * cs[:, c] + cs[:, cn] + np.where(xs & 1, 7, 8)[None, :]) >> 4


def _ycc_to_rgb(y, cb, cr, sem):
    if sem:  # zune-jpeg ycbcr_to_rgb (scalar)
        xb, xr = cb - 128, cr - 128
        rgb = [y + ((45 * xr) >> 5), y - ((11 * xb + 23 * xr) >> 5), y + ((113 * xb) >> 6)]
    else:  # libjpeg jdcolor.c build_ycc_rgb_table, SCALEBITS 16
        f = lambda v: int(v * 65536 + 0.5)
        xb, xr = (cb - 128).astype(np.int64), (cr - 128).astype(np.int64)
        rgb = [y + ((f(1.40200) * xr + 32768) >> 16),
               y + ((-f(0.34414) * xb + 32768 - f(0.71414) * xr) >> 16),
               y + ((f(1.77200) * xb + 32768) >> 16)]
    return np.stack(rgb, axis=2).clip(0, 255).astype(np.uint8)


def decode(comps, samp, width, height, qtabs, tq, sem):
    """HxWx3 uint8 pixels of the (JFIF, YCbCr) file these coefficients make."""
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    up = []
    for pl, (h, v) in zip(planes(comps, qtabs, tq, sem), samp):
        dsw, dsh = -(-width * h // hmax), -(-height * v // vmax)
        up.append(upsample(pl, hmax // h, vmax // v, width, height, dsw, dsh, sem))
    return _ycc_to_rgb(up[0], up[1], up[2], sem)


# ------------------------------------------------------------ progressive


def _dc_symbol(bw, codes, diff):
    s = abs(diff).bit_length()
    bw.put(*codes[s])
    if s:
        bw.put(diff if diff >= 0 else diff + (1 << s) - 1, s)


def _ac_band(bw, codes, z, ss, se):
    """Coefficients ss..se of one block, Al 0, first pass; a single EOB (run 1)
    where the band ends in zeros."""
    k0 = ss - 1
    for k in (np.flatnonzero(z[ss:se + 1]) + ss).tolist():
        run = k - k0 - 1
        while run > 15:
            bw.put(*codes[0xF0])
            run -= 16
        v = int(z[k])
        s = abs(v).bit_length()
        bw.put(*codes[(run << 4) | s])
        bw.put(v if v >= 0 else v + (1 << s) - 1, s)
        k0 = k
    if k0 < se:
        bw.put(*codes[0x00])


def progressive(comps, samp, width, height, qtabs, tq):
    """SOF2 file of the coefficients: an interleaved DC scan with Al 1, an
    interleaved DC refinement, then per component the AC scans 1..5 and 6..63
    (Al 0) over the component's own ceil(cdsw/8) x ceil(cdsh/8) blocks."""
    nc = len(comps)
    comps = [np.asarray(c) for c in comps]
    assert nc == 3 and [c.shape[:2] for c in comps] == J.geometry(samp, width, height)
    tid = [0] + [1] * (nc - 1)  # Huffman table ids (Annex K luminance / chrominance)
    codes = {k: _huff_codes(*v) for k, v in J.std_tables().items()}
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    out = bytearray(b"\xff\xd8")
    out += J._seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in sorted(set(tq)):
        out += J._seg(0xDB, bytes([t]) + bytes(int(qtabs[t][z]) for z in J.ZIGZAG))
    sof = struct.pack(">BHHB", 8, height, width, nc)
    for ci, (h, v) in enumerate(samp):
        sof += bytes([ci + 1, (h << 4) | v, tq[ci]])
    out += J._seg(0xC2, sof)
    for k in sorted(J.std_tables()):
        bits, vals = J.std_tables()[k]
        out += J._seg(0xC4, bytes([(k[0] << 4) | k[1]]) + bytes(bits[1:17]) + bytes(vals))

    def scan(cis, ss, se, ah, al, body):
        nonlocal out
        sos = bytes([len(cis)])
        for ci in cis:
            sos += bytes([ci + 1, (tid[ci] << 4) | tid[ci]])
        bw = _BitWriter()
        body(bw)
        bw.pad()
        out += J._seg(0xDA, sos + bytes([ss, se, (ah << 4) | al])) + bw.out

    def dc_first(bw):
        pred = [0] * nc
        for mcu in J._mcus(comps, samp):
            for ci, z in mcu:
                v = int(z[0]) >> 1  # point transform: arithmetic shift
                _dc_symbol(bw, codes[(0, tid[ci])], v - pred[ci])
                pred[ci] = v

    def dc_refine(bw):
        for mcu in J._mcus(comps, samp):
            for ci, z in mcu:
                bw.put(int(z[0]) & 1, 1)

    scan(range(nc), 0, 0, 0, 1, dc_first)
    scan(range(nc), 0, 0, 1, 0, dc_refine)
    for ci, (h, v) in enumerate(samp):
        nbx, nby = -(-(-(-width * h // hmax)) // 8), -(-(-(-height * v // vmax)) // 8)
        for ss, se in ((1, 5), (6, 63)):
            def ac(bw, ci=ci, ss=ss, se=se, nbx=nbx, nby=nby):
                for by in range(nby):
                    for bx in range(nbx):
                        _ac_band(bw, codes[(1, tid[ci])], comps[ci][by, bx], ss, se)
            scan([ci], ss, se, 0, 0, ac)
    return bytes(out + b"\xff\xd9")


def visible_coefs(comps, samp, width, height):
    """The coefficients a progressive file of `progressive` carries: blocks
    outside a component's own grid have no AC scans (their AC stays zero)."""
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    out = []
    for c, (h, v) in zip(comps, samp):
        c = np.array(c)
        nbx, nby = -(-(-(-width * h // hmax)) // 8), -(-(-(-height * v // vmax)) // 8)
        c[nby:, :, 1:] = 0
        c[:, nbx:, 1:] = 0
        out.append(c)
    return out
