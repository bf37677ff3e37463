"""Reference decode of four-component Adobe JPEGs (APP14 transform 0 = CMYK,
2 = YCCK; context option "jpeg_cmyk"), which the oracle refuses, from the
crafted coefficient arrays of tests/jpeg_craft.py.

A plain helper module (no tests).  The planes, the upsampling and the
YCbCr -> RGB step are those of tests/ref_jpeg_h1v2.py (the oracle's IDCT per
component, numpy restatements of both decode semantics).  On top of them:

  cmyk_planes: H x W x 4 in the stored ("Adobe", inverted) convention -- the
    samples as they are for transform 0; for transform 2 components 0..2 go
    through the semantics' YCbCr -> RGB and c, m, y = 255 - r, g, b, K as it
    is.  In decode_semantics 0 that is what libjpeg-turbo hands back for
    these files (JCS_CMYK; Pillow then inverts: test_jpeg_cmyk_cpu.py pins
    255 - Pillow against it).
  decode: H x W x 3, R, G, B = blinn(c, k), blinn(m, k), blinn(y, k) with
    blinn(a, b) = (t + (t >> 8)) >> 8, t = a b + 128: zune-jpeg's
    color_convert_cymk_to_rgb / color_convert_ycck_to_rgb (stb_image's
    blinn_8x8), recalled from the crate's source and parity-unpinned like the
    rest of that mode.  libjpeg-turbo leaves CMYK alone, so semantics 0 takes
    the same last step on its own planes.

Also a progressive (SOF2) writer for four components in ref_jpeg_h1v2's scan
script.
"""
import struct

import numpy as np

import jpeg_craft as J
import ref_jpeg_h1v2 as R
from datago_amd.synth import _STD_CHROMA_Q, _STD_LUMA_Q, _BitWriter, _huff_codes, _scaled_q, synth_pixels

CMYK_LAYOUTS = {
    "cmyk_444": [(1, 1)] * 4,
    "ycck_420": [(2, 2), (1, 1), (1, 1), (2, 2)],
    "ycck_422": [(2, 1), (1, 1), (1, 1), (2, 1)],
    # K at half the horizontal rate.  (K at a quarter, (2,2) x 3 + (1,1), would be 13 blocks per MCU: T.81's
    # limit is 10 and libjpeg-turbo refuses such a file, as the parser does.)
    "k_sub": [(2, 1), (2, 1), (2, 1), (1, 1)],
    "ycck_440": [(1, 2), (1, 1), (1, 1), (1, 2)],  # needs option "jpeg_h1v2" too
}
TQ = [0, 1, 1, 0]
visible_coefs = R.visible_coefs  # what a file of `progressive` carries (general in the component count)
_ADOBE0 = b"Adobe\x00\x64\x00\x00\x00\x00\x00"  # jpeg_craft's APP14 body: transform 0 at offset 11


def craft(samp, width, height, transform, seed=0, quality=75):
    """Coefficients of a seeded synthetic image in the factors `samp`: the
    three colour components from synth_pixels (YCbCr for transform 2, the
    pixels' channels as C, M, Y samples for transform 0), the K plane from a
    second seed.  Returns (comps, qtabs, tq) as jpeg_craft.from_coefs takes them."""
    assert len(samp) == 4 and transform in (0, 2)
    px = synth_pixels(np.random.default_rng(seed), width, height)
    kpx = synth_pixels(np.random.default_rng(seed + 7919), width, height)
    qtabs = [_scaled_q(_STD_LUMA_Q, quality), _scaled_q(_STD_CHROMA_Q, quality)]
    comps = J.coefs_from_pixels(px, samp, qtabs, TQ, ycc=transform == 2)
    assert len(comps) == 3
    # coefs_from_pixels pairs planes with factors in order: put K's factors first for its one plane
    ksamp = [samp[3]] + list(samp[:3])
    comps += J.coefs_from_pixels(kpx[:, :, 1], ksamp, qtabs, [TQ[3]] + TQ[:3])[:1]
    return comps, qtabs, list(TQ)


def _with_transform(data, transform):
    assert data.count(_ADOBE0) == 1
    return data.replace(_ADOBE0, _ADOBE0[:11] + bytes([transform]))


def baseline(comps, samp, width, height, qtabs, tq, transform, restart=0, tables="std", **kw):
    data = J.from_coefs(comps, samp, width, height, qtabs, restart=restart, tq=tq, tables=tables, header="adobe", **kw)
    return _with_transform(data, transform)


def progressive(comps, samp, width, height, qtabs, tq, transform):
    """SOF2 file of the coefficients with the Adobe header: an interleaved DC
    scan with Al 1, an interleaved DC refinement, then per component the AC
    scans 1..5 and 6..63 (Al 0) over the component's own blocks."""
    nc = len(comps)
    comps = [np.asarray(c) for c in comps]
    assert nc == 4 and [c.shape[:2] for c in comps] == J.geometry(samp, width, height)
    tid = [0] + [1] * (nc - 1)
    codes = {k: _huff_codes(*v) for k, v in J.std_tables().items()}
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    out = bytearray(b"\xff\xd8")
    out += J._seg(0xEE, _ADOBE0[:11] + bytes([transform]))
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
                R._dc_symbol(bw, codes[(0, tid[ci])], v - pred[ci])
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
                        R._ac_band(bw, codes[(1, tid[ci])], comps[ci][by, bx], ss, se)
            scan([ci], ss, se, 0, 0, ac)
    return bytes(out + b"\xff\xd9")


def blinn(a, b):
    """stb_image's blinn_8x8 on integer arrays of 0..255."""
    t = a.astype(np.int64) * b.astype(np.int64) + 128
    return (t + (t >> 8)) >> 8


def cmyk_planes(comps, samp, width, height, qtabs, tq, transform, sem):
    """H x W x 4 uint8 in the stored convention (module docstring)."""
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    up = []
    for pl, (h, v) in zip(R.planes(comps, qtabs, tq, sem), samp):
        dsw, dsh = -(-width * h // hmax), -(-height * v // vmax)
        up.append(R.upsample(pl, hmax // h, vmax // v, width, height, dsw, dsh, sem))
    if transform == 2:
        cmy = 255 - R._ycc_to_rgb(up[0], up[1], up[2], sem).astype(np.int32)
    else:
        cmy = np.stack(up[:3], axis=2)
    return np.concatenate([cmy, up[3][:, :, None]], axis=2).astype(np.uint8)


def rgb_of_planes(cmyk):
    """The RGB image of H x W x 4 planes in the stored convention."""
    k = cmyk[:, :, 3]
    return np.stack([blinn(cmyk[:, :, i], k) for i in range(3)], axis=2).astype(np.uint8)


def decode(comps, samp, width, height, qtabs, tq, transform, sem):
    """H x W x 3 uint8: what the GPU path returns for the file."""
    return rgb_of_planes(cmyk_planes(comps, samp, width, height, qtabs, tq, transform, sem))
