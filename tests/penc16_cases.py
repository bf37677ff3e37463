"""Inputs for the 16-bit PNG re-encoder's tests (context option "penc16"): a
label and a uint16 array H x W x spp per case, a few KB each so that the
Python reference (tests/ref_penc16.py) stays fast.  The set is chosen so that
the reference alone shows the properties tests/test_penc16_cpu.py asserts:
every filter type on rows after the first, Sub / Average / None on row 0,
every row alignment, the wave's stride, both byte orders told apart, and the
stream's edges (a 258-long match, matches at and across 1 KiB piece edges,
stream lengths beside 1024 and 2048).

A helper module (no fixtures).
"""
import numpy as np

import ref_penc16

H0, W0 = 12, 23  # the content cases' shape: an odd width, so gray and RGB rows alternate between 4- and 2-byte alignment


def _u16(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int64) & 0xFFFF, dtype=np.uint16)


def noise(h, w, spp, seed):
    return np.random.default_rng(seed).integers(0, 65536, size=(h, w, spp), dtype=np.uint16)


def hramp(h, w, spp, step=300):
    x = np.arange(w)[None, :, None] * step + np.arange(spp)[None, None, :] * 4000 + 1000
    return _u16(np.broadcast_to(x, (h, w, spp)))


def vramp(h, w, spp, step=300):
    y = np.arange(h)[:, None, None] * step + np.arange(spp)[None, None, :] * 4000 + 1000
    return _u16(np.broadcast_to(y, (h, w, spp)))


def plane(h, w, spp):
    yy, xx = np.mgrid[0:h, 0:w]
    return _u16((500 + 290 * xx + 410 * yy)[:, :, None] + np.arange(spp)[None, None, :] * 7000)


def running_average(h, w, spp, seed):
    """Each sample the floor mean of its left and upper neighbours plus small noise: the Average filter's own model."""
    rng = np.random.default_rng(seed)
    a = np.zeros((h + 1, w + 1, spp), np.int64)
    a[0, :, :] = rng.integers(20000, 40000, size=(w + 1, spp))
    a[:, 0, :] = rng.integers(20000, 40000, size=(h + 1, spp))
    for y in range(1, h + 1):
        for x in range(1, w + 1):
            a[y, x] = (a[y, x - 1] + a[y - 1, x]) // 2 + rng.integers(-2, 3, size=spp)
    return _u16(a[1:, 1:])


def flat(h, w, spp, value):
    return np.full((h, w, spp), value, np.uint16)


def content_cases():
    out = []
    for spp in (1, 2, 3, 4):
        out += [(f"noise_s{spp}", noise(H0, W0, spp, 1600 + spp)),
                (f"hramp_s{spp}", hramp(H0, W0, spp)),
                (f"vramp_s{spp}", vramp(H0, W0, spp)),
                (f"plane_s{spp}", plane(H0, W0, spp)),
                (f"runavg_s{spp}", running_average(H0, W0, spp, 1610 + spp)),
                (f"flat_s{spp}", flat(H0, W0, spp, 0x1234 + spp))]
    return out


# row 0 keeps None: 0x0000 / 0x7F7F alternate along the row, so Sub and Paeth pay 127 on every byte where
# None pays it on every other pixel only, and Average pays 127 / 63 in turn; on row 0 Up equals None
ROW0_NONE = "row0_none"


def row0_none():
    px = np.zeros((5, 24, 1), np.uint16)
    px[:, 1::2, 0] = 0x7F7F
    return px


def shape_cases():
    out = []
    for spp in (1, 2, 3, 4):
        out += [(f"1x1_s{spp}", noise(1, 1, spp, 1620 + spp)),
                (f"1x70_s{spp}", noise(1, 70, spp, 1630 + spp)),   # H x W = 1 x 70
                (f"70x1_s{spp}", noise(70, 1, spp, 1640 + spp))]   # 70 rows of one pixel
        out.append((f"w2_s{spp}", noise(7, 2, spp, 1650 + spp)))
    # row bytes beside 64, 128 and 256 (a wave takes 256 row bytes per step; the 8-bit kernel's stride was 64)
    for rb in (62, 64, 66, 126, 128, 130, 254, 256, 258, 510, 514):
        out.append((f"rb{rb}_gray", plane(5, rb // 2, 1) ^ noise(5, rb // 2, 1, rb) >> 12))
    out.append(("rb258_rgb", noise(4, 43, 3, 1661)))   # 43 * 6 = 258
    out.append(("rb256_rgba", noise(4, 32, 4, 1662)))  # 32 * 8 = 256
    out.append(("rb260_la", noise(4, 65, 2, 1663)))    # 65 * 4 = 260
    # odd widths: rows of gray / RGB samples that start 2 bytes off a dword on every other row
    out += [("odd3_gray", noise(9, 3, 1, 1664)), ("odd5_rgb", noise(9, 5, 3, 1665)), ("odd33_gray", plane(6, 33, 1))]
    return out


ALT_LABEL, SPLIT_LABELS, HIT80_LABEL = "alt_00ff_ff00", ("split_ramps_s1", "split_ramps_s2", "split_ramps_s3"), "hit80"


def split_ramps(h, w, spp):
    """High bytes ramp along the row, low bytes down the column (with a per-channel phase)."""
    yy, xx = np.mgrid[0:h, 0:w]
    hi = (xx * 5)[:, :, None] + np.arange(spp)[None, None, :] * 37 + 3
    lo = (yy * 11)[:, :, None] + np.arange(spp)[None, None, :] * 59 + 7
    return _u16(((hi & 0xFF) << 8) | (lo & 0xFF))


def byte_cases():
    alt = np.zeros((8, 21, 2), np.uint16)
    yy, xx = np.mgrid[0:8, 0:21]
    alt[:, :, 0] = np.where((xx + yy) & 1, 0x00FF, 0xFF00)
    alt[:, :, 1] = np.where((xx // 2 + yy) & 1, 0xFF00, 0x00FF)
    hit = np.zeros((6, 19, 1), np.uint16)
    hit[:, 1::2, 0] = 0x8080  # None and Sub both give 0x80 bytes; rows below the first go to Up (zeros)
    hit[3:, :, 0] += 0x0080   # ... and Up gives 0x80 low bytes on row 3
    return [(ALT_LABEL, alt), (HIT80_LABEL, hit)] + [(l, split_ramps(10, 17, int(l[-1]))) for l in SPLIT_LABELS]


# Stream lengths N = H x (2 W spp + 1): a row is odd, so N is a multiple of 1024 only for H a multiple of
# 1024 -- images of megabytes at the widths that matter.  The cases stop beside the edges instead.
STREAM_LENGTHS = {"n1023": (3, 170, 1), "n1025": (1, 512, 1), "n2047": (1, 1023, 1), "n2049": (1, 512, 2)}


def stream_cases():
    out = [("flat_zero_gray", flat(9, 140, 1, 0)),      # the stream is all zeros: 258-long matches, cut at and begun on edges
           ("flat_value_rgba", flat(6, 70, 4, 0xABCD)),  # Sub on row 0, Up below: rows of 560 zeros behind a filter byte
           ("flat_zero_rgb", flat(3, 200, 3, 0))]
    for label, (h, w, spp) in STREAM_LENGTHS.items():
        px = plane(h, w, spp)
        px[:, w // 3:w // 2] = 0x4040  # a flat stretch among the ramp: matches in a stream that is not all matches
        out.append((label, px))
    return out


def all_cases():
    return content_cases() + [(ROW0_NONE, row0_none())] + shape_cases() + byte_cases() + stream_cases()


_refs = {}


def ref(label, px, dynamic=False):
    """ref_penc16.encode(px, dynamic), computed once per label."""
    key = (label, dynamic)
    if key not in _refs:
        _refs[key] = ref_penc16.encode(px, dynamic)
    return _refs[key]
