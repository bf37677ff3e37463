"""Inputs of the "jenc_optimize" tests: enc_cases.jpeg_cases() and the cases
that reach the optimal-table rule's own edges, each with a property over the
REFERENCE's twin (tests/ref_jenc_opt.py), and the references of all of them,
computed once per process.  A plain helper module (NumPy and the oracle, no
GPU, no fixtures).

  cases()          -> [(label, uint8 H x W x C, qualities, property)]
                      property(twin at quality) for every quality of the case
  pairs()          -> [(label, array, quality)]
  std_file(label, arr, quality) -> oracle.jpeg_encode's file
  twin(label, arr, quality)     -> ref_jenc_opt.optimise(std_file)
"""
import numpy as np

import enc_cases as E

QUALITIES = (50, 92, 100)
LIMIT_LABEL = "limit_fibonacci_gray"
NOISE_LABEL = "noise_64x64_q100_rgb"
# counts of the 18 single-coefficient symbols of the limit case: f(n) = f(n-1) + f(n-2) + 1
LIMIT_COUNTS = (1, 1, 3, 5, 9, 15, 25, 41, 67, 109, 177, 287, 465, 753, 1219, 1973, 3193, 5167)


def _used(t):
    return sum(1 for s in t.sizes[:256] if s)


def _single_symbols(tw):
    """Both tables of a gray file hold one symbol, coded as the single bit 0."""
    return all(t.bits[1] == 1 and sum(t.bits) == 1 and len(t.vals) == 1 for t in tw.tables.values()) \
        and len(tw.tables) == 2


def limit_image():
    """1024 x 848 gray for quality 50: 13,510 blocks that hold one AC coefficient each, 18 distinct symbols with
    the counts above, the rest flat; shuffled.  The plain sizes reach 19, so K.3 has work to do (the CPU test
    asserts that, not this comment)."""
    from jpeg_craft import ZIGZAG
    from oracle import oracle as O
    cand = [np.rint(128 + a * E.basis(u, v)) for u in (0, 1) for v in range(1, 8) for a in (6, 12, 24, 48, 96, 120)]
    row = np.concatenate(cand, axis=1).astype(np.uint8)[:, :, None]
    st, co = O.jpeg_coefs(O.jpeg_encode(row, 50), len(cand) + 8)
    assert st == 0 and len(co) == len(cand)
    z = np.asarray(co)[:, ZIGZAG]
    by_symbol = {}
    for blk, zz in zip(cand, z):
        nz = np.flatnonzero(zz[1:]) + 1
        if zz[0] == 0 and len(nz) == 1 and nz[0] - 1 < 16:
            sym = (int(nz[0]) - 1) << 4 | int(abs(int(zz[nz[0]]))).bit_length()
            by_symbol.setdefault(sym, blk)
    syms = sorted(by_symbol)[:len(LIMIT_COUNTS)]
    assert len(syms) == len(LIMIT_COUNTS), len(by_symbol)
    bw, bh = 128, 106
    ids = np.repeat(np.arange(len(syms) + 1), list(LIMIT_COUNTS) + [bw * bh - sum(LIMIT_COUNTS)])
    np.random.default_rng(6100).shuffle(ids)
    blocks = np.stack([by_symbol[s] for s in syms] + [np.full((8, 8), 128.0)]).astype(np.uint8)
    img = blocks[ids].reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
    return np.ascontiguousarray(img)[:, :, None]


def _limit_binds(tw):
    t = tw.tables[(1, 0)]
    return (not tw.fallback and max(t.sizes) == 19 and t.bits[1:] == [1] * 13 + [0, 1, 5]
            and sorted(c for c in tw.hist[(1, 0)] if c)[:-1] == list(LIMIT_COUNTS))


def _dense_noise(tw):
    h = tw.hist[(1, 0)]
    return len(tw.tables) == 4 and 10 * h[0x00] < 64 and all(h[s] for s in range(1, 9)) \
        and sum(h[1:9]) * 10 > 9 * sum(h)


_cases = []


def cases():
    if _cases:
        return _cases
    rng = np.random.default_rng(6000)
    out = [("flat_8x8_gray", np.full((8, 8, 1), 200, np.uint8), QUALITIES, _single_symbols),
           ("block_8x8_rgb", rng.integers(0, 256, (8, 8, 3)).astype(np.uint8), QUALITIES, lambda tw: len(tw.tables) == 4),
           ("partial_13x9_gray", rng.integers(0, 256, (9, 13, 1)).astype(np.uint8), QUALITIES,
            lambda tw: len(tw.tables) == 2),
           ("partial_13x9_rgb", rng.integers(0, 256, (9, 13, 3)).astype(np.uint8), QUALITIES,
            lambda tw: len(tw.tables) == 4)]
    out += [(label, arr, QUALITIES, lambda tw: True) for label, arr, _ in E.jpeg_cases()]
    # uniform noise at quality 100: every divisor is 1 and a coefficient is roughly N(0, 74), so hardly any is
    # zero: blocks end without EOB (the rarest luma AC symbol but for stray runs, far from its 4-bit Annex K
    # code) and the run-0 symbols of categories 1..8 (|c| < 256, 3.5 sigma) carry the scan
    out.append((NOISE_LABEL, E._noise(6001, 64, 64, 3), (100,), _dense_noise))
    out.append((LIMIT_LABEL, limit_image(), (50,), _limit_binds))
    _cases.extend(out)
    return _cases


def pairs():
    return [(label, arr, q) for label, arr, qs, _ in cases() for q in qs]


_std, _twins = {}, {}


def std_file(label, arr, quality):
    key = (label, quality)
    if key not in _std:
        from oracle import oracle as O
        _std[key] = O.jpeg_encode(arr, quality)
    return _std[key]


def twin(label, arr, quality):
    key = (label, quality)
    if key not in _twins:
        import ref_jenc_opt
        _twins[key] = ref_jenc_opt.optimise(std_file(label, arr, quality))
    return _twins[key]
