"""Inputs for the PNG re-encoder's match parse (context option "penc_match"):
crafted filtered streams that meet the edges of the rule in ref_penc_match's
docstring, and the patterned images the option is for.

A crafted case states its filtered stream byte by byte.  Its pixels are small
values whose sign (as int8) alternates from pixel to pixel and from row to row,
so that every predictor is farther from a byte than zero is and each row keeps
filter None: the stream is the filter bytes 0 and the pixels.  craft() asserts
that.  On that noise a case copies bytes from earlier ones; `want` / `never`
name tokens (position, length, distance) the reference's parse must / must not
hold, which test_penc_match_cpu.py asserts.

  cases() -> [(label, uint8 H x W x C, want, never)]
  GRAY16: (label, uint16 H x W x 1) for "penc16"
"""
import numpy as np

import ref_penc

_refs = {}
_copied, _pairs = [], []  # of the case being crafted: (start, bytes) of copies; (dst, src) of _far


def _noise(h, w, c, seed):
    """The stream (h rows of 1 + w * c bytes) of sign-alternating noise, as int64 0..255."""
    rng = np.random.default_rng(seed)
    mag = rng.integers(1, 41, (h, w, c))
    sign = np.where((np.arange(h)[:, None, None] + np.arange(w)[None, :, None]) % 2 == 0, 1, -1)
    s = np.zeros((h, w * c + 1), np.int64)
    s[:, 1:] = ((mag * sign) & 0xFF).reshape(h, w * c)
    return s.reshape(-1)


def _copy(s, dst, src, n):
    """n bytes at dst repeat those at src (byte by byte: src + n may pass dst); the next byte does not."""
    for i in range(n):
        s[dst + i] = s[src + i]
    _copied.extend([(dst, n), (src, n)])
    if dst + n < len(s) and s[dst + n] == s[src + n]:
        s[dst + n] += 1 if s[dst + n] < 128 else -1


def _far(s, dst, src, n):
    """_copy for a source that the hash table must still hold when dst looks it up: the noise between them
    is moved off dst's hash (12 bits: on a long way a bucket is seldom left alone)."""
    _copy(s, dst, src, n)
    _pairs.append((dst, src))


def _isolate(s):
    from ref_penc_match import _hash
    fixed = set()
    for a, n in _copied:
        fixed.update(range(a - 3, a + n + 1))
    for dst, src in _pairs:
        r = src + 1
        while r < dst - dst % 64:  # (pieces start on multiples of 64: dst's group starts here)
            if _hash(bytes(s[r:r + 4].astype(np.uint8)), 0) == _hash(bytes(s[dst:dst + 4].astype(np.uint8)), 0):
                assert r not in fixed and s[r] != 0, (dst, src, r)
                s[r] += (1 if s[r] % 128 < 64 else -1) * (1 if s[r] < 128 else -1)  # same sign, another size
            else:
                r += 1


def craft(label, h, w, c, edit, want=(), never=()):
    s = _noise(h, w, c, sum(label.encode()))
    del _copied[:], _pairs[:]
    edit(s)
    _isolate(s)
    rows = s.reshape(h, w * c + 1)
    assert not rows[:, 0].any(), label  # an edit hit a filter byte
    arr = rows[:, 1:].astype(np.uint8).reshape(h, w, c)
    assert np.array_equal(ref_penc.filter_rows(arr)[1].reshape(-1), s), label
    return label, arr, tuple(want), tuple(never)


def _one(label, n, c, edit, want=(), never=()):
    """One row whose stream has at least n bytes."""
    return craft(label, 1, (n + c - 1) // c, c, edit, want, never)


def _tiled(h, w, c, seed, th=4, tw=4):
    t = np.random.default_rng(seed).integers(0, 256, (th, tw, c)).astype(np.uint8)
    return np.tile(t, ((h + th - 1) // th, (w + tw - 1) // tw, 1))[:h, :w]


def _every_symbol(s):
    # C = 4: distances 1, 4, 8 are near ones; the others come from the table, each at the start of a group, the
    # long ones first so that their sources lie inside the window
    for i, d in enumerate((6145, 4097, 3073, 2049, 1537, 1025, 769, 513, 385, 257, 193, 129, 97, 65, 49, 33, 25,
                           17, 13, 9, 5, 3, 2)):
        _far(s, 7168 + 64 * i, 7168 + 64 * i - d, 8)
    for i, d in enumerate((1, 4, 8)):
        _copy(s, 101 + 20 * i, 101 + 20 * i - d, 3)


def _margin(s):
    # C = 4: six bytes of 300.. stand at 492 and, with a seventh, at 500.  At 500 distance 8 gives 6; the table
    # still holds 300 (492 is in 500's own group) and gives 7, which is not 6 + 2
    _copy(s, 492, 300, 6)
    _far(s, 500, 300, 7)


def patterned():
    """The six 128 x 128 inputs of DESIGN.md's size table, and the gray text that the parent codes shorter."""
    from datago_amd import synth
    y, x = np.mgrid[0:128, 0:128]
    chk = (((x + y) & 1) * 255).astype(np.uint8)
    bayer = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]])
    ramp = ((x * 2 + bayer[y & 3, x & 3] * 16) // 256 * 255 + (x * 2) // 64 * 16).clip(0, 255).astype(np.uint8)
    rng = np.random.default_rng(77)
    glyphs = (rng.integers(0, 2, (12, 8, 6)) * 255).astype(np.uint8)
    text = np.full((128, 128), 255, np.uint8)
    for r in range(12):
        for k in range(18):
            text[2 + 10 * r:10 + 10 * r, 2 + 7 * k:8 + 7 * k] = 255 - glyphs[rng.integers(0, 12)]
    rgba = np.dstack([text, text, text, np.full_like(text, 255)])
    return [("checker_gray", chk[:, :, None]), ("checker_rgb", np.repeat(chk[:, :, None], 3, axis=2)),
            ("tile_rgb", _tiled(128, 128, 3, 78, 16, 16)), ("bayer_gray", ramp[:, :, None]), ("text_rgba", rgba),
            ("synth_rgb", synth.synth_pixels(np.random.default_rng(79), 128, 128)), ("text_gray", text[:, :, None])]


def cases():
    out = []
    for c in (1, 2, 3, 4):
        p = 40 * c + 1
        out.append(_one(f"near_C_c{c}", 200, c, lambda s: _copy(s, p, p - c, 3), [(p, 3, c)]))
        out.append(_one(f"near_2C_c{c}", 200, c, lambda s: _copy(s, p, p - 2 * c, 3), [(p, 3, 2 * c)]))
        out.append(_one(f"overlap_c{c}", 300, c, lambda s: _copy(s, p, p - c, 20 * c), [(p, 20 * c, c)]))
    out += [
        _one("d3_inside_group", 200, 1, lambda s: _copy(s, 20, 17, 8), never=[(20, 8, 3)]),
        _one("d3_across_groups", 200, 1, lambda s: _copy(s, 64, 61, 8), [(64, 8, 3)]),
        _one("far_5_refused", 400, 3, lambda s: _far(s, 300, 100, 5), never=[(300, 5, 200)]),
        _one("far_6_taken", 400, 3, lambda s: _far(s, 300, 100, 6), [(300, 6, 200)]),
        _one("far_loses_margin", 700, 4, _margin, [(492, 6, 192), (500, 6, 8)], [(500, 7, 200)]),
        _one("far_before_piece", 1300, 2, lambda s: _far(s, 1100, 900, 10), [(1100, 10, 200)]),
        _one("far_before_window", 8400, 4, lambda s: _copy(s, 8200, 1000, 10), never=[(8200, 10, 7200)]),
        # the longest distance a match of 6 can have: from the window's first byte to the piece's last six
        _one("far_longest", 9300, 4, lambda s: _far(s, 9210, 1024, 6), [(9210, 6, 8186)]),
        _one("far_cut_at_piece_end", 1300, 1, lambda s: _far(s, 1014, 500, 20), [(1014, 10, 514), (1024, 10, 514)]),
        _one("far_258", 900, 3, lambda s: _far(s, 500, 150, 300), [(500, 258, 350), (758, 42, 350)]),
        _one("overlap_period7", 300, 1, lambda s: _copy(s, 37, 30, 163), [(64, 136, 7)]),
        _one("one_distance_symbol", 600, 1, lambda s: _copy(s, 3, 1, 590), [(3, 258, 2)]),
        _one("every_distance_symbol", 8800, 4, _every_symbol),
    ]
    for n, (h, w, c) in ((2, (1, 1, 1)), (3, (1, 1, 2)), (4, (2, 1, 1)), (5, (1, 1, 4)), (1023, (33, 10, 3)),
                         (1024, (32, 31, 1)), (1025, (25, 10, 4)), (2049, (3, 341, 2))):
        out.append((f"stream_{n}", _tiled(h, w, c, n), (), ()))
    out += [(k, a, (), ()) for k, a in patterned()]
    return out


GRAY16 = ("ramp16", (np.arange(96)[None, :] * 517 + np.arange(40)[:, None] * 3).astype(np.uint16)[:, :, None])


def ref(label, arr, dynamic):
    """ref_penc_match.encode(arr, dynamic), kept per (label, dynamic)."""
    import ref_penc_match
    if (label, dynamic) not in _refs:
        _refs[label, dynamic] = ref_penc_match.encode(arr, dynamic)
    return _refs[label, dynamic]
