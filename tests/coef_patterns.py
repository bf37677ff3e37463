"""Coefficient patterns the sparse coefficient format has to get right, as
JPEGs built from chosen quantised coefficients (tests/jpeg_craft.py).

k_huff_write stores a block as the nonzero ones of its eight 16-byte parts
(part p = zigzag coefficients 8p .. 8p + 7) plus a mask of the parts stored;
k_idct_t reads the parts the mask names and takes the rest as zero.  Natural
images almost never produce a mask of 0, a lone high part, or all 256 masks;
these streams do.  A plain helper module shared by the CPU tests
(test_coef_patterns_cpu.py, test_entropy_emulator.py) and the GPU tests
(test_gpu_coef_patterns.py).

Geometries: "gray" = one component, 16 x 16 blocks (128 x 128 pixels);
"420" = (2,2),(1,1),(1,1) with 8 x 8 MCUs (128 x 128 pixels: 256 luma blocks
and 64 blocks in each chroma plane).
"""
import numpy as np

import jpeg_craft as J

GEOS = {"gray": [(1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}
W = H = 128
Q_SWEEP, Q_DENSE = 16, 4  # mask_sweep at q < 4 has parts whose removal changes no pixel: keep q >= 4


def sweep_masks(geo, seed=11):
    """Per component, the part mask of every block [bh, bw]: all 256 masks in
    a seeded random order on the first component; on the two chroma planes
    of "420" a seeded random 128 of them."""
    rng = np.random.default_rng(seed)
    luma = rng.permutation(256).reshape(16, 16)
    if geo == "gray":
        return [luma]
    chroma = rng.permutation(256)[:128]
    return [luma, chroma[:64].reshape(8, 8), chroma[64:].reshape(8, 8)]


def sweep_coefs(geo, seed=11, drop_part=None):
    """mask_sweep coefficients: each part named by a block's mask holds one
    or two coefficients with 1 <= |v| <= 3 at random positions of the part,
    every other coefficient is 0 (mask bit 0 clear: DC 0).  drop_part: that
    part zeroed in every block (for the sensitivity check)."""
    rng = np.random.default_rng(seed + 1)
    out = []
    for masks in sweep_masks(geo, seed):
        bh, bw = masks.shape
        z = np.zeros((bh, bw, 64), np.int64)
        for by in range(bh):
            for bx in range(bw):
                for p in range(8):
                    if not (masks[by, bx] >> p) & 1:
                        continue
                    pos = rng.choice(8, size=int(rng.integers(1, 3)), replace=False)
                    z[by, bx, 8 * p + pos] = rng.integers(1, 4, len(pos)) * rng.choice([-1, 1], len(pos))
        if drop_part is not None:
            z[:, :, 8 * drop_part:8 * drop_part + 8] = 0
        out.append(z)
    return out


def dense_coefs(geo, seed=12):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 3, (bh, bw, 64)) * rng.choice([-1, 1], (bh, bw, 64))
            for bh, bw in J.geometry(GEOS[geo], W, H)]


def zero_coefs(geo):
    return [np.zeros((bh, bw, 64), np.int64) for bh, bw in J.geometry(GEOS[geo], W, H)]


def eob_coefs(seed=13):
    """Gray, 8 x 8 blocks: block k's last nonzero coefficient is zigzag k.
    From k = 18 on the block is z[1], then a run of k - 2 >= 16 zeros (one to
    three ZRL symbols), then z[k]; below, random small coefficients."""
    rng = np.random.default_rng(seed)
    z = np.zeros((64, 64), np.int64)
    for k in range(64):
        if k >= 18:
            z[k, 1] = int(rng.integers(1, 4))
        else:
            z[k, :k] = rng.integers(-3, 4, k)
        z[k, k] = int(rng.choice([-3, -2, -1, 1, 2, 3]))
    return [z.reshape(8, 8, 64)]


def interleaved_coefs():
    """Gray: block rows of dense, all-zero and mask_sweep blocks in turn."""
    d, s = dense_coefs("gray")[0], sweep_coefs("gray")[0]
    z = np.zeros_like(d)
    z[0::3], z[2::3] = d[0::3], s[2::3]
    return [z]


def build(comps, geo, q, restart=0, tables="std"):
    n = len(GEOS[geo])
    h, w = (comps[0].shape[0] * 8, comps[0].shape[1] * 8) if n == 1 else (H, W)
    return J.from_coefs(comps, GEOS[geo], w, h, [np.full(64, q)] * 2, restart=restart, tables=tables)


def streams(restarts=(0, 1, 5)):
    """{name: bytes} of every pattern: mask_sweep, dense and allzero in both
    geometries and eob_sweep at each restart interval, and the interleaved
    image at restart interval 5."""
    out = {}
    for r in restarts:
        for geo in GEOS:
            sfx = ("" if geo == "gray" else "_420") + "_r%d" % r
            out["mask_sweep" + sfx] = build(sweep_coefs(geo), geo, Q_SWEEP, r)
            out["dense" + sfx] = build(dense_coefs(geo), geo, Q_DENSE, r, tables="optimal" if r == 1 else "std")
            out["allzero" + sfx] = build(zero_coefs(geo), geo, Q_SWEEP, r)
        out["eob_sweep_r%d" % r] = build(eob_coefs(), "gray", Q_SWEEP, r)
    out["interleaved_r5"] = build(interleaved_coefs(), "gray", Q_SWEEP, 5)
    return out
