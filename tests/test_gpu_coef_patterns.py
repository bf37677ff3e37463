"""The sparse coefficient format (k_huff_write stores a block's nonzero
16-byte parts and a part mask, k_idct_t loads the parts the mask names) on
the patterns natural images almost never hold -- all 256 masks, a mask of 0,
lone high parts, blocks shared by three or more entropy ranges, a sparse
block landing where the previous batch left a dense one -- bit-exact against
the oracle in both decode semantics, and identical to dense mode
(`sparse_coef` 0).  The streams are tests/coef_patterns.py's;
test_coef_patterns_cpu.py shows that dropping any stored part changes pixels."""
import numpy as np
import pytest

import coef_patterns as P
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEMS = [0, 1]
SEM_IDS = ["libjpeg", "zune"]
CFG = (224, 16, 0.5, 2.0)


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def files():
    return P.streams()


@pytest.fixture(scope="module")
def refs(files):
    """{(name, sem): the oracle's pixels}, computed once."""
    out = {}
    for sem in SEMS:
        with O.semantics(sem):
            for name, data in files.items():
                st, out[(name, sem)] = O.jpeg_decode(data)
                assert st == 0
    return out


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (kind, decode semantics): "dec" decode-only, "one"
    decode-only with a single slot, "resize" the 224/16 transform."""
    cache = {}

    def get(kind, sem):
        if (kind, sem) not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFG[0], downsampling_ratio=CFG[1],
                      min_aspect_ratio=CFG[2], max_aspect_ratio=CFG[3]) if kind == "resize" else {}
            cache[(kind, sem)] = c = _lib().Context(0, decode_semantics=sem, **kw)
            if kind == "one":
                c.set_option("slots", 1)
        return cache[(kind, sem)]
    yield get
    for c in cache.values():
        c.close()


def _exact(res, names, refs, sem, tag):
    for name, (st, arr, _) in zip(names, res):
        ref = refs[(name, sem)]
        assert st == 0, (tag, name, st)
        assert arr.shape == ref.shape, (tag, name)
        assert np.array_equal(arr, ref), (tag, name, int((arr != ref).sum()))


@pytest.mark.parametrize("sub_bits", [0, 64, 256])
@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_patterns_exact_sparse_and_dense(ctxs, files, refs, sem, sub_bits):
    """Every stream (restart intervals 0 / 1 / 5) in one batch; at sub_bits 64
    a dense block spans three or more ranges (wc_flush forces its mask)."""
    ctx = ctxs("dec", sem)
    names = list(files)
    got = {}
    ctx.set_option("sub_bits", sub_bits)
    try:
        for sparse in (1, 0):
            ctx.set_option("sparse_coef", sparse)
            got[sparse] = ctx.decode_batch([files[n] for n in names])
            _exact(got[sparse], names, refs, sem, ("sparse_coef", sparse))
    finally:
        ctx.set_option("sparse_coef", 1)
        ctx.set_option("sub_bits", 0)
    for name, a, b in zip(names, got[1], got[0]):
        assert np.array_equal(a[1], b[1]), name
    assert ctx.stat("write_mismatch") == 0


@pytest.mark.parametrize("geo", ["", "_420"], ids=["gray", "420"])
@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_sparse_blocks_over_a_stale_arena(ctxs, files, refs, sem, geo):
    """One slot, one image per batch, same geometry: the sparse blocks of
    mask_sweep and the mask-0 blocks of allzero land on the arena bytes where
    the batch before left dense coefficients.  A wrong mask reads those."""
    ctx = ctxs("one", sem)
    for order in (("dense", "mask_sweep", "allzero"), ("dense", "allzero", "mask_sweep")):
        for r in (0, 5):
            for kind in order:
                name = "%s%s_r%d" % (kind, geo, r)
                _exact(ctx.decode_batch([files[name]]), [name], refs, sem, order)
    assert ctx.stat("write_mismatch") == 0


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_restart_patterns_through_the_resize(ctxs, files, refs, sem):
    ctx = ctxs("resize", sem)
    t = B.ARAwareTransform(*CFG)
    names = [n for n in files if not n.endswith("_r0")]
    res = ctx.decode_batch([files[n] for n in names])
    for name, (st, arr, meta) in zip(names, res):
        src = refs[(name, sem)]
        tw, th = t.target_size(src.shape[1], src.shape[0])
        ref = O.crop_and_resize(src, tw, th, O.MODE_FIR)
        assert st == 0 and (meta.width, meta.height) == (tw, th), name
        assert np.array_equal(arr.reshape(ref.shape), ref), (name, int((arr.reshape(ref.shape) != ref).sum()))
