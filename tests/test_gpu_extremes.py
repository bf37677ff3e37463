"""Colour conversion, chroma upsampling and the 8-bit resize at the ends of
the pixel range (tests/extreme_cases.py; test_extremes_cpu.py pins the
references on the same content).  Tolerance 0 against the oracle in both
decode semantics: k_color on every lattice variant and on all 65,536 (Cb, Cr),
(Y, Cb) and (Y, Cr) pairs; the fused fills of the band H kernels (planar and
packed, with and without prefetch, chroma records on and off), of
k_resize_hm, k_resize_hv and k_band_dec on lattice tilings in every ratio
class; the H and V passes and the alpha programs on 0 / 255 checkerboards,
stripes and impulses as PNGs of 1-4 channels and as JPEGs.

Lattice tilings of the resize tests (source -> bucket, H scale, ksize =
2 * ceil(3 * max(scale, 1)) + 1; "crop" files declare 5 columns and 3 rows
less than the MCU grid; in brackets the scaled size when a crop follows):

  512/16 context
    4:4:4  T=2       432 x 432   -> 512 x 512  0.844   7  upscale
           T=2 crop  427 x 429   -> 512 x 512  0.834   7  [512 x 514, top 1]
           T=4       864 x 864   -> 512 x 512  1.688  13  (1.2, 2.5]
           T=4 crop  859 x 861   -> 512 x 512  1.678  13  [512 x 513, top 0.5]
           T=6      1296 x 1296  -> 512 x 512  2.531  17  (2.5, 5]
    4:2:2  T=1       432 x 216   -> 720 x 352  0.600   7  upscale [720 x 360, top 4]
           T=1 crop  427 x 213   -> 720 x 352  0.593   7  [720 x 359, top 3.5]
           T=3      1296 x 648   -> 720 x 352  1.800  13  (1.2, 2.5] [720 x 360, top 4]
           T=3 crop 1291 x 645   -> 720 x 352  1.793  13  [720 x 360, top 4]
           T=5      2160 x 1080  -> 720 x 352  3.000  19  (2.5, 5] [720 x 360, top 4]
    4:2:0  T=1       432 x 432   -> 512 x 512  0.844   7  upscale
           T=1 crop  427 x 429   -> 512 x 512  0.834   7  [512 x 514, top 1]
           T=2       864 x 864   -> 512 x 512  1.688  13  (1.2, 2.5]
           T=2 crop  859 x 861   -> 512 x 512  1.678  13  [512 x 513, top 0.5]
           T=4      1728 x 1728  -> 512 x 512  3.375  23  (2.5, 5]
  224/16 context
    4:4:4  T=6      1296 x 1296  -> 224 x 224  5.786  37  above 5
    4:2:2  T=5      2160 x 1080  -> 304 x 160  6.750  43  above 5 [320 x 160, left 8]
    4:2:0  T=3      1296 x 1296  -> 224 x 224  5.786  37  above 5
           T=6      2592 x 2592  -> 224 x 224 11.571  71  beyond 10
  1024/32 context
    pairs "cbcr"    2048 x 2048  -> 1024 x 1024 2.000 13  the 16-tap planar class

ksize + 1 <= 8, 16, 32 are the band H kernels' tap classes.  A first H pass
whose source segment (127 * scale + 6 * scale + ksize + 18 pixels) exceeds 640
goes to the direct kernel, which is from a scale of about 4.5: the four
224/16 files run the direct H kernel, and the V pass with 37 to 71 taps."""
import numpy as np
import pytest

import extreme_cases as X
import jpeg_craft as J
from datago_amd import synth
from oracle import buckets as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEMS = [0, 1]
SEM_IDS = ["libjpeg", "zune"]
CFGS = {512: (512, 16, 0.5, 2.0), 224: (224, 16, 0.5, 2.0), 1024: (1024, 32, 0.5, 2.0)}
# (sampling, T, crop, ac): the crop files are DC-only (flat blocks of exact lattice values), the others ramp
TILINGS = {
    512: [("444", 2, False, True), ("444", 2, True, False), ("444", 4, False, True), ("444", 4, True, False),
          ("444", 6, False, True),
          ("422", 1, False, True), ("422", 1, True, False), ("422", 3, False, True), ("422", 3, True, False),
          ("422", 5, False, True),
          ("420", 1, False, True), ("420", 1, True, False), ("420", 2, False, True), ("420", 2, True, False),
          ("420", 4, False, True)],
    224: [("444", 6, False, True), ("422", 5, False, True), ("420", 3, False, True), ("420", 6, False, True)],
}
# option, value, default: one at a time against the defaults
OPTIONS = [("h_planar", 0, 1), ("h_prefetch", 0, 1), ("chroma_rec", 0, 1), ("h_mfma", 1, 0), ("hv_fused", 1, 0),
           ("band_dec", 1, 0), ("v_tile", 0, 4), ("v_tile", 2, 4), ("v_tile", 8, 4)]
PNG_OPTIONS = [None, ("h_mfma", 1, 0), ("v_tile", 0, 4)]


def _lib():
    from datago_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (bucket configuration or None, decode semantics, image_to_rgb8), made once per module."""
    cache = {}

    def get(cfg, sem=0, rgb8=False):
        if (cfg, sem, rgb8) not in cache:
            kw = dict(crop_and_resize=True, default_image_size=CFGS[cfg][0], downsampling_ratio=CFGS[cfg][1],
                      min_aspect_ratio=CFGS[cfg][2], max_aspect_ratio=CFGS[cfg][3]) if cfg else {}
            cache[(cfg, sem, rgb8)] = _lib().Context(0, decode_semantics=sem, image_to_rgb8=rgb8, **kw)
        return cache[(cfg, sem, rgb8)]
    yield get
    for c in cache.values():
        c.close()


class _Refs:
    """The oracle's answer per (label, configuration, semantics), computed once."""

    def __init__(self, files):
        self.files = files  # {label: bytes}
        self.cache = {}

    def __call__(self, label, cfg, sem):
        if (label, cfg, sem) not in self.cache:
            with O.semantics(sem):
                st, dec = O.jpeg_decode(self.files[label])
            assert st == 0, label
            if cfg:
                tw, th = B.ARAwareTransform(*CFGS[cfg]).target_size(dec.shape[1], dec.shape[0])
                dec = O.crop_and_resize(dec, tw, th, O.MODE_FIR)
            self.cache[(label, cfg, sem)] = dec
        return self.cache[(label, cfg, sem)]


def _same(label, st, arr, ref):
    """Tolerance 0; the message names the first differing sample."""
    assert st == 0, (label, st, _lib().last_error())
    assert arr.size == ref.size and arr.shape[:2] == ref.shape[:2], (label, arr.shape, ref.shape)
    arr = arr.reshape(ref.shape)
    bad = np.argwhere(arr != ref)
    if bad.size:
        y, x, c = (int(v) for v in bad[0])
        raise AssertionError("%s: %d samples differ, first at (y %d, x %d, c %d): GPU %s, oracle %s"
                             % (label, len(bad), y, x, c, arr[y, x].tolist(), ref[y, x].tolist()))


def _batch(ctx, labels, files, want):
    for label, (st, arr, _) in zip(labels, ctx.decode_batch([files[k] for k in labels])):
        _same(label, st, arr, want(label))


class _option:
    """with _option(ctx, (name, value, default)): ... -- the default comes back on exit."""

    def __init__(self, ctx, opt):
        self.ctx, self.opt = ctx, opt

    def __enter__(self):
        if self.opt:
            self.ctx.set_option(self.opt[0], self.opt[1])

    def __exit__(self, *exc):
        if self.opt:
            self.ctx.set_option(self.opt[0], self.opt[2])
        return False


# ---------------------------------------------------------------- JPEG files
def _tiling_label(s, t, crop, ac):
    return "lattice_%s_T%d%s%s" % (s, t, "_ac" if ac else "", "_crop" if crop else "")


@pytest.fixture(scope="module")
def jpegs():
    """Every crafted JPEG of this module, each built once, with its references."""
    files = {}
    for s, samp in X.SAMPLINGS.items():  # decode only: every lattice variant at T = 1
        for ac in (False, True):
            for crop in (False, True):
                files[_tiling_label(s, 1, crop, ac)] = X.ycc_lattice(samp, 1, ac, crop, seed=7)
    for which in X.PAIR_PLANES:
        files["pairs_" + which] = X.ycc_pairs(which, seed=3)
    for cfg, tilings in TILINGS.items():
        for s, t, crop, ac in tilings:
            label = _tiling_label(s, t, crop, ac)
            if label not in files:
                files[label] = X.ycc_lattice(X.SAMPLINGS[s], t, ac, crop, seed=7 + t)
    return _Refs(files)


DECODE_LABELS = [_tiling_label(s, 1, crop, ac) for s in X.SAMPLINGS for ac in (False, True)
                 for crop in (False, True)] + ["pairs_" + w for w in X.PAIR_PLANES]


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_decode_only_lattices_and_pairs_in_one_batch(ctxs, jpegs, sem):
    ctx = ctxs(None, sem)
    _batch(ctx, DECODE_LABELS, jpegs.files, lambda k: jpegs(k, None, sem))
    assert ctx.stat("write_mismatch") == 0


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
@pytest.mark.parametrize("cfg", [512, 224])
def test_fused_fills_every_ratio_class(ctxs, jpegs, cfg, sem):
    labels = [_tiling_label(*t) for t in TILINGS[cfg]]
    _batch(ctxs(cfg, sem), labels, jpegs.files, lambda k: jpegs(k, cfg, sem))


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_every_chroma_pair_through_the_16_tap_planar_class(ctxs, jpegs, sem):
    _batch(ctxs(1024, sem), ["pairs_cbcr"], jpegs.files, lambda k: jpegs(k, 1024, sem))


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
@pytest.mark.parametrize("opt", OPTIONS, ids=["%s_%d" % o[:2] for o in OPTIONS])
def test_options_on_the_three_smallest_classes(ctxs, jpegs, opt, sem):
    ctx = ctxs(512, sem)
    labels = [_tiling_label(*t) for t in TILINGS[512]]
    before = ctx.stat("band_dec_images")
    with _option(ctx, opt):
        _batch(ctx, labels, jpegs.files, lambda k: jpegs(k, 512, sem))
    if opt[0] == "band_dec":
        assert ctx.stat("band_dec_images") > before  # the fused kernel did take some of them


# ----------------------------------------------------------- contrast images
@pytest.fixture(scope="module")
def pngs():
    """[(label, PNG bytes, the oracle's resize of the source at 224/16)]: the noisy contrast cases."""
    t = B.ARAwareTransform(*CFGS[224])
    out = []
    for label, kind, w, h, ch, sq, seed in X.png_cases():
        src = X.contrast(kind, w, h, ch, sq, seed, noisy=True)
        ref = O.crop_and_resize(src, *t.target_size(w, h), O.MODE_FIR)
        out.append((label, synth.pil_png(src), ref))
    return out


@pytest.mark.parametrize("opt", PNG_OPTIONS, ids=["defaults"] + ["%s_%d" % o[:2] for o in PNG_OPTIONS[1:]])
def test_contrast_pngs_every_channel_count(ctxs, pngs, opt):
    ctx = ctxs(224)
    with _option(ctx, opt):
        res = ctx.decode_batch([d for _, d, _ in pngs])
    for (label, _, ref), (st, arr, meta) in zip(pngs, res):
        assert meta.channels == ref.shape[2], label
        _same(label, st, arr, ref)


def test_contrast_pngs_with_alpha_to_rgb8(ctxs, pngs):
    cases = [p for p in pngs if p[2].shape[2] in (2, 4)]
    res = ctxs(224, 0, True).decode_batch([d for _, d, _ in cases])
    for (label, _, ref), (st, arr, meta) in zip(cases, res):
        assert meta.channels == 3, label
        _same(label, st, arr, O.to_rgb8(ref, True))


@pytest.fixture(scope="module")
def contrast_jpegs():
    return _Refs({label: J.from_pixels(X.contrast(kind, w, h, ch, sq), samp, quality=100)
                  for label, kind, w, h, ch, sq, samp in X.JPEG_CASES})


@pytest.mark.parametrize("sem", SEMS, ids=SEM_IDS)
def test_contrast_through_the_jpeg_path(ctxs, contrast_jpegs, sem):
    labels = [c[0] for c in X.JPEG_CASES]
    _batch(ctxs(512, sem), labels, contrast_jpegs.files, lambda k: contrast_jpegs(k, 512, sem))
