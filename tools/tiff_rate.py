#!/usr/bin/env python
"""The rate of TIFF files (context option "tiff") beside the paths the same pixels
could take: a pool of 1024x1536 RGB images (a few distinct seeded photo-like
images, repeated) written by Pillow (libtiff: 74 strips of 21 rows) as

    raw        uncompressed (4.7 MB each)
    lzw        LZW
    lzw_pred   LZW with predictor 2
    deflate       Adobe Deflate (option "tiff_deflate")
    deflate_pred  Adobe Deflate with predictor 2
    png        the same pixels as an RGB PNG: the nearest existing GPU path

With --deep, the 16-bit legs instead (option "tiff16"; samples = the pool's 8-bit ones x 257):

    gray16_lzw_pred  16-bit gray, LZW with predictor 2, written by Pillow (strips of 32 rows)
    rgb16_raw        16-bit RGB, uncompressed, MM byte order, one strip (Pillow writes no 16-bit colour, and
                     the tests' LZW writer is too slow for files of this size)
    gray16_png, rgb16_png   the same pixels as 16-bit PNGs (options "png16", "resize16")

With --bilevel, the 1-bit legs instead (option "tiff_bilevel"): 2,480 x 3,508 pages (A4 at 300 dpi) of a seeded
text-like pattern (lines of random 5 x 9 glyphs of 4 x 4-pixel cells), written by Pillow in one strip:

    g4           CCITT Group 4: one strip is one wave's serial walk (k_tiff_g4)
    bilevel_lzw  LZW over the packed rows
    gray_png     the same pixels as an 8-bit gray PNG

Pillow's leg there is gray only (decode, to float, Lanczos resize): it holds no 16-bit colour.

and sent through dg_submit_device, device-resident input and output, by one
context (crop_and_resize to the 512 / 16 buckets).  Per pool: ms per batch with
one batch in flight (median), the pipelined rate with three in flight and the
stages of dg_last_batch_timings.  Beside them, where these files go today:
Pillow decoding and a Lanczos resize to the bucket's size of the same TIFF
files on 16 processes (measured before the GPU is opened; the workers never
touch it).

    python tools/tiff_rate.py [--n 256] [--distinct 2] [--steps 12] [--warmup 3] [--procs 16] [--out r.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bmp_rate import pillow_rate  # noqa: E402  (the same 16-process Pillow leg)

W, H = 1024, 1536
KINDS = ("raw", "lzw", "lzw_pred", "deflate", "deflate_pred", "png")
TIFFS = KINDS[:5]
KINDS16 = ("gray16_lzw_pred", "rgb16_raw", "gray16_png", "rgb16_png")
KINDS1 = ("g4", "bilevel_lzw", "gray_png")
PAGE = (2480, 3508)


def make_pool(distinct: int):
    from PIL import Image
    from datago_amd import synth
    pool = {k: [] for k in KINDS}
    for i in range(distinct):
        im = Image.fromarray(synth.synth_pixels(np.random.default_rng(900 + i), W, H, False))
        for kind, kw in (("raw", dict(format="TIFF", compression="raw")), ("lzw", dict(format="TIFF", compression="tiff_lzw")),
                         ("lzw_pred", dict(format="TIFF", compression="tiff_lzw", tiffinfo={317: 2})),
                         ("deflate", dict(format="TIFF", compression="tiff_adobe_deflate")),
                         ("deflate_pred", dict(format="TIFF", compression="tiff_adobe_deflate", tiffinfo={317: 2})),
                         ("png", dict(format="PNG"))):
            buf = io.BytesIO()
            im.save(buf, **kw)
            pool[kind].append(buf.getvalue())
    return pool


def make_pool16(distinct: int):
    from PIL import Image
    from datago_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tiff16_craft
    pool = {k: [] for k in KINDS16}
    for i in range(distinct):
        px = synth.synth_pixels(np.random.default_rng(900 + i), W, H, False).astype(np.uint16) * 257
        for kind, kw in (("gray16_lzw_pred", dict(format="TIFF", compression="tiff_lzw", tiffinfo={317: 2})), ("gray16_png", dict(format="PNG"))):
            buf = io.BytesIO()
            Image.fromarray(px[:, :, 1]).save(buf, **kw)
            pool[kind].append(buf.getvalue())
        pool["rgb16_raw"].append(tiff16_craft.tiff16("", px, be=True)[1])
        pool["rgb16_png"].append(synth.encode_png16(px, 2, np.random.default_rng(i)))
    return pool


def text_page(seed: int):
    """A page of 0 / 255: lines of random glyphs, words apart, margins around."""
    rng = np.random.default_rng(seed)
    w, h = PAGE[0] // 4, PAGE[1] // 4
    cells = np.ones((h, w), np.uint8)
    n = (w - 80) // 6
    for y in range(40, h - 50, 14):
        g = (rng.random((9, n, 6)) > 0.4).astype(np.uint8)
        g[:, :, 5] = 1
        g[:, rng.random(n) < 0.15] = 1
        cells[y:y + 9, 40:40 + 6 * n] = g.reshape(9, 6 * n)
    return np.kron(cells, np.ones((4, 4), np.uint8))[:PAGE[1], :PAGE[0]] * 255


def make_pool1(distinct: int):
    from PIL import Image
    pool = {k: [] for k in KINDS1}
    for i in range(distinct):
        px = text_page(900 + i)
        for kind, im, kw in (("g4", px, dict(format="TIFF", compression="group4", tiffinfo={278: PAGE[1]})),
                             ("bilevel_lzw", px, dict(format="TIFF", compression="tiff_lzw", tiffinfo={278: PAGE[1]})),
                             ("gray_png", None, dict(format="PNG"))):
            buf = io.BytesIO()
            (Image.fromarray(px) if im is None else Image.fromarray(px).convert("1")).save(buf, **kw)
            pool[kind].append(buf.getvalue())
    return pool


def _pillow16_one(job):
    from PIL import Image
    data, size = job
    return len(Image.open(io.BytesIO(data)).convert("F").resize(size, Image.LANCZOS).tobytes())


def pillow16_rate(files, size, procs: int, passes: int = 3):
    import multiprocessing as mp
    jobs, secs = [(f, size) for f in files], []
    with mp.get_context("fork").Pool(procs) as pool:
        for k in range(passes + 1):  # the first pass warms the workers
            t0 = time.perf_counter()
            pool.map(_pillow16_one, jobs, chunksize=4)
            secs.append(time.perf_counter() - t0)
    return {"procs": procs, "files": len(files), "passes": passes, "images_per_s": round(len(files) / statistics.median(secs[1:]), 1)}


def run(ctx, L, files, steps: int, warmup: int, depth: int = 3):
    offs = np.cumsum([0] + [(len(f) + 15) // 16 * 16 for f in files])[:-1]
    host = ctx.host_alloc(int(offs[-1]) + len(files[-1]) + 64)
    for f, o in zip(files, offs):
        host[int(o):int(o) + len(f)] = np.frombuffer(f, np.uint8)
    d_in = ctx.alloc(host.nbytes + 64)
    ctx.h2d(d_in, host)
    sizes = []
    for f in files:
        st, nb = ctx.output_size(f)
        assert st == L.DG_OK, L.last_error()
        sizes.append(nb)
    d_outs = [ctx.alloc(nb) for nb in sizes]
    ctx.synchronize()
    hp = [host.ctypes.data + int(o) for o in offs]
    dp = [d_in + int(o) for o in offs]
    lens = [len(f) for f in files]

    def once():
        t0 = time.perf_counter()
        ticket, metas = ctx.submit_device(hp, dp, lens, d_outs, sizes)
        ctx.wait(ticket)
        dt = 1e3 * (time.perf_counter() - t0)
        assert all(metas[i].status == L.DG_OK for i in range(len(files))), L.last_error()
        return dt

    ms = [once() for _ in range(warmup + steps)][warmup:]
    t0, tickets = time.perf_counter(), []
    for _ in range(steps):
        tickets.append(ctx.submit_device(hp, dp, lens, d_outs, sizes))
        if len(tickets) >= depth:
            t, metas = tickets.pop(0)  # the library writes the metas until the wait returns: keep them
            ctx.wait(t)
    for t, metas in tickets:
        ctx.wait(t)
    piped = (time.perf_counter() - t0) / steps
    ctx.set_option("timing", 1)
    stages = []
    for _ in range(5):
        once()
        stages.append({k: float(v) for k, v in ctx.timings().items()})
    ctx.set_option("timing", 0)
    for p in d_outs + [d_in]:
        ctx.free(p)
    ctx.host_free(host)
    med = {k: round(statistics.median(s[k] for s in stages), 4) for k in stages[0]}
    return {"coded_mb": round(sum(lens) / 2 ** 20, 2), "ms_per_batch": round(statistics.median(ms), 3),
            "images_per_s_one_in_flight": round(1e3 * len(files) / statistics.median(ms), 1),
            "images_per_s_pipelined": round(len(files) / piped, 1),
            "gpx_s_pipelined": round(len(files) * W * H / piped / 1e9, 3),
            "stages_ms": {k: v for k, v in med.items() if v >= 0.01}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--deep", action="store_true", help="the 16-bit legs (option tiff16) instead")
    ap.add_argument("--bilevel", action="store_true", help="the 1-bit legs (option tiff_bilevel) instead")
    a = ap.parse_args()
    global W, H
    if a.bilevel:
        W, H = PAGE
    kinds, tiffs = (KINDS1, KINDS1[:2]) if a.bilevel else (KINDS16, KINDS16[:2]) if a.deep else (KINDS, TIFFS)
    pool = make_pool1(a.distinct) if a.bilevel else make_pool16(a.distinct) if a.deep else make_pool(a.distinct)
    res = {"images": a.n, "distinct": a.distinct, "size": [W, H], "coded_bytes": {k: len(v[0]) for k, v in pool.items()}}
    from oracle import buckets as B
    size = B.ARAwareTransform(512, 16, 0.5, 2.0).target_size(W, H)
    res["bucket"] = list(size)
    if not a.no_pillow:  # first: forked workers, before this process opens the GPU
        res["pillow"] = {k: (pillow16_rate if a.deep else pillow_rate)([pool[k][i % a.distinct] for i in range(a.n)], size, a.procs)
                         for k in tiffs[:1 if a.deep else None]}
    from datago_amd import _lib as L
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)
    for kind in kinds:
        ctx = L.Context(0, tiff=True, tiff_deflate=True, tiff16=a.deep, png16=a.deep, resize16=a.deep, tiff_bilevel=a.bilevel, **kw)
        res[kind] = run(ctx, L, [pool[kind][i % a.distinct] for i in range(a.n)], a.steps, a.warmup)
        ctx.close()
    r = lambda k: res[k]["images_per_s_pipelined"]  # noqa: E731
    for kind in tiffs:
        res["%s_over_png" % kind] = round(r(kind) / r("gray_png" if a.bilevel else kind[:kind.index("_")] + "_png" if a.deep else "png"), 3)
        if not a.no_pillow and kind in res["pillow"]:
            res["%s_over_pillow" % kind] = round(r(kind) / res["pillow"][kind]["images_per_s"], 2)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
