#!/usr/bin/env python
"""The rate of lossy WebP files (context option "webp_lossy") beside where they go
today: a pool of 256 images 1024x1536 (a few distinct seeded images, half
photo-like, half screenshot-like, repeated) written by Pillow's WebP writer at
quality 75, method 4, and sent through dg_submit_device, device-resident input and
output, by one context (crop_and_resize to the 512 / 16 buckets).  Reported: ms per
batch with one batch in flight (median), the pipelined rate with three in flight
and the stages of dg_last_batch_timings (option "timing": k_vp8_parse, k_vp8_recon
and k_vp8_filter run in the png_inflate span, k_vp8_rgb in png_unfilter).  Beside
them: Pillow decoding and a Lanczos resize to the bucket's size of the same files
on 16 processes (measured before the GPU is opened; the workers never touch it).
--no-pillow leaves that out (a run under a kernel trace, for the per-kernel spans);
--scaling adds batches of 1, 16 and 64 images.

    python tools/webp_lossy_rate.py [--n 256] [--distinct 4] [--steps 6] [--warmup 2] [--procs 16] [--scaling] [--no-pillow] [--out r.json]
"""
import argparse
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import webp_rate as WR  # noqa: E402  (the pool's images, the Pillow pool and the timed loop are its)

W, H = WR.W, WR.H


def make_pool(distinct: int):
    from PIL import Image
    from datago_amd import synth
    files = []
    for i in range(distinct):
        rng = np.random.default_rng(900 + i)
        rgb = WR.screenshot(rng) if i % 2 else synth.synth_pixels(rng, W, H, False)
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="WEBP", quality=75, method=4)
        files.append(buf.getvalue())
    return files


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--scaling", action="store_true", help="also time batches of 1, 16 and 64 images")
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pool = make_pool(a.distinct)
    res = {"images": a.n, "distinct": len(pool), "size": [W, H], "quality": 75, "method": 4, "coded_bytes": [len(f) for f in pool]}
    files = [pool[i % len(pool)] for i in range(a.n)]
    from oracle import buckets as B
    size = B.ARAwareTransform(512, 16, 0.5, 2.0).target_size(W, H)
    res["bucket"] = list(size)
    if not a.no_pillow:  # first: forked workers, before this process opens the GPU
        res["pillow"] = WR.pillow_rate(files, size, a.procs)
        print(json.dumps(res["pillow"]), flush=True)
    from datago_amd import _lib as L
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5, max_aspect_ratio=2.0)
    ctx = L.Context(0, webp_lossy=True, **kw)
    res["webp_lossy"] = WR.run(ctx, L, files, a.steps, a.warmup)
    print(json.dumps(res["webp_lossy"]), flush=True)
    if a.scaling:
        res["scaling"] = {str(n): WR.run(ctx, L, files[:n], 3, 1) for n in (1, 16, 64)}
    ctx.close()
    if not a.no_pillow:
        res["webp_lossy_over_pillow"] = round(res["webp_lossy"]["images_per_s_pipelined"] / res["pillow"]["images_per_s"], 2)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
