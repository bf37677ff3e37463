#!/usr/bin/env python
"""The rate of lossless WebP files (context option "webp") beside the two paths the
same pixels could take: a pool of 256 images 1024x1536 (a few distinct seeded
images, half photo-like, half screenshot-like: flat panels, rectangles and text,
repeated) written as

    webp     Pillow's WebP writer (lossless=True, exact=True, method 4, quality 75)
    png      the same pixels as an RGB PNG: the nearest existing GPU path

and sent through dg_submit_device, device-resident input and output, by one
context (crop_and_resize to the 512 / 16 buckets).  Per pool: ms per batch with
one batch in flight (median), the pipelined rate with three in flight, and the
stages of dg_last_batch_timings (option "timing"; k_vp8l_decode + k_vp8l_inverse
run in the png_inflate span, k_vp8l_store in png_unfilter).  Beside them, where
these files go today: Pillow decoding and a Lanczos resize to the bucket's size
of the same WebP files on 16 processes (measured before the GPU is opened; the
workers never touch it).

    python tools/webp_rate.py [--n 256] [--distinct 4] [--steps 6] [--warmup 2] [--pool pool.npz] [--procs 16] [--out r.json]

--pool caches the files.  --prepare writes the cache and stops (no GPU needed)."""
import argparse
import io
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1024, 1536
KINDS = ("webp", "png")


def screenshot(rng):
    from PIL import Image, ImageDraw
    im = Image.new("RGB", (W, H), (245, 245, 245))
    d = ImageDraw.Draw(im)
    for _ in range(200):
        x0, y0 = int(rng.integers(0, W - 100)), int(rng.integers(0, H - 60))
        d.rectangle([x0, y0, x0 + int(rng.integers(20, 300)), y0 + int(rng.integers(10, 120))],
                    fill=tuple(int(v) for v in rng.integers(0, 256, 3)))
    for i in range(300):
        d.text((int(rng.integers(0, W - 200)), int(rng.integers(0, H - 20))), "The quick brown fox %d" % i, fill=(0, 0, 0))
    return np.asarray(im)


def make_pool(distinct: int):
    from PIL import Image
    from datago_amd import synth
    pool = {k: [] for k in KINDS}
    for i in range(distinct):
        rng = np.random.default_rng(900 + i)
        rgb = screenshot(rng) if i % 2 else synth.synth_pixels(rng, W, H, False)
        for kind in KINDS:
            buf = io.BytesIO()
            if kind == "webp":
                Image.fromarray(rgb).save(buf, format="WEBP", lossless=True, exact=True, method=4, quality=75)
            else:
                Image.fromarray(rgb).save(buf, format="PNG")
            pool[kind].append(buf.getvalue())
    return pool


def load_pool(path: str, distinct: int):
    if path and os.path.exists(path):
        z = np.load(path)
        return {k: [z["%s_%d" % (k, i)].tobytes() for i in range(int(z["distinct"]))] for k in KINDS}
    pool = make_pool(distinct)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        np.savez(path, distinct=distinct, **{"%s_%d" % (k, i): np.frombuffer(f, np.uint8)
                                              for k in KINDS for i, f in enumerate(pool[k])})
    return pool


def _pillow_one(job):
    from PIL import Image
    data, size = job
    im = Image.open(io.BytesIO(data)).resize(size, Image.LANCZOS)
    return len(im.tobytes())


def pillow_rate(files, size, procs: int, passes: int = 3):
    jobs = [(f, size) for f in files]
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(_pillow_one, jobs[:4 * procs], chunksize=4)  # warm-up: workers started, Pillow imported
        secs = []
        for _ in range(passes):
            t0 = time.perf_counter()
            pool.map(_pillow_one, jobs, chunksize=4)
            secs.append(time.perf_counter() - t0)
    med = statistics.median(secs)
    return {"procs": procs, "ms_per_batch": round(1e3 * med, 1), "images_per_s": round(len(files) / med, 1)}


def run(ctx, L, files, steps: int, warmup: int, depth: int = 3):
    offs = np.cumsum([0] + [(len(f) + 15) // 16 * 16 for f in files])[:-1]
    host = np.zeros(int(offs[-1]) + len(files[-1]) + 64, np.uint8)
    for f, o in zip(files, offs):
        host[int(o):int(o) + len(f)] = np.frombuffer(f, np.uint8)
    ctx.host_register(host)
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
    ctx.host_unregister(host)
    for p in d_outs + [d_in]:
        ctx.free(p)
    med = {k: round(statistics.median(s[k] for s in stages), 4) for k in stages[0]}
    return {"coded_mb": round(sum(lens) / 2 ** 20, 2), "ms_per_batch": round(statistics.median(ms), 3),
            "images_per_s_one_in_flight": round(1e3 * len(files) / statistics.median(ms), 1),
            "images_per_s_pipelined": round(len(files) / piped, 1),
            "gpx_s_pipelined": round(len(files) * W * H / piped / 1e9, 3),
            "stages_ms": {k: v for k, v in med.items() if v >= 0.01}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pool", default="")
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--only", default="", help="webp, png or pillow")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pool = load_pool(a.pool, a.distinct)
    if a.prepare:
        print({k: [len(f) for f in v] for k, v in pool.items()})
        return 0
    res = {"images": a.n, "distinct": len(pool["webp"]), "size": [W, H], "coded_bytes": {k: [len(f) for f in v] for k, v in pool.items()}}
    webps = [pool["webp"][i % len(pool["webp"])] for i in range(a.n)]
    from oracle import buckets as B
    size = B.ARAwareTransform(512, 16, 0.5, 2.0).target_size(W, H)
    res["bucket"] = list(size)
    if a.only in ("", "pillow"):  # first: forked workers, before this process opens the GPU
        res["pillow"] = pillow_rate(webps, size, a.procs)
    from datago_amd import _lib as L
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)
    for kind in [k for k in KINDS if a.only in ("", k)]:
        ctx = L.Context(0, webp=True, **kw)
        files = [pool[kind][i % len(pool[kind])] for i in range(a.n)]
        res[kind] = run(ctx, L, files, a.steps, a.warmup)
        ctx.close()
    if not a.only:
        res["webp_over_png"] = round(res["webp"]["images_per_s_pipelined"] / res["png"]["images_per_s_pipelined"], 3)
        res["webp_over_pillow"] = round(res["webp"]["images_per_s_pipelined"] / res["pillow"]["images_per_s"], 2)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
