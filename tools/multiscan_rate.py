#!/usr/bin/env python
"""The rate of non-interleaved baseline JPEGs (context option "jpeg_multiscan")
beside the two paths the same coefficients could take: a pool of 256 4:2:0
files 1024x1536 (a few distinct seeded images, repeated) written three ways
from one set of quantised coefficients --

    multiscan    one scan per component (tests/ref_jpeg_multiscan.py)
    single       one interleaved scan: the ceiling
    progressive  SOF2 (tests/ref_jpeg_h1v2.py's writer): where these files would
                 otherwise go

-- and sent through dg_submit_device, device-resident input and output, by one
context (crop_and_resize to the 512 / 16 buckets).  Per pool: ms per batch with
one batch in flight (median), the pipelined rate with three in flight in
Gpx/s of source pixels, and the stages of dg_last_batch_timings (option
"timing"; huff_write is k_ms_zero + k_huff_write).

    python tools/multiscan_rate.py [--n 256] [--distinct 4] [--steps 12] [--warmup 3] [--pool pool.npz] [--only KIND] [--ctx-opt KEY=VALUE] [--out r.json]

--pool caches the crafted files (writing them is minutes of Python).
--prepare writes the cache and stops (no GPU needed)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, SAMP = 1024, 1536, [(2, 2), (1, 1), (1, 1)]
KINDS = ("multiscan", "single", "progressive")


def make_pool(distinct: int, quality: int = 90):
    import jpeg_craft as J
    import ref_jpeg_h1v2 as RH
    import ref_jpeg_multiscan as R
    pool = {k: [] for k in KINDS}
    for i in range(distinct):
        comps, qtabs = R.craft(SAMP, W, H, seed=700 + i, quality=quality)
        pool["multiscan"].append(R.multiscan(comps, SAMP, W, H, qtabs, [[0], [1], [2]]))
        pool["single"].append(J.from_coefs(comps, SAMP, W, H, qtabs, tq=[0, 1, 1]))
        pool["progressive"].append(RH.progressive(comps, SAMP, W, H, qtabs, [0, 1, 1]))
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
    px = len(files) * W * H
    med = {k: round(statistics.median(s[k] for s in stages), 4) for k in stages[0]}
    return {"coded_mb": round(sum(lens) / 2 ** 20, 2), "ms_per_batch": round(statistics.median(ms), 3),
            "gpx_s_one_in_flight": round(px / statistics.median(ms) / 1e6, 2),
            "gpx_s_pipelined": round(px / piped / 1e9, 2), "stages_ms": {k: v for k, v in med.items() if v >= 0.01},
            "huff_write_ms": med.get("huff_write", 0.0)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pool", default="")
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--only", default="", help="one of the three pools")
    ap.add_argument("--ctx-opt", action="append", default=[], metavar="KEY=VALUE", help="context options to set")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pool = load_pool(a.pool, a.distinct)
    if a.prepare:
        print({k: [len(f) for f in v] for k, v in pool.items()})
        return 0
    from datago_amd import _lib as L
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)
    res = {"images": a.n, "distinct": len(pool["single"]), "size": [W, H], "sampling": "4:2:0"}
    for kind in ([a.only] if a.only else KINDS):
        ctx = L.Context(0, **kw)
        ctx.set_option("jpeg_multiscan", 1)
        for kv in a.ctx_opt:
            ctx.set_option(kv.split("=")[0], int(kv.split("=")[1]))
        files = [pool[kind][i % len(pool[kind])] for i in range(a.n)]
        res[kind] = run(ctx, L, files, a.steps, a.warmup)
        ctx.close()
    if not a.only:
        res["multiscan_over_single"] = round(res["multiscan"]["gpx_s_pipelined"] / res["single"]["gpx_s_pipelined"], 3)
        res["multiscan_over_progressive"] = round(res["multiscan"]["gpx_s_pipelined"] / res["progressive"]["gpx_s_pipelined"], 2)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
