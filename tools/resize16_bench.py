#!/usr/bin/env python
"""First figure for the 16-bit resize (context option "resize16"): one batch,
device-resident input and output, of 24 16-bit PNGs 1024x768 (half RGB16, half
L16, random per-row filters, zlib level 6) under default_image_size=512,
downsampling_ratio=32, against the same batch decoded only (png16 without a
transform).  Median of 5 timed submissions after 3 warm-up ones, one batch in
flight: a latency figure, not the pipelined rate of bench.py.

    python tools/resize16_bench.py [--n 24] [--steps 5] [--warmup 3] [--out result.json]

Under rocprofv3 --kernel-trace --stats the same run gives the times of
k_r16_taps / k_r16_v / k_r16_h (pass --only resize to leave the decode-only
context out of the trace)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datago_amd import _lib as L  # noqa: E402
from datago_amd import synth  # noqa: E402


def make_files(n: int, w: int, h: int):
    rng = np.random.default_rng(16)
    files = []
    for i in range(n):
        rgb = i % 2 == 0
        p8 = synth.synth_pixels(rng, w, h, gray=not rgb).reshape(h, w, 3 if rgb else 1)
        px = (p8.astype(np.uint16) << 8) | rng.integers(0, 256, size=p8.shape, dtype=np.uint16)  # a noisy low byte
        files.append(synth.encode_png16(px, 2 if rgb else 0, rng, filters="random", level=6))
    return files


def run(ctx, files, steps: int, warmup: int):
    blob = np.concatenate([np.frombuffer(f, np.uint8) for f in files])
    offs = np.cumsum([0] + [len(f) for f in files])[:-1]
    host = np.ascontiguousarray(blob)
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
    ms = []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        ticket, metas = ctx.submit_device(hp, dp, lens, d_outs, sizes)
        ctx.wait(ticket)
        if k >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
        assert all(metas[i].status == L.DG_OK for i in range(len(files))), L.last_error()
    mpx = sum(metas[i].original_width * metas[i].original_height for i in range(len(files))) / 1e6
    med = statistics.median(ms)
    ctx.host_unregister(host)
    return {"ms_per_batch": round(med, 3), "mpx_per_s": round(mpx / med * 1e3, 1), "runs_ms": [round(v, 3) for v in ms],
            "file_mb": round(host.nbytes / 1e6, 1), "output_mb": round(sum(sizes) / 1e6, 1)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "resize", "decode"], default="both")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    files = make_files(a.n, 1024, 768)
    res = {}
    if a.only in ("both", "decode"):
        res["decode_only"] = run(L.Context(0, png16=True), files, a.steps, a.warmup)
    if a.only in ("both", "resize"):
        ctx = L.Context(0, crop_and_resize=True, default_image_size=512, downsampling_ratio=32, min_aspect_ratio=0.5,
                        max_aspect_ratio=2.0, png16=True, resize16=True)
        res["resize16"] = run(ctx, files, a.steps, a.warmup)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
