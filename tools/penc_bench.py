#!/usr/bin/env python
"""What context option "penc_dynamic" costs and saves: one batch, device-
resident input and output, of 24 photo-like RGB JPEGs 1024x768 decoded, resized
to their bucket (default_image_size=512, downsampling_ratio=32) and re-encoded
as PNG, through a context with the option at 0 (the fixed-Huffman block) and
one with it at 1 (per-image codes where shorter), in the same process.  Median
of 5 timed submissions after 3 warm-up ones, one batch in flight: a latency
figure, not the pipelined rate of bench.py.  Per context: ms per batch and the
total encoded bytes (and their ratio to the raw pixels).

    python tools/penc_bench.py [--n 24] [--steps 5] [--warmup 3] [--only both|fixed|dynamic] [--out result.json]

Under rocprofv3 --kernel-trace --stats the same run gives the times of
k_penc_tree and of the count / write kernels (pass --only dynamic to leave the
fixed context out of the trace)."""
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
    return [synth.make_jpeg(700 + i, w, h, 92, "4:2:0") for i in range(n)]


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
        assert all(metas[i].status == L.DG_OK and metas[i].is_encoded for i in range(len(files))), L.last_error()
    enc = sum(int(metas[i].nbytes) for i in range(len(files)))
    raw = sum(int(metas[i].width) * int(metas[i].height) * 3 for i in range(len(files)))
    med = statistics.median(ms)
    ctx.host_unregister(host)
    return {"ms_per_batch": round(med, 3), "runs_ms": [round(v, 3) for v in ms], "encoded_bytes": enc,
            "raw_pixel_bytes": raw, "encoded_over_raw": round(enc / raw, 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "fixed", "dynamic"], default="both")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    files = make_files(a.n, 1024, 768)
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=32, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0, pre_encode_images=True, encode_format=0)
    res = {}
    if a.only in ("both", "fixed"):
        res["fixed"] = run(L.Context(0, **kw), files, a.steps, a.warmup)
    if a.only in ("both", "dynamic"):
        res["dynamic"] = run(L.Context(0, penc_dynamic=True, **kw), files, a.steps, a.warmup)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
