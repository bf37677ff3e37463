#!/usr/bin/env python
"""What context option "jenc_optimize" costs and saves: one batch, device-
resident input and output, of 24 photo-like RGB JPEGs 1600x1200 decoded, resized
to their bucket (default_image_size=1024, downsampling_ratio=32, the headline
benchmark's buckets) and re-encoded as JPEG at quality 92, through a context
with the option at 0 (the Annex K tables) and one with it at 1 (per-image
tables), in the same process.  Median of the timed submissions after the
warm-up ones, one batch in flight: a latency figure, not the pipelined rate of
bench.py.  Per context: ms per batch, the "encode" stage of
dg_last_batch_timings over further submissions with option "timing" on (the
stage holds fdct, hist, tree, count, scan, write and stuff), and the encoded
bytes in total and per image.

    python tools/jenc_bench.py [--n 24] [--steps 9] [--warmup 3] [--only both|standard|optimized] [--out result.json]

A library built from a commit without the option (DG_LIB_PATH) runs with
--only standard.  Under rocprofv3 --kernel-trace --stats the same run gives the
times of k_enc_hist, k_enc_tree and of the count / write / stuff kernels (pass
--only to keep one context in the trace)."""
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
    return [synth.make_jpeg(900 + i, w, h, 92, "4:2:0") for i in range(n)]


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

    def once():
        t0 = time.perf_counter()
        ticket, metas = ctx.submit_device(hp, dp, lens, d_outs, sizes)
        ctx.wait(ticket)
        dt = 1e3 * (time.perf_counter() - t0)
        assert all(metas[i].status == L.DG_OK and metas[i].is_encoded for i in range(len(files))), L.last_error()
        return dt, metas

    ms = [once()[0] for _ in range(warmup + steps)][warmup:]
    ctx.set_option("timing", 1)
    enc_ms = []
    for _ in range(steps):
        _, metas = once()
        enc_ms.append(float(ctx.timings().get("encode", 0.0)))
    ctx.set_option("timing", 0)
    enc = [int(metas[i].nbytes) for i in range(len(files))]
    raw = sum(int(metas[i].width) * int(metas[i].height) * 3 for i in range(len(files)))
    ctx.host_unregister(host)
    return {"ms_per_batch": round(statistics.median(ms), 3), "runs_ms": [round(v, 3) for v in ms],
            "encode_stage_ms": round(statistics.median(enc_ms), 4), "encode_stage_runs_ms": [round(v, 4) for v in enc_ms],
            "encoded_bytes": sum(enc), "encoded_bytes_per_image": round(sum(enc) / len(enc), 1),
            "raw_pixel_bytes": raw, "encoded_over_raw": round(sum(enc) / raw, 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=24)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "standard", "optimized"], default="both")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    files = make_files(a.n, 1600, 1200)
    kw = dict(crop_and_resize=True, default_image_size=1024, downsampling_ratio=32, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0, pre_encode_images=True, encode_format=1, jpeg_quality=92)
    res = {}
    if a.only in ("both", "standard"):
        res["standard"] = run(L.Context(0, **kw), files, a.steps, a.warmup)
    if a.only in ("both", "optimized"):
        res["optimized"] = run(L.Context(0, jenc_optimize=True, **kw), files, a.steps, a.warmup)
    if len(res) == 2:
        res["bytes_ratio"] = round(res["optimized"]["encoded_bytes"] / res["standard"]["encoded_bytes"], 4)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
