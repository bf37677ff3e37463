#!/usr/bin/env python
"""First figure for the 16-bit PNG re-encode (context option "penc16"): one
batch, device-resident input and output, of 24 16-bit PNGs 512x512 -- depth-map
like (a smooth field with +-40 noise), half L16 (1,024 row bytes), half RGBA16
(4,096 row bytes) -- under default_image_size=512, downsampling_ratio=32, so
every image is its bucket's size.  Contexts, all with png16:

    decode   no pre_encode_images: the decode-only base
    fixed    pre_encode_images as PNG, penc16
    dynamic  ... and penc_dynamic
    base8    (not a 16-bit run) 8-bit RGBA PNGs with the same row bytes and
             rows (256x512 and 1024x512, no transform) through the 8-bit
             re-encoder: k_penc_filter beside k_penc_filter16 under a trace

Median of 5 timed submissions after 3 warm-up ones, one batch in flight: a
latency figure, not the pipelined rate of bench.py.  Reported: ms per batch
(the added time is fixed / dynamic minus decode), the encoded bytes over the
raw sample bytes, and the filtered stream's bytes per batch (what a filter
kernel's traced time is divided by).

    python tools/penc16_bench.py [--n 24] [--steps 5] [--warmup 3]
                                 [--only all|decode|fixed|dynamic|base8] [--out result.json]

Under rocprofv3 --kernel-trace --stats, --only dynamic gives k_penc_filter16's
time and --only base8 k_penc_filter's."""
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

SIDE = 512


def depth_like(rng, h, w, spp):
    yy, xx = np.mgrid[0:h, 0:w]
    field = 20000 + 9000 * np.sin(xx / 97.0) * np.cos(yy / 131.0) + 11 * xx + 7 * yy
    px = field[:, :, None] + 1500.0 * np.arange(spp)[None, None, :] + rng.integers(-40, 41, size=(h, w, spp))
    return np.clip(px, 0, 65535).astype(np.uint16)


def make_files16(n: int):
    rng = np.random.default_rng(1616)
    files = []
    for i in range(n):
        spp = 1 if i % 2 == 0 else 4
        files.append(synth.encode_png16(depth_like(rng, SIDE, SIDE, spp), 0 if spp == 1 else 6, rng, level=6))
    return files


def make_files8(n: int):
    """8-bit RGBA with the row bytes and rows of make_files16's images."""
    rng = np.random.default_rng(1608)
    files = []
    for i in range(n):
        w = SIDE // 2 if i % 2 == 0 else 2 * SIDE  # 1,024 / 4,096 row bytes
        px = (depth_like(rng, SIDE, w, 4) >> 8).astype(np.uint8)
        px ^= rng.integers(0, 4, size=px.shape, dtype=np.uint8)
        files.append(synth.pil_png(px))
    return files


def run(ctx, files, steps: int, warmup: int, sample_bytes: int):
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
    infos = [L.probe(f)[1] for f in files]
    raw = sum(int(p.width) * int(p.height) * int(p.components) * sample_bytes for p in infos)
    rows = sum(int(p.height) for p in infos)
    med = statistics.median(ms)
    res = {"ms_per_batch": round(med, 3), "runs_ms": [round(v, 3) for v in ms], "raw_sample_bytes": raw,
           "file_mb": round(host.nbytes / 1e6, 2)}
    if metas[0].is_encoded:
        enc = sum(int(metas[i].nbytes) for i in range(len(files)))
        res.update(encoded_bytes=enc, encoded_over_raw=round(enc / raw, 4), filtered_stream_bytes=raw + rows)
    ctx.host_unregister(host)
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["all", "decode", "fixed", "dynamic", "base8"], default="all")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    kw = dict(crop_and_resize=True, default_image_size=SIDE, downsampling_ratio=32, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0, png16=True)
    enc = dict(pre_encode_images=True, encode_format=0)
    res = {}
    files = make_files16(a.n) if a.only != "base8" else []
    if a.only in ("all", "decode"):
        res["decode"] = run(L.Context(0, **kw), files, a.steps, a.warmup, 2)
    if a.only in ("all", "fixed"):
        res["fixed"] = run(L.Context(0, penc16=True, **kw, **enc), files, a.steps, a.warmup, 2)
    if a.only in ("all", "dynamic"):
        res["dynamic"] = run(L.Context(0, penc16=True, penc_dynamic=True, **kw, **enc), files, a.steps, a.warmup, 2)
    if a.only in ("all", "base8"):
        res["base8_dynamic"] = run(L.Context(0, penc_dynamic=True, **enc), make_files8(a.n), a.steps, a.warmup, 1)
    if "decode" in res:
        for k in ("fixed", "dynamic"):
            if k in res:
                res[k]["added_ms_per_batch"] = round(res[k]["ms_per_batch"] - res["decode"]["ms_per_batch"], 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
