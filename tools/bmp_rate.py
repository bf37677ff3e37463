#!/usr/bin/env python
"""The rate of Windows bitmaps (context option "bmp") beside the paths the same
pixels could take: a pool of 1024x1536 images (a few distinct seeded photo-like
images, repeated) written as

    bmp24    24-bit uncompressed (4.7 MB each)
    bmp8     8-bit palette, uncompressed (Pillow's 256-colour quantisation)
    rle8     the same indices as BI_RLE8: runs of 3 and more as runs, the rest in
             absolute blocks (short runs and absolute blocks mix)
    png24    the 24-bit pixels as an RGB PNG   } the nearest existing GPU path
    png8     the indices as a paletted PNG     }

and sent through dg_submit_device, device-resident input and output, by one
context (crop_and_resize to the 512 / 16 buckets).  Per pool: ms per batch with
one batch in flight (median), the pipelined rate with three in flight, and the
stages of dg_last_batch_timings (option "timing"; k_bmp_rle runs in the
png_inflate span, k_bmp_expand in png_unfilter).  Beside them, where these files
go today: Pillow decoding, RGB conversion and a Lanczos resize to the bucket's
size of the same BMP files on 16 processes (measured before the GPU is opened;
the workers never touch it; Pillow's RLE decoder is a Python loop, so that pool
is a sample of the files and one pass).

    python tools/bmp_rate.py [--n 256] [--distinct 2] [--steps 12] [--warmup 3] [--pool pool.npz] [--procs 16] [--out r.json]

--pool caches the files.  --prepare writes the cache and stops (no GPU needed)."""
import argparse
import io
import json
import multiprocessing as mp
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1024, 1536
KINDS = ("bmp24", "bmp8", "rle8", "png24", "png8")
BMPS = ("bmp24", "bmp8", "rle8")


def rle8_stream(idx: np.ndarray) -> bytes:
    """BI_RLE8 of idx (rows top first), bottom-up: per row runs of 3 and more as runs, the stretches between them
    as absolute blocks (what is left under 3 pixels as runs of 1), end-of-line; end-of-bitmap."""
    out = bytearray()
    for r in range(idx.shape[0] - 1, -1, -1):
        row = idx[r]
        n = len(row)
        edge = np.flatnonzero(np.diff(row)) + 1
        starts = np.concatenate(([0], edge))
        lens = np.diff(np.concatenate((starts, [n])))
        lit = bytearray()

        def flush():
            k = 0
            while len(lit) - k >= 3:
                m = min(255, len(lit) - k)
                out.extend((0, m))
                out.extend(lit[k:k + m])
                if m & 1:
                    out.append(0)
                k += m
            for v in lit[k:]:
                out.extend((1, v))
            lit.clear()
        for s, ln in zip(starts.tolist(), lens.tolist()):
            v = int(row[s])
            if ln >= 3:
                flush()
                while ln > 0:
                    m = min(255, ln)
                    out.extend((m, v))
                    ln -= m
            else:
                lit.extend([v] * ln)
        flush()
        out.extend((0, 0))
    out.extend((0, 1))
    return bytes(out)


def bmp_file(bits: int, compression: int, data: bytes, pal_bgrx: bytes = b"") -> bytes:
    info = struct.pack("<IiiHHIIiiII", 40, W, H, 1, bits, compression, len(data), 2835, 2835, 0, 0)
    off = 14 + 40 + len(pal_bgrx)
    return b"BM" + struct.pack("<IHHI", off + len(data), 0, 0, off) + info + pal_bgrx + data


def make_pool(distinct: int):
    from PIL import Image
    from datago_amd import synth
    pool = {k: [] for k in KINDS}
    for i in range(distinct):
        rgb = synth.synth_pixels(np.random.default_rng(900 + i), W, H, False)
        im = Image.fromarray(rgb)
        q = im.quantize(256)
        idx = np.asarray(q)
        pal = np.zeros((256, 4), np.uint8)
        p = np.frombuffer(bytes(q.getpalette()[:768]).ljust(768, b"\0"), np.uint8).reshape(256, 3)
        pal[:, :3] = p[:, ::-1]
        for kind, img in (("bmp24", im), ("bmp8", q)):
            buf = io.BytesIO()
            img.save(buf, format="BMP")
            pool[kind].append(buf.getvalue())
        pool["rle8"].append(bmp_file(8, 1, rle8_stream(idx), pal.tobytes()))
        for kind, img in (("png24", im), ("png8", q)):
            buf = io.BytesIO()
            img.save(buf, format="PNG")
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
    im = Image.open(io.BytesIO(data)).convert("RGB").resize(size, Image.LANCZOS)
    return len(im.tobytes())


def pillow_rate(files, size, procs: int, passes: int = 3, warm: bool = True):
    jobs = [(f, size) for f in files]
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(_pillow_one, jobs[:procs] if not warm else jobs[:4 * procs], chunksize=1 if not warm else 4)
        secs = []
        for _ in range(passes):
            t0 = time.perf_counter()
            pool.map(_pillow_one, jobs, chunksize=1 if not warm else 4)
            secs.append(time.perf_counter() - t0)
    med = statistics.median(secs)
    return {"procs": procs, "files": len(files), "passes": passes, "ms_per_pass": round(1e3 * med, 1),
            "images_per_s": round(len(files) / med, 1)}


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
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pool", default="")
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--only", default="", help="one of the kinds, or pillow")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pool = load_pool(a.pool, a.distinct)
    if a.prepare:
        print({k: [len(f) for f in v] for k, v in pool.items()})
        return 0
    res = {"images": a.n, "distinct": len(pool["bmp24"]), "size": [W, H]}
    from oracle import buckets as B
    size = B.ARAwareTransform(512, 16, 0.5, 2.0).target_size(W, H)
    res["bucket"] = list(size)
    if a.only in ("", "pillow"):  # first: forked workers, before this process opens the GPU
        res["pillow"] = {}
        for kind in BMPS:
            files = [pool[kind][i % len(pool[kind])] for i in range(a.n)]
            if kind == "rle8":  # a Python loop per pixel: two files per worker, once
                res["pillow"][kind] = pillow_rate(files[:2 * a.procs], size, a.procs, passes=1, warm=False)
            else:
                res["pillow"][kind] = pillow_rate(files, size, a.procs)
    from datago_amd import _lib as L
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)
    for kind in [k for k in KINDS if a.only in ("", k)]:
        ctx = L.Context(0, bmp=True, **kw)
        files = [pool[kind][i % len(pool[kind])] for i in range(a.n)]
        res[kind] = run(ctx, L, files, a.steps, a.warmup)
        ctx.close()
    if not a.only:
        r = lambda k: res[k]["images_per_s_pipelined"]  # noqa: E731
        res["bmp24_over_png24"] = round(r("bmp24") / r("png24"), 3)
        res["bmp8_over_png8"] = round(r("bmp8") / r("png8"), 3)
        res["rle8_over_png8"] = round(r("rle8") / r("png8"), 3)
        for kind in BMPS:
            res["%s_over_pillow" % kind] = round(r(kind) / res["pillow"][kind]["images_per_s"], 2)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
