#!/usr/bin/env python
"""The rate of lossy WebP files with alpha (context options "webp_lossy" and "webp_alpha")
beside where they go today and beside the same frames without their alpha: the pool of
tools/webp_lossy_rate.py (256 images 1024x1536, a few distinct seeded images, half photo-like,
half screenshot-like, written by Pillow's WebP writer at quality 75, method 4), each with an
alpha plane.  Half of the distinct images carry a plane libwebp stores raw (per-pixel noise,
which its lossless coder cannot shrink), half a cut-out mask with soft edges, which it codes
as a VP8L stream; the header byte of every ALPH chunk is checked.  Sent through
dg_submit_device, device-resident input and output, by one context (crop_and_resize to the
512 / 16 buckets).  Reported: ms per batch with one batch in flight (median), the pipelined
rate with three in flight and the stages of dg_last_batch_timings (option "timing": the alpha
stream's k_vp8l_decode and k_vp8l_inverse, k_vp8_parse, k_vp8_recon, k_vp8_filter and
k_alph_plane run in the png_inflate span, one after the other on one stream; k_vp8_rgb in
png_unfilter), for all files, for the raw-coded and the VP8L-coded half alone, and for the same
files' `VP8 ` chunks as simple files under "webp_lossy" alone.  Beside them: Pillow decoding
and a Lanczos resize to the bucket's size of the same files on 16 processes (measured before
the GPU is opened; the workers never touch it).  --no-pillow leaves that out (a run under a
kernel trace, for the per-kernel spans).

    python tools/webp_alpha_rate.py [--n 256] [--distinct 4] [--steps 6] [--warmup 2] [--procs 16] [--no-pillow] [--out r.json]
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


def cutout(rng):
    """A product cut-out: opaque ellipses on a transparent ground, edges a few pixels soft."""
    y, x = np.mgrid[0:H, 0:W]
    a = np.zeros((H, W), np.float64)
    for _ in range(6):
        cx, cy = rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H
        rx, ry = rng.uniform(0.1, 0.35) * W, rng.uniform(0.1, 0.35) * H
        d = np.sqrt(((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2)
        a = np.maximum(a, np.clip((1.0 - d) * min(rx, ry) / 3.0, 0.0, 1.0))
    return (a * 255.0 + 0.5).astype(np.uint8)


def chunks(data):
    out, pos = {}, 12
    while pos + 8 <= len(data):
        n = int.from_bytes(data[pos + 4:pos + 8], "little")
        out.setdefault(data[pos:pos + 4], data[pos + 8:pos + 8 + n])
        pos += 8 + n + (n & 1)
    return out


def without_alpha(data):
    """The file's `VP8 ` chunk as a simple file."""
    body = chunks(data)[b"VP8 "]
    riff = b"WEBP" + b"VP8 " + len(body).to_bytes(4, "little") + body + (b"\0" if len(body) & 1 else b"")
    return b"RIFF" + len(riff).to_bytes(4, "little") + riff


def make_pool(distinct: int):
    """[(file, compression of its ALPH chunk)]: the first half raw, the second VP8L."""
    from PIL import Image
    from datago_amd import synth
    files = []
    for i in range(distinct):
        rng = np.random.default_rng(900 + i)
        rgb = WR.screenshot(rng) if i % 2 else synth.synth_pixels(rng, W, H, False)
        want = 0 if i < distinct // 2 else 1
        alpha = rng.integers(0, 256, (H, W), dtype=np.uint8) if want == 0 else cutout(rng)
        buf = io.BytesIO()
        Image.fromarray(np.dstack([rgb, alpha]), "RGBA").save(buf, format="WEBP", quality=75, method=4)
        hdr = chunks(buf.getvalue())[b"ALPH"][0]
        assert hdr & 3 == want, (i, hdr)
        files.append((buf.getvalue(), hdr))
    return files


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pool = make_pool(a.distinct)
    res = {"images": a.n, "distinct": len(pool), "size": [W, H], "quality": 75, "method": 4,
           "coded_bytes": [len(f) for f, _ in pool], "alph_header_bytes": [h for _, h in pool],
           "alph_bytes": [len(chunks(f)[b"ALPH"]) for f, _ in pool]}
    files = [pool[i % len(pool)][0] for i in range(a.n)]
    half = {"raw": [pool[i % (len(pool) // 2)][0] for i in range(a.n)],
            "vp8l": [pool[len(pool) // 2 + i % (len(pool) - len(pool) // 2)][0] for i in range(a.n)]}
    from oracle import buckets as B
    size = B.ARAwareTransform(512, 16, 0.5, 2.0).target_size(W, H)
    res["bucket"] = list(size)
    if not a.no_pillow:  # first: forked workers, before this process opens the GPU
        res["pillow"] = WR.pillow_rate(files, size, a.procs)
        print(json.dumps(res["pillow"]), flush=True)
    from datago_amd import _lib as L
    kw = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=16, min_aspect_ratio=0.5, max_aspect_ratio=2.0)
    ctx = L.Context(0, webp_lossy=True, webp_alpha=True, **kw)
    res["webp_alpha"] = WR.run(ctx, L, files, a.steps, a.warmup)
    print(json.dumps(res["webp_alpha"]), flush=True)
    for k, fs in half.items():  # a whole batch of one kind each
        res["webp_alpha_" + k] = WR.run(ctx, L, fs, 3, 1)
    ctx.close()
    ctx = L.Context(0, webp_lossy=True, **kw)  # the same frames without their alpha
    res["webp_lossy_same_frames"] = WR.run(ctx, L, [without_alpha(f) for f in files], a.steps, a.warmup)
    ctx.close()
    res["alpha_over_same_frames"] = round(res["webp_alpha"]["images_per_s_pipelined"] / res["webp_lossy_same_frames"]["images_per_s_pipelined"], 3)
    if not a.no_pillow:
        res["webp_alpha_over_pillow"] = round(res["webp_alpha"]["images_per_s_pipelined"] / res["pillow"]["images_per_s"], 2)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
