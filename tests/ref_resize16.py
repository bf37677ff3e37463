"""NumPy float32 restatement of the 16-bit resize (context option "resize16";
DESIGN.md §3 "16-bit resize"): the image crate's resize_to_fill(Lanczos3) as
the reference applies it to every non-U8 pixel type.  Written independently of
the C++ (datago_amd/csrc/dg_resize16.h): plain loops over the taps, np.float32
values so that every operation rounds on its own, np.sin on float64 rounded to
float32, and the trunc-based rounding.  The reference for the resize16 tests."""
import math

import numpy as np

F = np.float32
PI32 = F(math.pi)


def round_half_away(v: float) -> int:
    """f64, v >= 0: half away from zero without the v + 0.5 rounding trap."""
    f = math.floor(v)
    return int(f) + (1 if v - f >= 0.5 else 0)


def geometry(W: int, H: int, bw: int, bh: int):
    """(w2, h2, x0, y0): resize_to_fill's intermediate size and the crop origin in it."""
    r = max(bw / W, bh / H)
    w2 = max(round_half_away(W * r), 1)
    h2 = max(round_half_away(H * r), 1)
    assert w2 >= bw and h2 >= bh
    if bw * h2 > w2 * bh:
        return w2, h2, 0, (h2 - bh) // 2
    return w2, h2, (w2 - bw) // 2, 0


def sinc(t):
    if t == 0:
        return F(1)
    a = F(t * PI32)
    return F(F(np.sin(np.float64(a))) / a)


def lanczos3(x):
    if abs(x) < 3:
        return F(sinc(x) * sinc(F(x / F(3))))
    return F(0)


def taps(n_in: int, n_out: int, o0: int = 0, count: int = None):
    """[(left, float32 weights)] for outputs o0 .. o0 + count of an axis n_in -> n_out."""
    ratio = F(F(n_in) / F(n_out))
    sratio = F(1) if ratio < 1 else ratio
    support = F(F(3) * sratio)
    out = []
    for o in range(o0, o0 + (n_out - o0 if count is None else count)):
        c = F(F(F(o) + F(0.5)) * ratio)
        left = min(max(int(np.floor(F(c - support))), 0), n_in - 1)
        right = min(max(int(np.ceil(F(c + support))), left + 1), n_in)
        c = F(c - F(0.5))
        w = np.zeros(right - left, F)
        s = F(0)
        for k, i in enumerate(range(left, right)):
            w[k] = lanczos3(F(F(F(i) - c) / sratio))
            s = F(s + w[k])
        out.append((left, (w / s).astype(F)))
    return out


def round_sample(t: np.ndarray) -> np.ndarray:
    """clamp to [0, 65535], round half away from zero: r = trunc(t); if t - r >= 0.5: r += 1."""
    t = np.minimum(np.maximum(np.asarray(t, F), F(0)), F(65535))
    r = np.trunc(t)
    r = r + ((t - r) >= F(0.5)).astype(F)
    return r.astype(np.uint16)


def accumulate(rows, weights):
    """t = 0; for the taps in order: t = t + sample * w (a rounded multiply, then a rounded add)."""
    t = np.zeros(rows[0].shape, F)
    for r, w in zip(rows, weights):
        t = (t + (r.astype(F) * F(w)).astype(F)).astype(F)
    return t


def vpass(img: np.ndarray, h2: int, y0: int = 0, count: int = None) -> np.ndarray:
    """(H, W, C) samples -> float32 rows y0 .. y0 + count of the h2-row intermediate."""
    tp = taps(img.shape[0], h2, y0, count)
    return np.stack([accumulate([img[left + k] for k in range(len(w))], w) for left, w in tp], axis=0)


def hpass(mid: np.ndarray, w2: int, x0: int = 0, count: int = None) -> np.ndarray:
    """float32 (rows, W, C) -> uint16 columns x0 .. x0 + count of the w2-column result."""
    tp = taps(mid.shape[1], w2, x0, count)
    return np.stack([round_sample(accumulate([mid[:, left + k] for k in range(len(w))], w)) for left, w in tp], axis=1)


def resize_to_fill(img: np.ndarray, bw: int, bh: int) -> np.ndarray:
    """uint16 (H, W, C) -> uint16 (bh, bw, C).  Only the crop window of the
    intermediate is computed: every output depends on its own taps alone."""
    assert img.dtype == np.uint16 and img.ndim == 3
    H, W, _ = img.shape
    w2, h2, x0, y0 = geometry(W, H, bw, bh)
    if (w2, h2) == (W, H):
        return img[y0:y0 + bh, x0:x0 + bw].copy()
    return hpass(vpass(img, h2, y0, bh), w2, x0, bw)


def to_rgb8(px: np.ndarray) -> np.ndarray:
    """image_to_rgb8 on 16-bit samples: (v + 128) // 257, luma replicated, alpha dropped."""
    colour = px[:, :, :3] if px.shape[2] >= 3 else np.repeat(px[:, :, :1], 3, axis=2)
    return ((colour.astype(np.uint32) + 128) // 257).astype(np.uint8)
