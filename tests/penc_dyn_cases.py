"""Inputs of the "penc_dynamic" tests beyond enc_cases.png_cases(), and the
references of all of them under tests/ref_penc_dyn.py, computed once per
process.  A plain helper module (NumPy only, no GPU, no fixtures).

  new_cases()  -> [(label, uint8 H x W x C)]
  all_cases()  -> png_cases() (label, array) followed by new_cases()
  dyn_ref(label, arr) -> ref_penc_dyn.encode(arr), kept per label
  huffman_depth(freq) -> the longest code of a plain (unlimited) Huffman code
"""
import heapq

import numpy as np

import enc_cases as E

FIB_LABEL = "fibonacci_gray"
# the cases whose run-length tokens need the 7-bit limiter (test_penc_dyn_cpu.py asserts it)
CL_LIMITED = ("filt_vramp_c4", "filt_paeth_c3", "expand_gray_odd")


def fibonacci_image():
    """256 x 475 gray: byte values 0..23 with Fibonacci frequencies, 0 the most frequent, shuffled: a plain
    Huffman code of its literals is deeper than 15 (the CPU test asserts that, not this comment)."""
    h, w = 256, 475
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    counts = fib[::-1]  # value 0 takes the largest
    counts[0] += h * w - sum(counts)
    assert counts[0] > 0
    px = np.repeat(np.arange(24, dtype=np.uint8), counts)
    np.random.default_rng(4100).shuffle(px)
    return px.reshape(h, w, 1)


def new_cases():
    from datago_amd import synth
    rng = np.random.default_rng(4000)
    rgb = np.ascontiguousarray(synth.synth_pixels(np.random.default_rng(4001), 128, 128)).reshape(128, 128, 3)
    gray = np.ascontiguousarray(synth.synth_pixels(np.random.default_rng(4002), 176, 80, gray=True)).reshape(80, 176, 1)
    return [("photo_rgb_128", rgb.astype(np.uint8)),
            ("photo_gray_176x80", gray.astype(np.uint8)),
            ("const_gray_128", np.full((128, 128, 1), 77, np.uint8)),
            ("random_rgba_64", rng.integers(0, 256, (64, 64, 4)).astype(np.uint8)),
            ("one_pixel_gray", np.array([[[201]]], np.uint8)),
            ("rgb_3x2", rng.integers(0, 256, (2, 3, 3)).astype(np.uint8)),
            (FIB_LABEL, fibonacci_image())]


PHOTO_LABELS = ("photo_rgb_128", "photo_gray_176x80")
_all = []


def all_cases():
    if not _all:
        _all.extend([(label, arr) for label, arr, _ in E.png_cases()] + new_cases())
    return _all


_refs = {}


def dyn_ref(label, arr):
    if label not in _refs:
        import ref_penc_dyn
        _refs[label] = ref_penc_dyn.encode(arr)
    return _refs[label]


def huffman_depth(freq):
    """(longest code, sum of f * length) of a plain Huffman code over the used symbols (two or more).  At equal
    weight a leaf goes before a merged node and older nodes before newer: of the optimal codes, a shallow one,
    so a depth above a limit says that the limit binds."""
    heap = [(f, i, 0, 0) for i, f in enumerate(freq) if f > 0]  # weight, tiebreak, depth, cost
    assert len(heap) >= 2
    heapq.heapify(heap)
    tie = len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tie, max(a[2], b[2]) + 1, a[3] + b[3] + a[0] + b[0]))
        tie += 1
    return heap[0][2], heap[0][3]
