// dg_alph.h — the alpha plane of a lossy WebP (an ALPH chunk, option "webp_alpha"): the
// statements of k_alph_plane (dg_alph.hip), shared with the CPU emulation in
// tests/native/alph_emu.cpp.
//
// What they restate: libwebp's alpha unfilter (tests/ref_alph.py is the plain
// restatement the tests compare to, pinned to Pillow).  An ALPH payload is one header
// byte and then the filtered plane g, raw or as the green channel of a header-less VP8L
// stream; the output o is, mod 256, o[y][x] = g[y][x] + p with
//   no filter    p = 0
//   row 0        p = o[0][x-1] (0 at x = 0), with any other filter
//   column 0     p = o[y-1][0] below row 0, with any other filter
//   horizontal   p = o[y][x-1]
//   vertical     p = o[y-1][x]
//   gradient     p = clip(o[y][x-1] + o[y-1][x] - o[y-1][x-1], 0, 255)
//
// The walk is written once, here, over an environment E that supplies what differs
// between the wave and its emulation:
//   e.g(i)          filtered value of pixel i (a raw byte, or the green of the VP8L plane)
//   e.put(i, v)     store o of pixel i
//   e.get(i)        o of pixel i that an earlier lanes() section stored
//   e.sh(k)         a word of the wave's exchange area, k < kAlphShWords
//   e.lanes(f)      f(lane) for the 64 lanes, the sections ordered against each other
//   e.lanes_sh(f)   the same for a section that reads of other lanes only what they left
//                   in the exchange area (the wave does not wait for its loads and stores)
// A work item is one wave.  Sums mod 256 have no order, so three filters need no
// exchange between lanes at all:
//   none         item k copies pixels [k, k + 1) * 64 * w, lanes over consecutive pixels
//   horizontal   item k owns rows [k, k + 1) * 64, a lane per row: o[y][0] is the sum of
//                g[0..y][0], then the lane walks its row
//   vertical     item k owns columns [k, k + 1) * 64, a lane per column (neighbouring
//                lanes load neighbouring bytes): o[0][x] is the sum of g[0][0..x], then the
//                lane walks down its column; column 0 falls under the same rule
//   gradient     one item per image, over strips of 64 rows: lane r owns row y0 + r and
//                stands at x = t - r in step t, so L is its own last value and T, TL are
//                the last two values of lane r - 1, handed over through the exchange
//                area (two halves, by step parity); lane 0 of a strip below the first
//                reads T and TL from the plane.  What a step needs from memory is
//                fetched for kAlphAhead steps at once, so the wave waits for memory
//                once per kAlphAhead steps
// Every loop is bounded by w and h; no wave waits on another.
#pragma once
#include "dg_types.h"

namespace dg {

constexpr uint32_t kAlphNone = 0, kAlphHoriz = 1, kAlphVert = 2, kAlphGrad = 3;  // bits 2-3 of the header byte
constexpr uint32_t kAlphRaw = 0, kAlphVp8l = 1;                                  // bits 0-1
constexpr uint32_t kAlphAhead = 8;  // steps of the gradient walk served by one fetch
// the exchange area: 2 x (value, value before it) x 64 lanes, the fetched g per step and lane, lane 0's T and TL per step
constexpr uint32_t kAlphShG = 256, kAlphShUp = kAlphShG + 64 * kAlphAhead, kAlphShWords = kAlphShUp + 2 * kAlphAhead;

// What the host refuses of a header byte, as libwebp does: a compression above 1, a
// pre-processing (bits 4-5) above 1, a reserved bit.  Pre-processing 1 says the encoder
// quantised the levels; decoding does not change with it.
DG_HD bool alph_header_ok(uint32_t hdr) { return (hdr & 3u) <= kAlphVp8l && !(hdr & 0xe0u); }
DG_HD uint32_t alph_compression(uint32_t hdr) { return hdr & 3u; }
DG_HD uint32_t alph_filter(uint32_t hdr) { return (hdr >> 2) & 3u; }

// Work items (waves) of a w x h plane.
DG_HD uint32_t alph_items(uint32_t filter, uint32_t w, uint32_t h) {
  return filter == kAlphGrad ? 1u : filter == kAlphVert ? (w + 63u) / 64u : (h + 63u) / 64u;
}

DG_HD uint32_t alph_grad(uint32_t L, uint32_t T, uint32_t TL) {
  const int32_t v = (int32_t)L + (int32_t)T - (int32_t)TL;
  return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v;
}

template <class E>
DG_HD void alph_gradient(E &e, uint32_t w, uint32_t h) {
  const uint32_t steps = w + 63u;
  for (uint32_t y0 = 0; y0 < h; y0 += 64u) {
    e.lanes([&](uint32_t r) {
      for (uint32_t k = 0; k < 4u; k++) e.sh(64u * k + r) = 0u;
    });
    for (uint32_t t0 = 0; t0 < steps; t0 += kAlphAhead) {
      e.lanes([&](uint32_t r) {  // the strip above is stored by now
        const uint32_t y = y0 + r;
        for (uint32_t q = 0; q < kAlphAhead; q++) {
          const uint32_t x = t0 + q - r;  // (below zero it wraps: then >= w)
          const bool on = y < h && x < w;
          e.sh(kAlphShG + 64u * q + r) = on ? e.g(y * w + x) : 0u;
          if (r == 0u) {
            e.sh(kAlphShUp + 2u * q) = (y0 && on) ? e.get((y - 1u) * w + x) : 0u;
            e.sh(kAlphShUp + 2u * q + 1u) = (y0 && on && x) ? e.get((y - 1u) * w + x - 1u) : 0u;
          }
        }
      });
      for (uint32_t q = 0; q < kAlphAhead && t0 + q < steps; q++) {
        const uint32_t t = t0 + q, rb = (t & 1u) * 128u, wb = rb ^ 128u;
        e.lanes_sh([&](uint32_t r) {
          const uint32_t y = y0 + r, x = t - r;
          const uint32_t L = e.sh(rb + r);
          const uint32_t T = r ? e.sh(rb + r - 1u) : e.sh(kAlphShUp + 2u * q);
          const uint32_t TL = r ? e.sh(rb + 64u + r - 1u) : e.sh(kAlphShUp + 2u * q + 1u);
          uint32_t v = 0;
          if (y < h && x < w) {
            const uint32_t p = y == 0u ? (x ? L : 0u) : x == 0u ? T : alph_grad(L, T, TL);
            v = (e.sh(kAlphShG + 64u * q + r) + p) & 255u;
            e.put(y * w + x, v);
          }
          e.sh(wb + r) = v;
          e.sh(wb + 64u + r) = L;
        });
      }
    }
  }
}

// Item `item` of alph_items(filter, w, h).
template <class E>
DG_HD void alph_unfilter(E &e, uint32_t filter, uint32_t w, uint32_t h, uint32_t item) {
  if (filter == kAlphGrad) {
    if (item == 0u) alph_gradient(e, w, h);
    return;
  }
  e.lanes([&](uint32_t r) {
    if (filter == kAlphNone) {
      const uint32_t n = w * h, i0 = item * 64u * w;
      const uint32_t i1 = n - i0 < 64u * w ? n : i0 + 64u * w;
      for (uint32_t i = i0 + r; i < i1; i += 64u) e.put(i, e.g(i));
    } else if (filter == kAlphHoriz) {
      const uint32_t y = item * 64u + r;
      if (y >= h) return;
      uint32_t acc = 0;
      for (uint32_t k = 0; k < y; k++) acc += e.g(k * w);
      for (uint32_t x = 0; x < w; x++) {
        acc = (acc + e.g(y * w + x)) & 255u;
        e.put(y * w + x, acc);
      }
    } else {
      const uint32_t x = item * 64u + r;
      if (x >= w) return;
      uint32_t acc = 0;
      for (uint32_t k = 0; k < x; k++) acc += e.g(k);
      for (uint32_t y = 0; y < h; y++) {
        acc = (acc + e.g(y * w + x)) & 255u;
        e.put(y * w + x, acc);
      }
    }
  });
}

}  // namespace dg
