// dg_resize16.h — the 16-bit resize (option "resize16"): arithmetic shared by
// the host planner, the kernels in dg_resize16.hip and the CPU emulator in
// tests/native/resize16_emu.cpp.
//
// The reference sends every non-U8 pixel type to the image crate's
// resize_to_fill(w, h, Lanczos3) (image_processing.rs:269-331): a vertical
// pass into an f32 intermediate, then a horizontal pass, f32 weights and
// accumulation, one rounding at the end, an integer centre crop, no alpha
// premultiply.  DESIGN.md §3 "16-bit resize" holds the normative restatement.
//
// Every f32 operation here is rounded on its own (IEEE binary32, nearest
// even): no contraction into FMAs, no reassociation, correctly rounded
// division.  On the device the explicit *_rn intrinsics say so whatever the
// build's flags; the host side is compiled with -ffp-contract=off.
#pragma once
#include <stddef.h>

#include "dg_pixel.h"

namespace dg {

#if defined(__HIP_DEVICE_COMPILE__)
DG_HD float r16_add(float a, float b) { return __fadd_rn(a, b); }
DG_HD float r16_sub(float a, float b) { return __fsub_rn(a, b); }
DG_HD float r16_mul(float a, float b) { return __fmul_rn(a, b); }
DG_HD float r16_div(float a, float b) { return __fdiv_rn(a, b); }
#else
DG_HD float r16_add(float a, float b) { return a + b; }
DG_HD float r16_sub(float a, float b) { return a - b; }
DG_HD float r16_mul(float a, float b) { return a * b; }
DG_HD float r16_div(float a, float b) { return a / b; }
#endif

// resize_to_fill's intermediate size (w2, h2) and the origin (x0, y0) of the
// bw x bh crop inside it.  False when the intermediate would not cover the
// target (the formulas never produce that; the caller refuses the image).
struct R16Geom {
  uint32_t w2, h2, x0, y0;
};
DG_HD bool r16_geom(uint32_t W, uint32_t H, uint32_t bw, uint32_t bh, R16Geom &g) {
  const double rw = (double)bw / (double)W, rh = (double)bh / (double)H;
  const double r = rw > rh ? rw : rh;
  const double fw = __builtin_round((double)W * r), fh = __builtin_round((double)H * r);  // half away from zero
  g.w2 = fw < 1.0 ? 1u : (uint32_t)fw;
  g.h2 = fh < 1.0 ? 1u : (uint32_t)fh;
  g.x0 = g.y0 = 0;
  if (g.w2 < bw || g.h2 < bh) return false;
  if ((uint64_t)bw * g.h2 > (uint64_t)g.w2 * bh)
    g.y0 = (g.h2 - bh) / 2;
  else
    g.x0 = (g.w2 - bw) / 2;
  return true;
}

// The taps of output o of an axis n_in -> n_out: source samples [left, right),
// the centre c and the filter scale the weights are evaluated with.
struct R16Window {
  int32_t left, right;
  float c, sratio;
};
DG_HD R16Window r16_window(uint32_t n_in, uint32_t n_out, uint32_t o) {
  R16Window w;
  const float ratio = r16_div((float)n_in, (float)n_out);
  w.sratio = ratio < 1.0f ? 1.0f : ratio;
  const float support = r16_mul(3.0f, w.sratio);
  const float c = r16_mul(r16_add((float)o, 0.5f), ratio);
  int64_t l = (int64_t)__builtin_floorf(r16_sub(c, support));
  l = l < 0 ? 0 : (l > (int64_t)n_in - 1 ? (int64_t)n_in - 1 : l);
  int64_t r = (int64_t)__builtin_ceilf(r16_add(c, support));
  r = r < l + 1 ? l + 1 : (r > (int64_t)n_in ? (int64_t)n_in : r);
  w.left = (int32_t)l;
  w.right = (int32_t)r;
  w.c = r16_sub(c, 0.5f);
  return w;
}

// sin(a) = (f32) sin_f64((f64) a) with the portable fdlibm sin of dg_pixel.h
// (the crate calls the platform's sinf: faithful, not always correctly
// rounded -- the one known source of a 1-ulp weight difference).
DG_HD float r16_sinc(float t) {
  if (t == 0.0f) return 1.0f;
  const float a = r16_mul(t, 3.14159265358979323846f);
  return r16_div((float)dg_sin((double)a), a);
}
DG_HD float r16_lanczos3(float x) {
  const float ax = x < 0.0f ? -x : x;
  return ax < 3.0f ? r16_mul(r16_sinc(x), r16_sinc(r16_div(x, 3.0f))) : 0.0f;
}

// Normalised weights of output o into w[0 .. right - left): the raw weights,
// their sequential sum in tap order from 0, then every weight divided by it.
// Returns the count and sets left.  P: a pointer to float (any address space).
template <class P>
DG_HD uint32_t r16_taps(uint32_t n_in, uint32_t n_out, uint32_t o, P w, int32_t &left) {
  const R16Window b = r16_window(n_in, n_out, o);
  const uint32_t n = (uint32_t)(b.right - b.left);
  float sum = 0.0f;
  for (uint32_t k = 0; k < n; k++) {
    const float v = r16_lanczos3(r16_div(r16_sub((float)(b.left + (int32_t)k), b.c), b.sratio));
    w[k] = v;
    sum = r16_add(sum, v);
  }
  for (uint32_t k = 0; k < n; k++) w[k] = r16_div(w[k], sum);
  left = b.left;
  return n;
}

// One tap of either pass: a rounded multiply, then a rounded add.
DG_HD float r16_acc(float t, float sample, float w) { return r16_add(t, r16_mul(sample, w)); }

// The horizontal pass's final sample: clamp to [0, 65535], round half away
// from zero.  (floor(t + 0.5) is wrong: at t = 0.5 - 2^-25 the sum rounds up to 1.)
DG_HD uint16_t r16_round(float t) {
  t = t < 0.0f ? 0.0f : (t > 65535.0f ? 65535.0f : t);
  float r = __builtin_truncf(t);
  if (r16_sub(t, r) >= 0.5f) r = r16_add(r, 1.0f);
  return (uint16_t)r;
}

}  // namespace dg
