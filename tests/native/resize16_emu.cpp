// resize16_emu.cpp — a C ABI over datago_amd/csrc/dg_resize16.h for
// tests/test_resize16_cpu.py: the tap computation, the per-sample accumulate
// and the rounding that k_r16_taps / k_r16_v / k_r16_h run, on the CPU.
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -I datago_amd/csrc
#include <vector>

#include "dg_resize16.h"

using namespace dg;

extern "C" {

int r16e_geom(uint32_t W, uint32_t H, uint32_t bw, uint32_t bh, uint32_t out[4]) {
  R16Geom g;
  const bool ok = r16_geom(W, H, bw, bh, g);
  out[0] = g.w2;
  out[1] = g.h2;
  out[2] = g.x0;
  out[3] = g.y0;
  return ok ? 1 : 0;
}

// weights of output o into w (n_in slots are always enough); returns the count
uint32_t r16e_taps(uint32_t n_in, uint32_t n_out, uint32_t o, float *w, int32_t *left) {
  return r16_taps(n_in, n_out, o, w, *left);
}

uint16_t r16e_round(float t) { return r16_round(t); }

// src: H x W x C samples, tight; out: bh x bw x C.  The passes in the
// kernels' order: tap tables, vertical pass over the crop window's rows into
// f32, horizontal pass over its columns.  Returns 0 when the geometry fails.
int r16e_resize(const uint16_t *src, uint32_t W, uint32_t H, uint32_t C, uint32_t bw, uint32_t bh, uint16_t *out) {
  R16Geom g;
  if (!r16_geom(W, H, bw, bh, g)) return 0;
  if (g.w2 == W && g.h2 == H) {
    for (uint32_t y = 0; y < bh; y++)
      for (uint32_t i = 0; i < bw * C; i++)
        out[(size_t)y * bw * C + i] = src[((size_t)(y + g.y0) * W + g.x0) * C + i];
    return 1;
  }
  std::vector<float> mid((size_t)bh * W * C), w(W > H ? W : H);
  for (uint32_t y = 0; y < bh; y++) {
    int32_t left;
    const uint32_t n = r16_taps(H, g.h2, g.y0 + y, w.data(), left);
    for (uint32_t i = 0; i < W * C; i++) {
      float t = 0.0f;
      for (uint32_t k = 0; k < n; k++) t = r16_acc(t, (float)src[(size_t)(left + k) * W * C + i], w[k]);
      mid[(size_t)y * W * C + i] = t;
    }
  }
  for (uint32_t x = 0; x < bw; x++) {
    int32_t left;
    const uint32_t n = r16_taps(W, g.w2, g.x0 + x, w.data(), left);
    for (uint32_t y = 0; y < bh; y++)
      for (uint32_t c = 0; c < C; c++) {
        float t = 0.0f;
        for (uint32_t k = 0; k < n; k++) t = r16_acc(t, mid[((size_t)y * W + left + k) * C + c], w[k]);
        out[((size_t)y * bw + x) * C + c] = r16_round(t);
      }
  }
  return 1;
}

}  // extern "C"
