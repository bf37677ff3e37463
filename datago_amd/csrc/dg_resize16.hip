// dg_resize16.hip — the 16-bit resize (option "resize16"): the image crate's
// resize_to_fill(Lanczos3) for 16-bit PNGs, restated in dg_resize16.h.
//
//   k_r16_taps  f32 tap tables of both passes (side stream, beside the inflate)
//   k_r16_v     u16 decoded rows -> f32 intermediate rows (vertical pass)
//   k_r16_h     f32 intermediate -> u16 output samples (horizontal pass, clamp, round)
//
// An image on this path holds its vertical pass in ImageDesc::pass[0]
// (kind kR16V) and its horizontal pass in pass[1] (kind kR16H):
//   bounds  int32 {left, count} per computed output (row of the crop window / output column)
//   coef    f32 weights, ksize slots per computed output
//   out0    first output of out_size that is computed (the crop folds into both passes)
// The intermediate holds the crop window's rows only, and of every row the
// samples [row0, row0 + width) of the decoded row that the cropped columns'
// taps read (pass[0].width samples, a multiple of 4; pass[1].row0 = that
// first sample).
#include <hip/hip_runtime.h>

#include "dg_resize16.h"
#include "kernels.h"

namespace dg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One lane per computed output of a pass; the taps run serially in the lane
// (the sequential sum is the semantics).  item0: bit 31 = pass, the rest =
// first output of the workgroup.
__global__ __launch_bounds__(256) void k_r16_taps(const ImageDesc *__restrict__ imgs,
                                                  const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  const ResizePass &ps = imgs[it.image].pass[it.item0 >> 31];
  const uint32_t j = (it.item0 & 0x7FFFFFFFu) + threadIdx.x;
  const uint32_t n_tab = ps.kind == kR16V ? ps.rows : ps.width;
  if (j >= n_tab) return;
  int32_t left;
  const uint32_t n = r16_taps(ps.in_size, ps.out_size, ps.out0 + j, gp<float>(ps.coef) + (size_t)j * ps.ksize, left);
  DG_GLOBAL int32_t *bd = gp<int32_t>(ps.bounds) + 2 * (size_t)j;
  bd[0] = left;
  bd[1] = (int32_t)n;
}

// Vertical pass: a workgroup takes 256 quads of adjacent samples of one
// intermediate row; a lane loads its quad (8 bytes of u16) from every tap row
// and stores 16 bytes of f32.  The row's weights are uniform in the workgroup.
__global__ __launch_bounds__(256) void k_r16_v(const ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  const ResizePass &ps = imgs[it.image].pass[0];
  const uint32_t qpr = ps.width >> 2, wgpr = (qpr + 255) / 256;
  const uint32_t row = it.item0 / wgpr;
  const uint32_t q = (it.item0 - row * wgpr) * 256 + threadIdx.x;
  if (q >= qpr) return;
  const DG_GLOBAL int32_t *bd = gp<const int32_t>(ps.bounds) + 2 * (size_t)row;
  const uint32_t left = (uint32_t)bd[0], n = (uint32_t)bd[1];
  const DG_GLOBAL float *w = gp<const float>(ps.coef) + (size_t)row * ps.ksize;
  const DG_GLOBAL uint8_t *s = gp<const uint8_t>(ps.src) + (size_t)left * ps.src_stride + (size_t)q * 8;
  float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
  for (uint32_t k = 0; k < n; k++) {
    const u32x2 v = *(const DG_GLOBAL u32x2 *)s;
    const float wk = w[k];
    t0 = r16_acc(t0, (float)(v.x & 0xFFFFu), wk);
    t1 = r16_acc(t1, (float)(v.x >> 16), wk);
    t2 = r16_acc(t2, (float)(v.y & 0xFFFFu), wk);
    t3 = r16_acc(t3, (float)(v.y >> 16), wk);
    s += ps.src_stride;
  }
  f32x4 r;
  r.x = t0;
  r.y = t1;
  r.z = t2;
  r.w = t3;
  *(DG_GLOBAL f32x4 *)(gp<uint8_t>(ps.dst) + (size_t)row * ps.dst_stride + (size_t)q * 16) = r;
}

// Horizontal pass: a workgroup takes 256 adjacent output pixels of one row, a
// lane one pixel with all its channels.  The taps are looped over the table
// (a 16x downscale has ~98); the intermediate row segment a workgroup reads
// stays in L2 / the vector cache between its lanes.
__global__ __launch_bounds__(256) void k_r16_h(const ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  const ResizePass &ps = imgs[it.image].pass[1];
  const uint32_t wgpr = (ps.width + 255) / 256;
  const uint32_t row = it.item0 / wgpr;
  const uint32_t x = (it.item0 - row * wgpr) * 256 + threadIdx.x;
  if (x >= ps.width) return;
  const uint32_t C = ps.C;
  const DG_GLOBAL int32_t *bd = gp<const int32_t>(ps.bounds) + 2 * (size_t)x;
  const uint32_t left = (uint32_t)bd[0], n = (uint32_t)bd[1];
  const DG_GLOBAL float *w = gp<const float>(ps.coef) + (size_t)x * ps.ksize;
  const DG_GLOBAL float *s = gp<const float>(ps.src + (uint64_t)row * ps.src_stride) + ((size_t)left * C - ps.row0);
  float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t k = 0; k < n; k++) {
    const float wk = w[k];
#pragma unroll
    for (uint32_t c = 0; c < 4; c++)
      if (c < C) t[c] = r16_acc(t[c], s[c], wk);
    s += C;
  }
  DG_GLOBAL uint16_t *d = gp<uint16_t>(ps.dst + (uint64_t)row * ps.dst_stride) + (size_t)x * C;
#pragma unroll
  for (uint32_t c = 0; c < 4; c++)
    if (c < C) d[c] = r16_round(t[c]);
}

#define DG_LAUNCH(kern, nwg, st, ...)                                              \
  do {                                                                            \
    if (nwg) hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), 0, st, __VA_ARGS__); \
  } while (0)

void launch_r16_taps(hipStream_t st, const ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  DG_LAUNCH(k_r16_taps, nwg, st, imgs, list);
}
void launch_r16_v(hipStream_t st, const ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  DG_LAUNCH(k_r16_v, nwg, st, imgs, list);
}
void launch_r16_h(hipStream_t st, const ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  DG_LAUNCH(k_r16_h, nwg, st, imgs, list);
}

}  // namespace dg
