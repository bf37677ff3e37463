// dg_bmp.hip — CDNA4 (gfx950) kernels of the BMP decode stage (option "bmp").
//
//   k_bmp_rle      RLE8 / RLE4 stream -> the bitmap's index plane (one byte per pixel,
//                  rows in stream order), one wave per image
//   k_bmp_expand   the file's pixel array or that index plane -> Rgb8 / Rgba8, top row
//                  first (row flip, palette, BGR -> RGB, mask byte selection)
//
// What they restate: image 0.25's BmpDecoder for load_from_memory, for the files it and
// Pillow decode to the same bytes; dg_bmp.h holds the lane routines and the scheme,
// tests/ref_bmp.py the CPU restatement the tests compare to.
//
// k_bmp_rle takes 64 two-byte units per step.  Every lane classifies its unit as a
// command; the lanes that are data of an absolute block are found by hopping from one
// absolute command to the next (a loop over the absolute commands of the window, not
// over its units); a prefix sum of the pixel counts gives the output positions; the
// step is cut at the first command that breaks the row order, where the data ends and
// with the last pixel.  Every loop is bounded by the stream's length: a step consumes
// 128 bytes or ends the decode.
//
// k_bmp_expand gives a lane four pixels of a row.  The coded bytes sit at any byte
// alignment, so a lane loads the aligned dwords that cover its 2 to 16 source bytes and
// shifts them into place: no byte loads, and the lanes of a wave read one contiguous span.
#include <hip/hip_runtime.h>

#include "dg_bmp.h"
#include "kernels.h"

namespace dg {

__device__ __forceinline__ uint32_t bmp_excl_scan(uint32_t v, uint32_t lane, uint32_t *total) {
  uint32_t x = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  *total = __shfl(x, 63);
  return x - v;
}

// Bits 0 .. k-1 (k <= 64).
__device__ __forceinline__ uint64_t bmp_below(uint32_t k) { return k >= 64u ? ~0ull : (1ull << k) - 1ull; }

// The aligned dword at `ad`; its bytes at or past `end` read as zero.
__device__ __forceinline__ uint32_t bmp_ld32(uint64_t ad, uint64_t end) {
  if (ad + 4u <= end) return *gp<const uint32_t>(ad);
  uint32_t v = 0;
  for (uint32_t q = 0; q < 4; q++)
    if (ad + q < end) v |= (uint32_t)*gp<const uint8_t>(ad + q) << (8u * q);
  return v;
}

// ------------------------------------------------------------ RLE

__global__ __launch_bounds__(64) void k_bmp_rle(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kBmpWinBytes];
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const BmpDesc g = im.bmp;
  const uint32_t lane = threadIdx.x;
  const uint32_t W = im.width, npix = W * im.height, len = g.data_len;
  const uint32_t rle4 = g.rle == 2u ? 1u : 0u, ppu = bmp_ppu(rle4);
  DG_GLOBAL uint8_t *out = gp<uint8_t>(g.idx);
  BmpRle s = {0u, 0u, 0u, 0u, 0u};
  uint64_t win_addr = 0;
  bool win_valid = false;
  uint32_t fail = 0;
  const uint32_t max_steps = len / (2u * kBmpStepUnits) + 2u;
  for (uint32_t step = 0; step < max_steps && s.o < npix; step++) {
    // ---- the source window: the bytes of this step's units
    if (s.pos < len) {
      const uint32_t k1 = len - s.pos < 2u * kBmpStepUnits ? len : s.pos + 2u * kBmpStepUnits;
      const uint64_t a0 = g.src + s.pos, a1 = g.src + k1 - 1u;
      if (!win_valid || a0 < win_addr || a1 >= win_addr + kBmpWinBytes) {
        __syncthreads();
        win_addr = a0 & ~3ull;
        win_valid = true;
#pragma unroll
        for (uint32_t r = 0; r < kBmpWinBytes / 256u; r++) {
          const uint32_t i = lane + 64u * r;
          ((uint32_t *)win)[i] = bmp_ld32(win_addr + 4ull * i, g.src_end);
        }
        __syncthreads();
      }
    }
    // ---- every unit as a command
    const uint32_t bp = s.pos + 2u * lane;
    const bool inb = bp + 2u <= len && bp + 2u > bp;
    uint32_t a = 0, b = 0;
    if (inb) {
      const uint32_t wi = (uint32_t)(g.src + bp - win_addr);
      a = win[wi];
      b = win[wi + 1u];
    }
    const uint32_t kind = bmp_unit_kind(a, b), q = bmp_unit_pixels(a, b);
    // ---- which units are data of an absolute block: the block carried in, then hop over the window's own
    const uint32_t first = s.data_units < kBmpStepUnits ? s.data_units : kBmpStepUnits;
    uint64_t data = bmp_below(first);
    uint32_t blk_left = s.data_left, blk_base = 0;
    uint32_t carry_units = s.data_units - first, carry_left = carry_units ? s.data_left - kBmpStepUnits * ppu : 0u;
    uint64_t rest = __ballot(inb && kind == kBmpAbs) & ~data;
    while (rest) {  // one trip per absolute command
      const uint32_t m = (uint32_t)__builtin_ctzll(rest);
      const uint32_t n = __shfl(q, m);
      const uint32_t lo = m + 1u, hi = lo + bmp_abs_units(n, rle4);
      const uint64_t cov = bmp_below(hi) & ~bmp_below(lo);
      if (lane >= lo && lane < hi) {
        blk_left = n;
        blk_base = lo;
      }
      data |= cov;
      if (hi > kBmpStepUnits) {
        carry_units = hi - kBmpStepUnits;
        carry_left = n - (kBmpStepUnits - lo) * ppu;
      }
      rest &= ~(cov | (1ull << m));
    }
    const bool isdata = (data >> lane) & 1ull;
    // ---- pixel counts and output positions
    uint32_t c = isdata ? bmp_data_count(blk_left, lane - blk_base, rle4) : kind == kBmpRun ? q : 0u;
    if (!inb) c = 0u;
    uint32_t total;
    const uint32_t o = s.o + bmp_excl_scan(c, lane, &total);
    // ---- the command before each command
    const uint64_t starts = ~data;
    const uint64_t before = starts & bmp_below(lane);
    const uint32_t pk = __shfl(kind, before ? 63u - (uint32_t)__builtin_clzll(before) : 0u);
    const bool prev_eol = before ? pk == kBmpEol : s.prev_eol != 0u;
    // ---- what cuts the step: the last pixel, the data's end, a command out of the row order
    const bool done = o >= npix;
    uint32_t f = 0;
    if (!inb)
      f = kBmpFailShort;
    else if (!isdata)
      f = bmp_cmd_fail(kind, q, o, W, prev_eol);
    const uint64_t evm = __ballot(done || f != 0u);
    const uint32_t ke = evm ? (uint32_t)__builtin_ctzll(evm) : kBmpStepUnits;
    if (ke < kBmpStepUnits && !__shfl((uint32_t)done, ke)) {
      fail = __shfl(f, ke);
      break;
    }
    // ---- the pixels
    const uint32_t cw = lane < ke ? c : 0u;
    if (isdata) {
#pragma unroll
      for (uint32_t t = 0; t < 4; t++)
        if (t < cw) out[o + t] = (uint8_t)bmp_data_pixel(a, b, t, rle4);
    } else if (cw <= kBmpShort) {
#pragma unroll
      for (uint32_t t = 0; t < kBmpShort; t++)
        if (t < cw) out[o + t] = (uint8_t)bmp_run_pixel(b, t, rle4);
    }
    uint64_t big = __ballot(!isdata && cw > kBmpShort);
    while (big) {  // long runs: the whole wave
      const uint32_t m = (uint32_t)__builtin_ctzll(big);
      big &= big - 1ull;
      const uint32_t ob = __shfl(o, m), cb = __shfl(cw, m), bb = __shfl(b, m);
      for (uint32_t t = lane; t < cb; t += 64u) out[ob + t] = (uint8_t)bmp_run_pixel(bb, t, rle4);
    }
    // ---- the state after the step
    if (ke < kBmpStepUnits) {
      s.o = npix;
    } else {
      s.pos += 2u * kBmpStepUnits;
      s.o += total;
      s.data_units = carry_units;
      s.data_left = carry_left;
      if (starts) s.prev_eol = __shfl(kind, 63u - (uint32_t)__builtin_clzll(starts)) == kBmpEol ? 1u : 0u;
    }
  }
  if (!fail && s.o < npix) fail = kBmpFailShort;
  if (fail && lane == 0) {
    im.bmp.fail = fail;
    im.status = 1;  // DG_ERR_UNSUPPORTED: the caller's CPU decoder decides
  }
}

// ------------------------------------------------------------ expand

// Four pixels of a row per thread, 64 threads: 256 outputs per work item.
__global__ __launch_bounds__(64) void k_bmp_expand(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const BmpDesc &g = im.bmp;
  const uint32_t W = im.width, H = im.height, gpr = bmp_row_groups(W);
  const uint32_t grp = it.item0 + threadIdx.x;
  if (grp >= gpr * H) return;
  const uint32_t y = grp / gpr, gx = grp - y * gpr, x0 = 4u * gx;
  const uint32_t n = W - x0 < 4u ? W - x0 : 4u;
  // the source: the file's rows, or the index plane of an RLE stream (bottom-up, one byte per pixel)
  const uint32_t bits = g.rle ? 8u : g.bits, stride = g.rle ? W : g.stride;
  const uint64_t base = g.rle ? g.idx : g.src, end = g.rle ? g.idx + (uint64_t)W * H : g.src_end;
  const uint64_t A = base + (uint64_t)bmp_src_row(y, H, g.rle ? 0u : g.top_down) * stride + bmp_group_off(x0, bits);
  const uint64_t last = A + bmp_group_bytes(x0, n, bits);
  const uint64_t A0 = A & ~3ull;
  const uint32_t sh = (uint32_t)(A & 3ull) * 8u;
  uint32_t r[5], v[4];
#pragma unroll
  for (uint32_t k = 0; k < 5; k++) r[k] = A0 + 4u * k < last ? bmp_ld32(A0 + 4u * k, end) : 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) v[k] = __funnelshift_r(r[k], r[k + 1], sh);
  uint32_t px[4] = {0u, 0u, 0u, 0u};  // R | G << 8 | B << 16 | A << 24
  bool past = false;
  if (bits <= 8u) {
    const DG_GLOBAL uint32_t *pal = gp<const uint32_t>(g.pal);
#pragma unroll
    for (uint32_t t = 0; t < 4; t++)
      if (t < n) {
        const uint32_t i = bmp_index_at(v, x0, t, bits);
        if (i < g.npal)
          px[t] = pal[i];
        else
          past = true;
      }
  } else if (bits == 24u) {
#pragma unroll
    for (uint32_t t = 0; t < 4; t++)
      px[t] = bmp_byte(v, 3u * t + 2u) | (bmp_byte(v, 3u * t + 1u) << 8) | (bmp_byte(v, 3u * t) << 16) | 0xFF000000u;
  } else {
    const uint32_t pr = g.pos & 255u, pg = (g.pos >> 8) & 255u, pb = (g.pos >> 16) & 255u, pa = g.pos >> 24;
#pragma unroll
    for (uint32_t t = 0; t < 4; t++) {
      const uint32_t d = v[t];
      const uint32_t al = pa < 4u ? (d >> (8u * pa)) & 255u : 255u;
      px[t] = ((d >> (8u * pr)) & 255u) | (((d >> (8u * pg)) & 255u) << 8) | (((d >> (8u * pb)) & 255u) << 16) | (al << 24);
    }
  }
  if (past) {
    im.bmp.fail = kBmpFailPalette;
    im.status = 1;  // DG_ERR_UNSUPPORTED
  }
  DG_GLOBAL uint8_t *row = gp<uint8_t>(im.pix) + (size_t)y * im.pix_stride;
  if (im.dec_c == 4u) {
    DG_GLOBAL uint32_t *o = (DG_GLOBAL uint32_t *)(row + 16u * (size_t)gx);
    if (n == 4u) {
      *(DG_GLOBAL u32x4 *)o = u32x4{px[0], px[1], px[2], px[3]};
    } else {
#pragma unroll
      for (uint32_t t = 0; t < 3; t++)
        if (t < n) o[t] = px[t];
    }
  } else {
    DG_GLOBAL uint8_t *o = row + 12u * (size_t)gx;
    if (n == 4u) {  // 12 bytes on a dword boundary (pix_stride is a multiple of 16)
      DG_GLOBAL uint32_t *ow = (DG_GLOBAL uint32_t *)o;
      ow[0] = (px[0] & 0xFFFFFFu) | (px[1] << 24);
      ow[1] = ((px[1] >> 8) & 0xFFFFu) | (px[2] << 16);
      ow[2] = ((px[2] >> 16) & 0xFFu) | (px[3] << 8);
    } else {
#pragma unroll
      for (uint32_t t = 0; t < 3; t++)
        if (t < n) {
          o[3u * t] = (uint8_t)px[t];
          o[3u * t + 1u] = (uint8_t)(px[t] >> 8);
          o[3u * t + 2u] = (uint8_t)(px[t] >> 16);
        }
    }
  }
}

// ------------------------------------------------------------ launchers

void launch_bmp_rle(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_bmp_rle, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_bmp_expand(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_bmp_expand, dim3(nwg), dim3(64), 0, st, imgs, list);
}

}  // namespace dg
