// dg_penc16.h — the filter stage of the PNG re-encoder for 16-bit samples
// (context option "penc16"): byte order and per-byte filter arithmetic shared
// by k_penc_filter16 in dg_penc.hip and the CPU form in
// tests/native/penc16_emu.cpp.
//
// A bit-depth-16 PNG row holds every sample high byte first (PNG spec 7.2);
// the five filters (spec 9.2) run over those bytes with bpp = 2 x samples per
// pixel.  The encoder's input is native-endian uint16, tightly packed, so a
// row is 2-byte aligned and only every other row of an odd-sample-count image
// is 4-byte aligned.  The unit of work here is a QUAD: four consecutive row
// bytes = two samples, held as one dword whose byte k is row byte x + k.
//
//   p16_load_pair   samples i, i + 1 of a row as one dword (one 4-byte load
//                   where the address allows, two 2-byte loads otherwise;
//                   samples outside the row read as 0)
//   p16_be          that dword's samples turned high byte first
//   p16_quad        the quad at row byte x with its left, upper and
//                   upper-left neighbours (bpp bytes back; 0 outside the image)
//   p16_sums        |byte as int8| sums of the five filters over a quad
//   p16_apply       the quad under one filter
//   p16_best        the filter choice from the five row sums
#pragma once
#include <stdint.h>

#include "dg_types.h"

namespace dg {

#if defined(__HIP_DEVICE_COMPILE__)
#define P16_UNROLL _Pragma("unroll")
#else
#define P16_UNROLL
#endif

// ---- per byte (PNG spec 9.2, 9.4, 12.8)

DG_HD uint32_t p16_paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int32_t p = (int32_t)a + (int32_t)b - (int32_t)c;
  const int32_t da = p - (int32_t)a, db = p - (int32_t)b, dc = p - (int32_t)c;
  const int32_t pa = da < 0 ? -da : da, pb = db < 0 ? -db : db, pc = dc < 0 ? -dc : dc;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// byte x under filter f with left a, upper b, upper-left c
DG_HD uint32_t p16_filt(uint32_t f, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t pr = f == 0 ? 0u : f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) >> 1 : p16_paeth(a, b, c);
  return (x - pr) & 0xFFu;
}

DG_HD uint32_t p16_abs_i8(uint32_t v) { return v < 128u ? v : 256u - v; }  // 0x80 counts 128

// ---- byte order

// Two native-endian samples (the first in the low half) -> their four row
// bytes, the first row byte in byte 0: each half's bytes change places.
DG_HD uint32_t p16_be(uint32_t pair) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(pair, pair, 0x02030001u);  // one v_perm_b32
#else
  return ((pair & 0x00FF00FFu) << 8) | ((pair >> 8) & 0x00FF00FFu);
#endif
}

// Samples i and i + 1 of a row of n samples as one dword, sample i in the low
// half; a sample outside [0, n) is 0.  al4: sample 0 of the row sits on a
// 4-byte address, so an even i inside the row is one dword load.
typedef uint32_t __attribute__((may_alias)) p16_u32;  // a dword read of two uint16 samples
DG_HD uint32_t p16_load_pair(const DG_GLOBAL uint16_t *row, int32_t i, uint32_t n, bool al4) {
  if (i >= 0 && (uint32_t)i + 1 < n && (((uint32_t)i & 1u) == 0u) == al4)
    return *(const DG_GLOBAL p16_u32 *)(row + i);
  const uint32_t lo = (i >= 0 && (uint32_t)i < n) ? row[i] : 0u;
  const uint32_t hi = (i + 1 >= 0 && (uint32_t)(i + 1) < n) ? row[i + 1] : 0u;
  return lo | hi << 16;
}

// ---- per quad

struct P16Quad {
  uint32_t v, a, b, c;  // the row bytes x .. x + 3 and their left, upper, upper-left neighbours
};

// The quad at row byte x (a multiple of 4) of row `cur`; `up` is the row
// above or null for row 0.  n: samples per row, hs = bpp / 2: samples per
// pixel.  cur_al4 / up_al4: the row's first sample sits on a 4-byte address.
DG_HD P16Quad p16_quad(const DG_GLOBAL uint16_t *cur, const DG_GLOBAL uint16_t *up, uint32_t x, uint32_t n, uint32_t hs,
                       bool cur_al4, bool up_al4) {
  const int32_t i = (int32_t)(x >> 1), j = i - (int32_t)hs;
  P16Quad q;
  q.v = p16_be(p16_load_pair(cur, i, n, cur_al4));
  q.a = p16_be(p16_load_pair(cur, j, n, cur_al4));
  q.b = up ? p16_be(p16_load_pair(up, i, n, up_al4)) : 0u;
  q.c = up ? p16_be(p16_load_pair(up, j, n, up_al4)) : 0u;
  return q;
}

DG_HD uint32_t p16_byte(uint32_t quad, uint32_t k) { return (quad >> (8 * k)) & 0xFFu; }

// sum[f] += |byte as int8| of the quad's first nb bytes (1..4) under filter f
DG_HD void p16_sums(const P16Quad &q, uint32_t nb, uint32_t sum[5]) {
  P16_UNROLL
  for (uint32_t k = 0; k < 4; k++) {
    if (k >= nb) break;
    const uint32_t v = p16_byte(q.v, k), a = p16_byte(q.a, k), b = p16_byte(q.b, k), c = p16_byte(q.c, k);
    P16_UNROLL
    for (uint32_t f = 0; f < 5; f++) sum[f] += p16_abs_i8(p16_filt(f, v, a, b, c));
  }
}

// the quad under filter f, byte k of the result = filtered row byte x + k
DG_HD uint32_t p16_apply(uint32_t f, const P16Quad &q) {
  uint32_t r = 0;
  P16_UNROLL
  for (uint32_t k = 0; k < 4; k++)
    r |= p16_filt(f, p16_byte(q.v, k), p16_byte(q.a, k), p16_byte(q.b, k), p16_byte(q.c, k)) << (8 * k);
  return r;
}

// the smallest sum wins, a tie goes to the lower type
DG_HD uint32_t p16_best(const uint32_t sum[5]) {
  uint32_t best = 0, bs = sum[0];
  P16_UNROLL
  for (uint32_t f = 1; f < 5; f++)
    if (sum[f] < bs) {
      bs = sum[f];
      best = f;
    }
  return best;
}

}  // namespace dg
