// dg_destuff.h — the per-lane routines of the destuff count and write passes
// (k_destuff_count, k_destuff_write in kernels.hip), shared with the CPU form
// in tests/native/destuff_emu.cpp.
//
// A wave owns one raw chunk of kDestuffChunk bytes, a lane kDsLane = 64
// consecutive bytes of it.  The lane reads the 72-byte dword-aligned window
// around its span and the two bytes beside it (four 16-byte loads and one of
// 8), shifts it by the scan pointer's misalignment (ds_window; a span whose
// window would leave the scan takes byte loads, ds_span_bytes) and classifies
// the 64 bytes four at a time with one flag per byte (ds_keep_flags64,
// ds_marker_flags64).  The write pass removes the dropped bytes in registers
// (ds_compact64) and puts the kept ones at the lane's place in a staging
// buffer on the output's dword grid (ds_put_bytes): whole dwords where the
// lane owns them, single bytes only in the dwords it shares with its
// neighbours.  The span that holds the scan's last bytes (fewer than 64
// valid ones) goes byte by byte instead (ds_classify64, ds_emit64).
#pragma once
#include "dg_entropy.h"

namespace dg {

constexpr uint32_t kDsLane = 64;  // raw bytes per lane
static_assert(kDsLane * 64 == kDestuffChunk, "a wave owns a chunk");
// The staging buffer of a workgroup holds its output on the dword grid of
// the logical stream (up to 3 bytes of the first word belong to the
// workgroup before it), one spare dword after every 32: a lane's dwords lie
// 16 apart from its neighbour's, the store phase reads words a subsequence
// apart, and without the spare both would meet on a few banks.
constexpr uint32_t kDsStageWords = kDsWgChunks * kDestuffChunk / 4 + 1;
constexpr uint32_t kDsStageAlloc = kDsStageWords + (kDsStageWords >> 5) + 1;

DG_HD uint32_t ds_pad(uint32_t d) { return d + (d >> 5); }

DG_HD bool ds_has_ff(uint32_t x) {
  const uint32_t v = ~x;
  return ((v - 0x01010101u) & ~v & 0x80808080u) != 0u;
}

// bytes b.. of the 8 bytes lo (low), hi; b = 0..4
DG_HD uint32_t ds_funnel(uint32_t lo, uint32_t hi, uint32_t b) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * b));
}

// The 72 bytes from the dword that holds byte i0 - 1 of a scan of n bytes lie
// inside the scan (and hold bytes i0 - 1 .. i0 + 64).
DG_HD bool ds_window_in_scan(uint32_t i0, uint32_t n) { return i0 >= 4u && i0 + 72u <= n; }

// x = the 18 dwords from the dword that holds the byte before the span, which
// is byte sh = 0..3 of x[0].  r = the span's 16 dwords, prev / next = the
// bytes before and after it.
DG_HD void ds_window(const uint32_t x[18], uint32_t sh, uint32_t r[16], uint32_t *prev, uint32_t *next) {
#pragma unroll
  for (int m = 0; m < 16; m++) r[m] = ds_funnel(x[m], x[m + 1], sh + 1u);
  *prev = (x[0] >> (8u * sh)) & 0xFFu;
  *next = ds_funnel(x[16], x[17], sh + 1u) & 0xFFu;
}

// The same for a span at the head or the tail of the scan, where the dword
// window would leave the scan: byte loads, bytes past the scan read as 0.
// p = the span's first byte, nv <= 64 its valid bytes, has_prev / has_next:
// the scan holds p[-1] / p[64].
DG_HD void ds_span_bytes(const DG_GLOBAL uint8_t *p, uint32_t nv, bool has_prev, bool has_next, uint32_t r[16],
                         uint32_t *prev, uint32_t *next) {
#pragma unroll
  for (uint32_t m = 0; m < 16; m++) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
      if (4u * m + j < nv) v |= (uint32_t)p[4u * m + j] << (8u * j);
    r[m] = v;
  }
  *prev = has_prev ? p[-1] : 0u;
  *next = has_next ? p[64] : 0u;
}

// Keep / marker masks of a span of nv <= 64 valid bytes (bit j = byte j).
// prev = the byte before the span (0 at the start of the scan), next = the
// byte after its last valid byte (0xD9 at the end of the scan).
DG_HD void ds_classify64(const uint32_t r[16], uint32_t prev, uint32_t next, uint32_t nv, uint64_t *km,
                         uint64_t *mm) {
  uint64_t k = 0, m = 0;
  uint32_t p = prev;
#pragma unroll
  for (uint32_t g = 0; g < 4; g++) {
    const uint32_t base = 16u * g;
    if (base < nv) {
      if (base + 16u <= nv && p != 0xFFu && !ds_has_ff(r[4 * g]) && !ds_has_ff(r[4 * g + 1]) &&
          !ds_has_ff(r[4 * g + 2]) && !ds_has_ff(r[4 * g + 3])) {
        k |= 0xFFFFull << base;
      } else {
        uint32_t kk = 0, mk = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
          const uint32_t i = base + j;
          const uint32_t cur = (r[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
          const uint32_t fol = i < 63u ? (r[(i + 1u) >> 2] >> (8u * ((i + 1u) & 3u))) & 0xFFu : next;
          const uint32_t nx = i + 1u < nv ? fol : next;
          uint32_t mark;
          const uint32_t keep = destuff_keep(p, cur, nx, false, &mark);
          if (i < nv) {
            kk |= keep << j;
            mk |= mark << j;
          }
          p = cur;
        }
        k |= (uint64_t)kk << base;
        m |= (uint64_t)mk << base;
      }
    }
    p = r[4 * g + 3] >> 24;
  }
  *km = k;
  *mm = m;
}

DG_HD void ds_put_byte(uint32_t *st, uint32_t pos, uint32_t v) {
  ((uint8_t *)st)[ds_pad(pos >> 2) * 4u + (pos & 3u)] = (uint8_t)v;
}
DG_HD uint32_t ds_get_byte(const uint32_t *st, uint32_t pos) {
  return ((const uint8_t *)st)[ds_pad(pos >> 2) * 4u + (pos & 3u)];
}

// ---- a whole span (64 valid bytes) four bytes at a time
// The lanes of a wave diverge wherever the data decides a branch, and a wave
// of 64 lanes holds an 0xFF byte somewhere in nearly every group of 16, so
// per-byte work behind a test is done by every wave.  A whole span is
// therefore classified without branches, with one flag (0x80) per byte.

DG_HD uint32_t ds_popc32(uint32_t v) {
#if defined(DG_DEVICE)
  return (uint32_t)__popc(v);
#else
  return (uint32_t)__builtin_popcount(v);
#endif
}
DG_HD uint32_t ds_top_bit(uint32_t v) {  // index of the highest set bit, v != 0
#if defined(DG_DEVICE)
  return 31u - (uint32_t)__clz((int)v);
#else
  return 31u - (uint32_t)__builtin_clz(v);
#endif
}

// 0x80 in every byte of v that is 0 (exact: no borrow between bytes)
DG_HD uint32_t ds_zero_bytes(uint32_t v) { return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu); }

// K[m]: 0x80 in every kept byte of r[m].  Returns nonzero if an 0xFF byte is
// followed by a byte other than 0 (a fill byte or a marker: ds_marker_flags64).
DG_HD uint32_t ds_keep_flags64(const uint32_t r[16], uint32_t prev, uint32_t next, uint32_t K[16]) {
  uint32_t fprev = prev == 0xFFu ? 0x80000000u : 0u, any = 0;
#pragma unroll
  for (int m = 0; m < 16; m++) {
    const uint32_t y = ds_funnel(r[m], m < 15 ? r[m + 1] : next, 1);  // the byte after each byte
    const uint32_t f = ds_zero_bytes(~r[m]);                          // 0xFF bytes
    const uint32_t fp = ds_funnel(fprev, f, 3);                       // bytes after an 0xFF byte
    const uint32_t z = ds_zero_bytes(y);
    K[m] = ((f | fp) ^ 0x80808080u) | (f & z);
    any |= f & ~z;
    fprev = f;
  }
  return any;
}

// M[m]: 0x80 in every byte of r[m] that is the FF of an RST marker
DG_HD void ds_marker_flags64(const uint32_t r[16], uint32_t next, uint32_t M[16]) {
#pragma unroll
  for (int m = 0; m < 16; m++) {
    const uint32_t y = ds_funnel(r[m], m < 15 ? r[m + 1] : next, 1);
    M[m] = ds_zero_bytes(~r[m]) & ds_zero_bytes((y & 0xF8F8F8F8u) ^ 0xD0D0D0D0u);
  }
}

DG_HD uint32_t ds_count_flags64(const uint32_t F[16]) {
  uint32_t n = 0;
#pragma unroll
  for (int m = 0; m < 16; m++) n += ds_popc32(F[m]);
  return n;
}

// mark(p) for every marker of the span, p = the staging position of the next kept byte
template <class F>
DG_HD void ds_mark64(uint32_t pos, const uint32_t K[16], const uint32_t M[16], F &mark) {
#pragma unroll
  for (int m = 0; m < 16; m++) {
    if (M[m]) {
#pragma unroll
      for (uint32_t b = 0; b < 4; b++)
        if ((M[m] >> (8u * b + 7u)) & 1u) mark(pos + ds_popc32(K[m] & ((1u << (8u * b)) - 1u)));
    }
    pos += ds_popc32(K[m]);
  }
}

// Remove the bytes of r that K does not keep, from the last one down (the
// bytes below a removed byte, and their flags, stay where they are); the
// kept bytes end up in r's first bytes, in order.
DG_HD void ds_compact64(uint32_t r[16], const uint32_t K[16]) {
#pragma unroll
  for (int m = 15; m >= 0; m--) {
    uint32_t d = ~K[m] & 0x80808080u;
    while (d) {
      const uint32_t b8 = ds_top_bit(d) & ~7u;  // 8 * the byte's index
      d &= ~(0x80u << b8);
      const uint32_t low = (1u << b8) - 1u;
      r[m] = (r[m] & low) | (ds_funnel(r[m], m < 15 ? r[m + 1] : 0u, 1) & ~low);
#pragma unroll
      for (int n = m + 1; n < 16; n++) r[n] = ds_funnel(r[n], n < 15 ? r[n + 1] : 0u, 1);
    }
  }
}

// The first k <= 64 bytes of c to staging byte position pos: whole dwords
// where they fill one, single bytes in the edge dwords a neighbour shares
DG_HD void ds_put_bytes(uint32_t *st, uint32_t pos, const uint32_t c[16], uint32_t k) {
  const uint32_t sh = pos & 3u, d0 = pos >> 2;
  const uint32_t e = sh + k, mt = e >> 2, nb = e & 3u;  // dword d0 + mt holds the last nb bytes
  uint32_t tail = 0;
#pragma unroll
  for (int m = 0; m <= 16; m++) {
    // staging dword d0 + m = bytes 4 m - sh .. of c
    const uint32_t o = ds_funnel(m > 0 ? c[m - 1] : 0u, m < 16 ? c[m] : 0u, 4u - sh);
    if ((uint32_t)m < mt && (m > 0 || sh == 0u)) st[ds_pad(d0 + m)] = o;
    if ((uint32_t)m == mt) tail = o;
  }
  if (sh) {
#pragma unroll
    for (uint32_t j = 0; j < 3; j++)
      if (j < 4u - sh && j < k) ds_put_byte(st, pos + j, c[0] >> (8u * j));
  }
  if (nb && (mt > 0u || sh == 0u)) {
#pragma unroll
    for (uint32_t j = 0; j < 3; j++)
      if (j < nb) ds_put_byte(st, 4u * (d0 + mt) + j, tail >> (8u * j));
  }
}

DG_HD uint32_t ds_popc64(uint64_t v) {
#if defined(DG_DEVICE)
  return (uint32_t)__popcll(v);
#else
  return (uint32_t)__builtin_popcountll(v);
#endif
}

// 4 N kept bytes r[C0 .. C0 + N) to staging byte position pos: the dwords the bytes
// fill whole as dwords, the (at most two) shared edge dwords byte by byte
template <int N, int C0>
DG_HD void ds_put_words(uint32_t *st, uint32_t pos, const uint32_t *r) {
  uint32_t c[N];
#pragma unroll
  for (int m = 0; m < N; m++) c[m] = r[C0 + m];
  const uint32_t sh = pos & 3u, d0 = pos >> 2;
  if (sh == 0u) {
#pragma unroll
    for (int m = 0; m < N; m++) st[ds_pad(d0 + m)] = c[m];
    return;
  }
#pragma unroll
  for (uint32_t j = 0; j < 3; j++)
    if (j < 4u - sh) ds_put_byte(st, pos + j, c[0] >> (8u * j));
#pragma unroll
  for (int m = 1; m < N; m++) st[ds_pad(d0 + m)] = ds_funnel(c[m - 1], c[m], 4u - sh);
#pragma unroll
  for (uint32_t j = 0; j < 3; j++)
    if (j < sh) ds_put_byte(st, 4u * (d0 + N) + j, c[N - 1] >> (8u * (4u - sh + j)));
}

// group G of 16 bytes of a span; returns the position after it
template <int G, class F>
DG_HD uint32_t ds_emit16(uint32_t *st, uint32_t pos, const uint32_t r[16], uint64_t km, uint64_t mm, F &mark) {
  const uint32_t kk = (uint32_t)(km >> (16 * G)) & 0xFFFFu, mk = (uint32_t)(mm >> (16 * G)) & 0xFFFFu;
  if (kk == 0xFFFFu) {
    ds_put_words<4, 4 * G>(st, pos, r);
    return pos + 16u;
  }
#pragma unroll
  for (uint32_t j = 0; j < 16; j++) {
    const uint32_t i = 16u * G + j;
    if ((mk >> j) & 1u) mark(pos);
    if ((kk >> j) & 1u) ds_put_byte(st, pos++, (r[i >> 2] >> (8u * (i & 3u))) & 0xFFu);
  }
  return pos;
}

// The span's kept bytes to staging byte position pos.  mark(p) is called for
// every RST marker with the staging position of the next kept byte.
template <class F>
DG_HD void ds_emit64(uint32_t *st, uint32_t pos, const uint32_t r[16], uint64_t km, uint64_t mm, F mark) {
  if (km == ~0ull) {
    ds_put_words<16, 0>(st, pos, r);
    return;
  }
  pos = ds_emit16<0>(st, pos, r, km, mm, mark);
  pos = ds_emit16<1>(st, pos, r, km, mm, mark);
  pos = ds_emit16<2>(st, pos, r, km, mm, mark);
  ds_emit16<3>(st, pos, r, km, mm, mark);
}

}  // namespace dg
