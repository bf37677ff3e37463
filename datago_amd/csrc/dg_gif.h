// dg_gif.h — the per-lane routines of the GIF LZW decode (k_gif_lzw, dg_gif.hip)
// and of the placement on the screen (k_gif_expand), shared with the CPU form in
// tests/native/gif_emu.cpp.
//
// What they restate: weezl's LSB-first GIF decoder as gif 0.13 drives it.  A
// table entry is not a prefix chain but the (position, length) of its first
// occurrence in the indices already written: the entry added on reading code
// j is string(code j-1) + first byte of string(code j), and those bytes lie
// contiguously in the output from where string(code j-1) was written.  Decoding
// a code is then an LZ77-style copy, and KwKwK (the code that is being created)
// the overlapping copy whose last byte equals its first.
//
// A wave takes 64 codes per step.  With nf entries in the table a code is
// gif_width(nf) bits wide, and nf is a closed-form function of the code count
// since the last clear (gif_lane_nf), so lane j knows its width and, after a
// prefix sum, its bit offset without decoding what comes before.  The step is
// cut at the first clear / end code, at the first bad code and where the data
// ends.  Lengths of entries created inside the step come from the lanes that
// created them (gif_creator); prefix sums give the output positions.
#pragma once
#include "dg_types.h"

namespace dg {

constexpr uint32_t kGifMaxCodes = 4096;   // 12-bit codes
constexpr uint32_t kGifWinBytes = 2048;   // source window a wave keeps in LDS
constexpr uint32_t kGifStepBits = 64 * 12;  // most bits one step reads
constexpr uint32_t kGifShort = 8;         // strings up to this length are copied by their own lane

// Bits of a code read while the table holds nf entries (clear and end code
// included): the width grows when the next free code reaches 2^width, up to 12,
// and stays 12 while the table is full (deferred clear).
DG_HD uint32_t gif_width(uint32_t nf, uint32_t w0) {
  uint32_t w = 32u - (uint32_t)__builtin_clz(nf | 1u);
  w = w < w0 ? w0 : w;
  return w > 12u ? 12u : w;
}

// Entries in the table when code j of a step is read: nf0 at the step's start;
// every code adds one except the first after a clear (a = 1: code 0 has no
// predecessor), until the table is full.
DG_HD uint32_t gif_lane_nf(uint32_t nf0, uint32_t a, uint32_t j) {
  const uint32_t n = nf0 + (j > a ? j - a : 0u);
  return n > kGifMaxCodes ? kGifMaxCodes : n;
}

// Code c read with nfj entries by lane j: above the next free code, or the
// next free code where no predecessor exists (straight after a clear).
DG_HD bool gif_code_bad(uint32_t c, uint32_t nfj, uint32_t j, uint32_t a) {
  return c > nfj || (c == nfj && j < a);
}

// The lane of the step that creates entry c >= nf0 (c <= the reading lane's nf).
DG_HD uint32_t gif_creator(uint32_t c, uint32_t nf0, uint32_t a) { return c - nf0 + a; }

// Source byte of code byte k: through the sub-block chain (a length byte in
// front of every 255 data bytes) or in the gathered copy.
DG_HD uint32_t gif_src_index(uint32_t k, uint32_t blocked) { return blocked ? 1u + k + k / 255u : k; }

// Byte t of a string of length L copied from its source: a KwKwK string's
// last byte is its first (its source is one byte shorter than the string).
DG_HD uint32_t gif_copy_index(uint32_t t, uint32_t L, bool kwkwk) { return (kwkwk && t + 1u == L) ? 0u : t; }

// Row of the index plane (stream order) that holds frame row y: an interlaced
// frame's rows come as 0,8,..; 4,12,..; 2,6,..; 1,3,...
DG_HD uint32_t gif_stream_row(uint32_t y, uint32_t fh, uint32_t interlace) {
  if (!interlace) return y;
  const uint32_t n0 = (fh + 7u) / 8u, n1 = (fh + 3u) / 8u, n2 = (fh + 1u) / 4u;
  if ((y & 7u) == 0u) return y >> 3;
  if ((y & 7u) == 4u) return n0 + (y >> 3);
  if ((y & 3u) == 2u) return n0 + n1 + (y >> 2);
  return n0 + n1 + n2 + (y >> 1);
}

// The uniform state of a decode between steps.
struct GifLzw {
  uint32_t bitpos;   // next code's bit offset in the stream
  uint32_t nf;       // table entries (clear and end code included)
  uint32_t pv;       // 1: the previous code's string exists (0 straight after a clear)
  uint32_t ppos, plen;  // ... where it was written and its length
  uint32_t o;        // indices written
};

}  // namespace dg
