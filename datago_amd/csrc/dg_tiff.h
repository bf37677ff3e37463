// dg_tiff.h — the per-lane routines of the TIFF decode (k_tiff_lzw, k_tiff_packbits and
// k_tiff_expand, dg_tiff.hip), shared with the CPU form in tests/native/tiff_emu.cpp.
//
// LZW.  The scheme is dg_gif.h's: an entry is the (position, length) of its first
// occurrence in the segment's own output, a wave takes 64 codes per step, and a lane
// knows the table size its code is read with in closed form (gif_lane_nf, gif_creator,
// gif_code_bad and gif_copy_index coincide and are used as they are).  What TIFF
// changes is the code stream: codes are packed MSB-first (tiff_code), clear is 256, end
// is 257, the first free code 258, and the width is the bit length of entries + 1
// (tiff_width): it grows one code earlier than in GIF.  A full table keeps 12 bits.
//
// PackBits.  A header byte n is a literal run of n + 1 bytes (0 .. 127), a repeat of
// the next byte 257 - n times (129 .. 255) or nothing (128).  Every lane reads its byte
// as a header; which lanes are headers is settled by hopping from header to header.
//
// Expand.  A lane holds four pixels as four dwords, sample s of a pixel in byte s
// (tiff_px); predictor 2 is a prefix sum per byte lane, modulo 256 (tiff_badd), and
// tiff_pack turns the four pixels back into the 4 x spp bytes of the row.  The 16-bit form
// (k_tiff_expand16; tests/native/tiff16_emu.cpp on the CPU) is the tiff16_* routines below, the
// 1-bit form (k_tiff_expand1; tests/native/tiff_g4_emu.cpp) is tiff1_spread.
#pragma once
#include "dg_gif.h"
#include "dg_types.h"

namespace dg {

constexpr uint32_t kTiffClear = 256, kTiffEnd = 257, kTiffFirst = 258;
constexpr uint32_t kTiffWinBytes = 256;       // source window of k_tiff_lzw: one dword per lane, in registers
constexpr uint32_t kTiffStepBytes = 96 + 4;   // most bytes one step's codes touch: 64 x 12 bits, three bytes from the last offset
constexpr uint32_t kTiffLdsOut = 65536;       // a segment that decodes to no more than this stays in LDS while it is read back
constexpr uint32_t kTiffFullCodes = 1000;     // data codes a full table may serve before the segment is refused
constexpr uint32_t kTiffShort = 8;            // strings / runs up to this length are copied by their own lane
constexpr uint32_t kTiffExpandPieces = 4;     // row pieces per work item of k_tiff_expand

// Bits of a code read while the table holds nf entries (clear and end code included).
DG_HD uint32_t tiff_width(uint32_t nf) {
  const uint32_t w = 32u - (uint32_t)__builtin_clz(nf + 1u);
  return w > 12u ? 12u : w;
}

// The w-bit code at bit offset off of an MSB-first stream, from the three bytes b0 b1 b2 at byte off / 8.
DG_HD uint32_t tiff_code(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t off, uint32_t w) {
  const uint32_t v = (b0 << 16) | (b1 << 8) | b2;
  return (v >> (24u - (off & 7u) - w)) & ((1u << w) - 1u);
}

// ---- PackBits: bytes a header writes, and bytes it takes from the stream (itself included)
DG_HD uint32_t tiff_pb_out(uint32_t n) { return n < 128u ? n + 1u : n == 128u ? 0u : 257u - n; }
DG_HD uint32_t tiff_pb_size(uint32_t n) { return n < 128u ? n + 2u : n == 128u ? 1u : 2u; }

// ---- expand
// Byte-wise a + b modulo 256 on four packed bytes.
DG_HD uint32_t tiff_badd(uint32_t a, uint32_t b) {
  return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
}
// Pixel t (< 4) of the 4 x spp bytes in v: its samples in bytes 0 .. spp - 1.
DG_HD uint32_t tiff_px(const uint32_t v[4], uint32_t t, uint32_t spp) {
  if (spp == 4u) return v[t];
  if (spp == 1u) return (v[0] >> (8u * t)) & 0xFFu;
  if (spp == 2u) return (v[t >> 1] >> (16u * (t & 1u))) & 0xFFFFu;
  return t == 0u ? v[0] & 0xFFFFFFu : t == 1u ? (v[0] >> 24) | ((v[1] & 0xFFFFu) << 8) : t == 2u ? (v[1] >> 16) | ((v[2] & 0xFFu) << 16) : v[2] >> 8;
}
// Dword k (< spp) of the row bytes of the four pixels p.
DG_HD uint32_t tiff_pack(const uint32_t p[4], uint32_t k, uint32_t spp) {
  if (spp == 4u) return p[k];
  if (spp == 1u) return p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
  if (spp == 2u) return p[2u * k] | (p[2u * k + 1u] << 16);
  return k == 0u ? p[0] | (p[1] << 24) : k == 1u ? (p[1] >> 8) | (p[2] << 16) : (p[2] >> 16) | (p[3] << 8);
}
// ---- expand, 16-bit samples (k_tiff_expand16, option "tiff16")
// A lane's four pixels are 4 x spp samples in 2 x spp dwords, two samples to a dword in row order (sample j
// in half j & 1 of dword j >> 1).  For predictor 2 a pixel's samples are regrouped into ceil(spp / 2) dwords of
// its own (tiff16_px: sample c in half c & 1 of dword c >> 1, the spare half of an odd spp zero), so the sum
// with stride spp is one packed add per pixel dword, modulo 65536 per half (tiff16_hadd); tiff16_pack goes back.
// Both halves of v with their two bytes exchanged: an MM file's samples, two at a time.
DG_HD uint32_t tiff16_swap(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(v, v, 0x02030001u);
#else
  return ((v & 0x00FF00FFu) << 8) | ((v >> 8) & 0x00FF00FFu);
#endif
}
// Half-wise a + b modulo 65536 on two packed samples.
DG_HD uint32_t tiff16_hadd(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));  // v_pk_add_u16
#else
  return ((a & 0x7FFF7FFFu) + (b & 0x7FFF7FFFu)) ^ ((a ^ b) & 0x80008000u);
#endif
}
// Sample j of samples packed two to a dword.
DG_HD uint32_t tiff16_at(const uint32_t *v, uint32_t j) { return (v[j >> 1] >> (16u * (j & 1u))) & 0xFFFFu; }
// Dword k (< ceil(spp / 2)) of pixel t (< 4) of the row dwords v.
DG_HD uint32_t tiff16_px(const uint32_t *v, uint32_t t, uint32_t k, uint32_t spp) {
  const uint32_t j = t * spp + 2u * k;
  return tiff16_at(v, j) | (2u * k + 1u < spp ? tiff16_at(v, j + 1u) << 16 : 0u);
}
// Dword m (< 2 spp) of the row from the four pixels' dwords p[t][k].
DG_HD uint32_t tiff16_pack(const uint32_t p[4][2], uint32_t m, uint32_t spp) {
  const uint32_t j0 = 2u * m, j1 = j0 + 1u;
  return tiff16_at(p[j0 / spp], j0 % spp) | (tiff16_at(p[j1 / spp], j1 % spp) << 16);
}
// ---- expand, 1-bit samples (k_tiff_expand1, option "tiff_bilevel")
// Four pixels, the first in bit 3 of n, as four bytes of 0 / 255 in memory order: one multiply puts bit 3 - k
// into byte k, one more turns the 1s into 255s.
DG_HD uint32_t tiff1_spread(uint32_t n) { return ((((n & 15u) * 0x08040201u) & 0x08080808u) >> 3) * 0xFFu; }

// Row piece pc of an image (a piece is one row of one segment column, pieces run row by row): its image
// row, its segment, the byte offset of its first pixel inside the segment, its first pixel in the row and
// its pixel count (an edge tile's padding columns are dropped).  spp: bytes per pixel (16-bit samples: 2 x spp).
struct TiffPiece {
  uint32_t y, seg, off, px0, npx;
};
DG_HD TiffPiece tiff_piece(uint32_t pc, uint32_t width, uint32_t spp, uint32_t seg_w, uint32_t seg_h, uint32_t across) {
  const uint32_t y = pc / across, tx = pc - y * across, sy = y / seg_h, px0 = tx * seg_w;
  return TiffPiece{y, sy * across + tx, (y - sy * seg_h) * seg_w * spp, px0, width - px0 < seg_w ? width - px0 : seg_w};
}

}  // namespace dg
