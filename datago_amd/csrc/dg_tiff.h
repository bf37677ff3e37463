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
// tiff_pack turns the four pixels back into the 4 x spp bytes of the row.
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
// Row piece pc of an image (a piece is one row of one segment column, pieces run row by row): its image
// row, its segment, the byte offset of its first pixel inside the segment, its first pixel in the row and
// its pixel count (an edge tile's padding columns are dropped).
struct TiffPiece {
  uint32_t y, seg, off, px0, npx;
};
DG_HD TiffPiece tiff_piece(uint32_t pc, uint32_t width, uint32_t spp, uint32_t seg_w, uint32_t seg_h, uint32_t across) {
  const uint32_t y = pc / across, tx = pc - y * across, sy = y / seg_h, px0 = tx * seg_w;
  return TiffPiece{y, sy * across + tx, (y - sy * seg_h) * seg_w * spp, px0, width - px0 < seg_w ? width - px0 : seg_w};
}

}  // namespace dg
