// dg_bmp.h — the per-lane routines of the BMP decode (k_bmp_rle and k_bmp_expand,
// dg_bmp.hip), shared with the CPU form in tests/native/bmp_emu.cpp.
//
// RLE8 / RLE4 (BI_RLE8 on 8 bits, BI_RLE4 on 4 bits).  Every command is two
// bytes and an absolute block's data is padded to a 16-bit boundary relative to
// the start of the stream, so the stream is a sequence of two-byte units and a
// command can only start on one.  A wave takes 64 units per step.  Each lane
// classifies its unit as if a command started there (bmp_unit); only the
// units inside an absolute block are not commands, so which lanes are command
// starts is settled by hopping over the absolute blocks of the window alone.
// A data unit of an absolute block yields 2 (RLE8) or 4 (RLE4) pixels, the
// block's last unit what is left (bmp_data_count); a run yields its count at
// its own lane.  A prefix sum gives every lane its output position.
//
// Only streams that write every pixel exactly once in row order decode: a row
// is filled by runs and absolute blocks that end exactly at its end and is then
// closed by end-of-line (the last one by anything: the decode stops with the
// last pixel).  bmp_cmd_fail names what else a command can be; the first such
// command in stream order, or the data's end, ends the decode as
// DG_ERR_UNSUPPORTED (the CPU decoders disagree on every one of them).
#pragma once
#include "dg_types.h"

namespace dg {

constexpr uint32_t kBmpStepUnits = 64;   // two-byte units per step: one per lane
constexpr uint32_t kBmpWinBytes = 2048;  // source window a wave keeps in LDS
constexpr uint32_t kBmpShort = 8;        // runs up to this length are written by their own lane

enum BmpKind : uint32_t { kBmpRun = 0, kBmpAbs = 1, kBmpEol = 2, kBmpEob = 3, kBmpDelta = 4 };

// What the unit (a, b) is when a command starts on it.
DG_HD uint32_t bmp_unit_kind(uint32_t a, uint32_t b) {
  return a ? kBmpRun : b == 0u ? kBmpEol : b == 1u ? kBmpEob : b == 2u ? kBmpDelta : kBmpAbs;
}
// Pixels the command writes (a run's count, an absolute block's length).
DG_HD uint32_t bmp_unit_pixels(uint32_t a, uint32_t b) { return a ? a : b >= 3u ? b : 0u; }
// Pixels one data unit of an absolute block holds.
DG_HD uint32_t bmp_ppu(uint32_t rle4) { return rle4 ? 4u : 2u; }
// Data units behind an absolute command of n pixels: n bytes (RLE8) or ceil(n / 2) bytes (RLE4),
// padded to a whole unit.
DG_HD uint32_t bmp_abs_units(uint32_t n, uint32_t rle4) { return rle4 ? (n + 3u) / 4u : (n + 1u) / 2u; }
// Pixels of the data unit k of a block that has `left` pixels at its unit 0.
DG_HD uint32_t bmp_data_count(uint32_t left, uint32_t k, uint32_t rle4) {
  const uint32_t p = bmp_ppu(rle4), done = k * p;
  return done >= left ? 0u : left - done < p ? left - done : p;
}
// Pixel t of the data unit (a, b).
DG_HD uint32_t bmp_data_pixel(uint32_t a, uint32_t b, uint32_t t, uint32_t rle4) {
  if (!rle4) return t ? b : a;
  const uint32_t v = t < 2u ? a : b;
  return (t & 1u) ? v & 15u : v >> 4;
}
// Pixel t of a run whose value byte is b: RLE4 alternates the high and the low nibble.
DG_HD uint32_t bmp_run_pixel(uint32_t b, uint32_t t, uint32_t rle4) { return !rle4 ? b : (t & 1u) ? b & 15u : b >> 4; }

// A command that starts with o pixels written, of a w pixels wide bitmap, the command before it
// (prev_eol: it was an end-of-line): 0 when it keeps the row order, else the kBmpFail* it is.  (An
// end-of-bitmap is only ever looked at with pixels still unwritten: the decode stops with the last.)
DG_HD uint32_t bmp_cmd_fail(uint32_t kind, uint32_t q, uint32_t o, uint32_t w, bool prev_eol) {
  const uint32_t r = o % w;
  if (kind == kBmpRun || kind == kBmpAbs) {
    if (r == 0u && o != 0u && !prev_eol) return kBmpFailRow;  // the row before is full and not closed
    return r + q > w ? kBmpFailRow : 0u;
  }
  if (kind == kBmpEol) return (r == 0u && o != 0u && !prev_eol) ? 0u : kBmpFailDelta;
  return kBmpFailDelta;
}

// The uniform state of a decode between steps.
struct BmpRle {
  uint32_t pos;        // byte offset of the next unit in the stream (even)
  uint32_t o;          // pixels written
  uint32_t prev_eol;   // the last command was an end-of-line
  uint32_t data_units; // data units of an absolute block still to come ...
  uint32_t data_left;  // ... and the pixels they hold
};

// ---- k_bmp_expand: a lane takes 4 pixels of a row (fewer at the row's end)

// File row that holds image row y.
DG_HD uint32_t bmp_src_row(uint32_t y, uint32_t h, uint32_t top_down) { return top_down ? y : h - 1u - y; }
// Groups of 4 pixels per row.
DG_HD uint32_t bmp_row_groups(uint32_t w) { return (w + 3u) / 4u; }
// Byte offset inside the row, and count, of the source bytes of the group at pixel x0 (a multiple of 4)
// with n pixels.
DG_HD uint32_t bmp_group_off(uint32_t x0, uint32_t bits) { return (uint32_t)(((uint64_t)x0 * bits) >> 3); }
DG_HD uint32_t bmp_group_bytes(uint32_t x0, uint32_t n, uint32_t bits) {
  return (uint32_t)((((uint64_t)(x0 + n) * bits + 7u) >> 3) - (((uint64_t)x0 * bits) >> 3));
}
// Byte k (< 16) of four little-endian dwords.
DG_HD uint32_t bmp_byte(const uint32_t v[4], uint32_t k) {
  const uint32_t d = k < 4u ? v[0] : k < 8u ? v[1] : k < 12u ? v[2] : v[3];
  return (d >> (8u * (k & 3u))) & 255u;
}
// Index of pixel t of a 1 / 4 / 8-bit group from its source bytes (x0 is a multiple of 4, so a
// 1-bit group lies in one half of byte 0, MSB first; a 4-bit one in bytes 0 and 1).
DG_HD uint32_t bmp_index_at(const uint32_t v[4], uint32_t x0, uint32_t t, uint32_t bits) {
  if (bits == 8u) return bmp_byte(v, t);
  if (bits == 4u) return (bmp_byte(v, t >> 1) >> ((t & 1u) ? 0u : 4u)) & 15u;
  return (v[0] >> (7u - ((x0 & 4u) + t))) & 1u;
}

}  // namespace dg
