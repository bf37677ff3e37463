// dg_tiff_g4.h — the per-lane routines of k_tiff_g4 (dg_tiff_g4.hip, option "tiff_bilevel"),
// shared with the CPU form in tests/native/tiff_g4_emu.cpp.
//
// A TIFF segment of compression 4 is one CCITT Group 4 (ITU-T T.6) stream: MSB-first bits,
// byte-aligned at the segment's start only, every row coded against the row above (the first
// against an all-white one).  A row starts white with a0 before its first pixel and ends
// where a0 reaches the width.  The mode codes:
//   pass 0001, horizontal 001, V0 1, VR1..3 011 000011 0000011, VL1..3 010 000010 0000010,
//   extension 0000001xxx (refused).
// Horizontal mode is followed by two Modified Huffman run lengths (T.4 tables 2 and 3), the
// current colour's first: zero or more make-up codes (64 .. 1728 per colour, 1792 .. 2560
// shared) and one terminating code (0 .. 63).
//
// Tokens.  A lane decodes the whole token that would start at its own bit offset (g4_token)
// from a 64-bit window: the mode in closed form from the count of leading zeros, and for
// horizontal mode both run lengths under both colour hypotheses, each run with at most one
// make-up code (3 + 25 + 25 bits at the most).  A longer chain (a run of 2,624 pixels or
// more) is flagged and decoded by the whole wave from the stream (g4_run_slow).
//
// Tables.  kG4White, kG4Black and kG4Ext list the codes of T.4 as (1 << length) | code, by
// run slot (g4_slot_run).  g4_fill spreads one code over the lookup tables in LDS:
//   white   [512]  the next 9 bits (white codes have 4 .. 9);
//   black1  [128]  the next 7 bits, for black codes that do not start with 0000 (2 .. 6 bits);
//   black2  [512]  bits 4 .. 12 behind 0000: the other black codes (7 .. 13 bits) and the
//                  shared make-up codes (11 and 12 bits), which white looks up here too.
// An entry is length << 12 | run; 0 is no code.
//
// Rows.  A row is a bitmap with pixel x in bit x & 31 of word x >> 5, black = 1, zero past
// the width.  g4_trans gives a word's changing elements, g4_span the pixels of [x0, x1) in a
// word, g4_nth the n-th set bit, g4_out the word as four bytes of the TIFF row (MSB first).
#pragma once
#include "dg_types.h"

namespace dg {

constexpr uint32_t kG4MaxWidth = 16384;               // pixels of a row: 2 KiB of LDS per row bitmap
constexpr uint32_t kG4RowWords = kG4MaxWidth / 32;
constexpr uint32_t kG4WinBytes = 256;                 // the source window: one dword per lane
constexpr uint32_t kG4StepBytes = 24;                 // source bytes a step's 64 lanes may touch: 63 + 7 + 64 bits, whole dwords
constexpr uint32_t kG4WhiteSize = 512, kG4Black1Size = 128, kG4Black2Size = 512;
constexpr uint32_t kG4TabSize = kG4WhiteSize + kG4Black1Size + kG4Black2Size;
constexpr uint32_t kG4OwnCodes = 91, kG4ExtCodes = 13, kG4Codes = 2 * kG4OwnCodes + kG4ExtCodes;

// Kinds of a token's mode.
constexpr uint32_t kG4Bad = 0, kG4V = 1, kG4H = 2, kG4P = 3;
constexpr uint32_t kG4Slow = 0x80000000u;  // a horizontal token whose make-up chain does not fit the lane's window

#if defined(DG_DEVICE)
__constant__
#endif
static const uint16_t kG4White[kG4OwnCodes] = {
    // terminating codes, runs 0 .. 63
    0b100110101, 0b1000111, 0b10111, 0b11000, 0b11011, 0b11100, 0b11110, 0b11111,
    0b110011, 0b110100, 0b100111, 0b101000, 0b1001000, 0b1000011, 0b1110100, 0b1110101,
    0b1101010, 0b1101011, 0b10100111, 0b10001100, 0b10001000, 0b10010111, 0b10000011, 0b10000100,
    0b10101000, 0b10101011, 0b10010011, 0b10100100, 0b10011000, 0b100000010, 0b100000011, 0b100011010,
    0b100011011, 0b100010010, 0b100010011, 0b100010100, 0b100010101, 0b100010110, 0b100010111, 0b100101000,
    0b100101001, 0b100101010, 0b100101011, 0b100101100, 0b100101101, 0b100000100, 0b100000101, 0b100001010,
    0b100001011, 0b101010010, 0b101010011, 0b101010100, 0b101010101, 0b100100100, 0b100100101, 0b101011000,
    0b101011001, 0b101011010, 0b101011011, 0b101001010, 0b101001011, 0b100110010, 0b100110011, 0b100110100,
    // make-up codes, runs 64 .. 1728
    0b111011, 0b110010, 0b1010111, 0b10110111, 0b100110110, 0b100110111, 0b101100100, 0b101100101,
    0b101101000, 0b101100111, 0b1011001100, 0b1011001101, 0b1011010010, 0b1011010011, 0b1011010100, 0b1011010101,
    0b1011010110, 0b1011010111, 0b1011011000, 0b1011011001, 0b1011011010, 0b1011011011, 0b1010011000, 0b1010011001,
    0b1010011010, 0b1011000, 0b1010011011};

#if defined(DG_DEVICE)
__constant__
#endif
static const uint16_t kG4Black[kG4OwnCodes] = {
    // terminating codes, runs 0 .. 63
    0b10000110111, 0b1010, 0b111, 0b110, 0b1011, 0b10011, 0b10010, 0b100011,
    0b1000101, 0b1000100, 0b10000100, 0b10000101, 0b10000111, 0b100000100, 0b100000111, 0b1000011000,
    0b10000010111, 0b10000011000, 0b10000001000, 0b100001100111, 0b100001101000, 0b100001101100, 0b100000110111, 0b100000101000,
    0b100000010111, 0b100000011000, 0b1000011001010, 0b1000011001011, 0b1000011001100, 0b1000011001101, 0b1000001101000, 0b1000001101001,
    0b1000001101010, 0b1000001101011, 0b1000011010010, 0b1000011010011, 0b1000011010100, 0b1000011010101, 0b1000011010110, 0b1000011010111,
    0b1000001101100, 0b1000001101101, 0b1000011011010, 0b1000011011011, 0b1000001010100, 0b1000001010101, 0b1000001010110, 0b1000001010111,
    0b1000001100100, 0b1000001100101, 0b1000001010010, 0b1000001010011, 0b1000000100100, 0b1000000110111, 0b1000000111000, 0b1000000100111,
    0b1000000101000, 0b1000001011000, 0b1000001011001, 0b1000000101011, 0b1000000101100, 0b1000001011010, 0b1000001100110, 0b1000001100111,
    // make-up codes, runs 64 .. 1728
    0b10000001111, 0b1000011001000, 0b1000011001001, 0b1000001011011, 0b1000000110011, 0b1000000110100, 0b1000000110101, 0b10000001101100,
    0b10000001101101, 0b10000001001010, 0b10000001001011, 0b10000001001100, 0b10000001001101, 0b10000001110010, 0b10000001110011, 0b10000001110100,
    0b10000001110101, 0b10000001110110, 0b10000001110111, 0b10000001010010, 0b10000001010011, 0b10000001010100, 0b10000001010101, 0b10000001011010,
    0b10000001011011, 0b10000001100100, 0b10000001100101};

// The make-up codes both colours share, runs 1792 .. 2560.
#if defined(DG_DEVICE)
__constant__
#endif
static const uint16_t kG4Ext[kG4ExtCodes] = {
    0b100000001000, 0b100000001100, 0b100000001101, 0b1000000010010, 0b1000000010011, 0b1000000010100, 0b1000000010101,
    0b1000000010110, 0b1000000010111, 0b1000000011100, 0b1000000011101, 0b1000000011110, 0b1000000011111};

struct G4Tabs {
  const uint16_t *white, *black1, *black2;
};
struct G4Tok {
  uint32_t mode;  // kG4* | bits of the mode code << 4 | (vertical offset + 3) << 8
  uint32_t h[2];  // horizontal mode with white [0] or black [1] first: first run | second run << 12 | bits of the
                  // whole token << 24; 0 = an invalid code, kG4Slow = a make-up chain for g4_run_slow
};

// The run of slot s: 0 .. 63 terminating, 64 .. 90 the colour's make-up codes, 91 .. 103 the shared ones.
DG_HD uint32_t g4_slot_run(uint32_t s) { return s < 64u ? s : (s - 63u) * 64u; }

// Code i (< kG4Codes: white, black, shared) into the zeroed lookup tables.  Codes are prefix-free, so no
// two fill the same entry.
DG_HD void g4_fill(uint16_t *white, uint16_t *black1, uint16_t *black2, uint32_t i) {
  const bool w = i < kG4OwnCodes, ext = i >= 2u * kG4OwnCodes;
  const uint32_t s = w ? i : ext ? i - kG4OwnCodes : i - kG4OwnCodes;  // the run slot
  const uint32_t v = w ? kG4White[i] : ext ? kG4Ext[i - 2u * kG4OwnCodes] : kG4Black[s];
  const uint32_t len = 31u - (uint32_t)__builtin_clz(v), code = v ^ (1u << len);
  const uint16_t e = (uint16_t)(len << 12 | g4_slot_run(s));
  uint16_t *t = w ? white : len < 7u ? black1 : black2;
  const uint32_t idx = w ? 9u : len < 7u ? 7u : 13u;  // (black2: the code's 0000 is its index's too)
  for (uint32_t k = 0; k < (1u << (idx - len)); k++) t[(code << (idx - len)) + k] = e;
}

// The entry of the code at the top of w (bit 63 first) read as a run of the given colour; 0 if there is none.
DG_HD uint32_t g4_lookup(const G4Tabs &t, uint64_t w, uint32_t black) {
  const uint32_t far = t.black2[(uint32_t)(w >> 51) & 511u];
  if (black) return (w >> 60) ? t.black1[(uint32_t)(w >> 57)] : far;
  const uint32_t e = t.white[(uint32_t)(w >> 55)];
  return e || (w >> 57) || (far & 4095u) < 1792u ? e : far;
}

// One run with at most one make-up code: its length and bits; false for an invalid code; *slow for a longer chain.
DG_HD bool g4_run(const G4Tabs &t, uint64_t w, uint32_t black, uint32_t *run, uint32_t *nb, bool *slow) {
  const uint32_t e = g4_lookup(t, w, black);
  if (!e) return false;
  *run = e & 4095u;
  *nb = e >> 12;
  if (*run < 64u) return true;
  const uint32_t e2 = g4_lookup(t, w << *nb, black);
  if (!e2) return false;
  if ((e2 & 4095u) >= 64u) *slow = true;
  *run += e2 & 4095u;
  *nb += e2 >> 12;
  return true;
}

// The two runs behind a horizontal mode code (w starts at the first run), `black` first.
DG_HD uint32_t g4_pair(const G4Tabs &t, uint64_t w, uint32_t black) {
  uint32_t r1 = 0, r2 = 0, n1 = 0, n2 = 0;
  bool slow = false;
  if (!g4_run(t, w, black, &r1, &n1, &slow)) return 0u;
  if (slow) return kG4Slow;
  if (!g4_run(t, w << n1, black ^ 1u, &r2, &n2, &slow)) return 0u;
  if (slow) return kG4Slow;
  return r1 | r2 << 12 | (3u + n1 + n2) << 24;
}

// The token at the top of w.
DG_HD G4Tok g4_token(const G4Tabs &t, uint64_t w) {
  const uint32_t z = w ? (uint32_t)__builtin_clzll(w) : 64u;
  const uint32_t right = (uint32_t)(w >> (62u - (z < 6u ? z : 0u))) & 1u;  // the bit after the first 1: VR, not VL
  G4Tok k = {kG4Bad, {0u, 0u}};
  if (z == 0u) k.mode = kG4V | 1u << 4 | 3u << 8;
  if (z == 1u) k.mode = kG4V | 3u << 4 | (right ? 4u : 2u) << 8;
  if (z == 2u) k.mode = kG4H | 3u << 4;
  if (z == 3u) k.mode = kG4P | 4u << 4;
  if (z == 4u) k.mode = kG4V | 6u << 4 | (right ? 5u : 1u) << 8;
  if (z == 5u) k.mode = kG4V | 7u << 4 | (right ? 6u : 0u) << 8;
  if (z == 2u) k.h[0] = g4_pair(t, w << 3, 0u), k.h[1] = g4_pair(t, w << 3, 1u);
  return k;
}

// A run of any make-up chain, read from the stream at bit *pos by peek(pos) (64 bits, bit 63 first, zero
// past the data): the whole wave takes this path together.  False for an invalid code or a run over kG4MaxWidth.
template <class Peek>
DG_HD bool g4_run_slow(const G4Tabs &t, Peek peek, uint32_t *pos, uint32_t black, uint32_t *run) {
  for (*run = 0u; *run <= kG4MaxWidth;) {
    const uint32_t e = g4_lookup(t, peek(*pos), black);
    if (!e) return false;
    *pos += e >> 12;
    *run += e & 4095u;
    if ((e & 4095u) < 64u) return true;
  }
  return false;
}

// 64 bits of an MSB-first stream from three dwords read in memory order, s (< 32) bits into the first.
DG_HD uint64_t g4_window(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t s) {
  const uint32_t b0 = __builtin_bswap32(d0), b1 = __builtin_bswap32(d1), b2 = __builtin_bswap32(d2);
  const uint32_t hi = s ? b0 << s | b1 >> (32u - s) : b0, lo = s ? b1 << s | b2 >> (32u - s) : b1;
  return (uint64_t)hi << 32 | lo;
}

// ---- rows
// The changing elements of a row word: pixels that differ from the pixel before (prev: the word before, 0 for the first).
DG_HD uint32_t g4_trans(uint32_t r, uint32_t prev) { return r ^ (r << 1 | prev >> 31); }
// The pixels of [x0, x1) that lie in word i.
DG_HD uint32_t g4_span(uint32_t i, uint32_t x0, uint32_t x1) {
  const uint32_t lo = x0 > 32u * i ? x0 : 32u * i, hi = x1 < 32u * i + 32u ? x1 : 32u * i + 32u;
  if (lo >= hi) return 0u;
  return (hi - lo == 32u ? ~0u : (1u << (hi - lo)) - 1u) << (lo - 32u * i);
}
// The position of set bit n (from 0) of m, which has more than n.
DG_HD uint32_t g4_nth(uint32_t m, uint32_t n) {
  for (uint32_t k = 0; k < n && k < 32u; k++) m &= m - 1u;
  return (uint32_t)__builtin_ctz(m | 0x80000000u);
}
// A row word as the four bytes of the TIFF row in memory order: pixel x in bit 7 - (x & 7) of byte x >> 3.
DG_HD uint32_t g4_out(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bswap32(__builtin_bitreverse32(v));
#else
  v = (v & 0x55555555u) << 1 | (v >> 1 & 0x55555555u);
  v = (v & 0x33333333u) << 2 | (v >> 2 & 0x33333333u);
  return (v & 0x0F0F0F0Fu) << 4 | (v >> 4 & 0x0F0F0F0Fu);
#endif
}

}  // namespace dg
