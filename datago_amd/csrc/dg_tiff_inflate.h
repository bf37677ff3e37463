// dg_tiff_inflate.h — the per-lane routines of k_tiff_inflate (dg_tiff_inflate.hip, option
// "tiff_deflate"), shared with the CPU form in tests/native/tiff_inflate_emu.cpp.
//
// A TIFF segment of compression 8 (or 32946) is one zlib stream (RFC 1950 around RFC 1951).
// Inside a Huffman block every lane decodes the whole token that would start at its own bit
// offset (tinf_token): a literal, an end-of-block code, or a length with its extra bits, its
// distance code and that code's extra bits, at most 48 bits.  Which lanes are token starts is
// settled afterwards by hopping from start to start.
//
// Tables.  A code is kept in canonical form: cnt[l] codes of length l and the symbols sorted by
// (length, symbol).  tinf_walk is the canonical walk over them; the primary tables (the next
// kTinfLlBits / kTinfDdBits bits -> an entry) are filled by running it once per entry, and a lane
// whose code is longer than the primary index resumes the walk where the index ends (TinfWalk), five
// or six more bits at the most.  An entry holds all a lane needs: code length, extra bit count, kind
// and the literal, the base length or the base distance (tinf_ll_entry, tinf_dd_entry: the bases in
// closed form).  Entry 0 says "walk".
#pragma once
#include "dg_types.h"

namespace dg {

constexpr uint32_t kTinfLlBits = 10, kTinfLlSize = 1u << kTinfLlBits;  // primary literal/length index
constexpr uint32_t kTinfDdBits = 9, kTinfDdSize = 1u << kTinfDdBits;   // primary distance index
constexpr uint32_t kTinfClBits = 7, kTinfClSize = 1u << kTinfClBits;   // the code-length code: whole
constexpr uint32_t kTinfMaxLl = 286, kTinfMaxDd = 30;                  // zlib refuses HLIT / HDIST above these
constexpr uint32_t kTinfStepBytes = 24;  // source bytes a step's 64 lanes may touch: 63 + 7 + 64 bits, whole dwords
constexpr uint32_t kTinfWinBytes = 256;  // the source window: one dword per lane
constexpr uint32_t kTinfShort = 8;       // matches up to this length are copied by their own lane
constexpr uint32_t kTinfAdlerMod = 65521;

// Kinds of a token.  The first four stand in table entries; kTinfPast is given to a token that passes the data's end.
constexpr uint32_t kTinfLit = 0, kTinfMatch = 1, kTinfEob = 2, kTinfBad = 3, kTinfPast = 4;

struct TinfTok {
  uint32_t nb;    // bits of the whole token (at least 1)
  uint32_t kind;  // kTinf*
  uint32_t val;   // the literal, or the match length
  uint32_t dist;
};
// Where a walk resumes after the pb bits of a primary index: the canonical first code and the
// symbol index of length pb + 1.
struct TinfWalk {
  uint32_t first, index;
};
struct TinfTabs {
  const uint32_t *ll, *dd;            // primary tables
  const uint16_t *lcnt, *lsym;        // literal/length code: counts per length [16], sorted symbols
  const uint16_t *dcnt, *dsym;        // distance code
  TinfWalk lw, dw;
};

// The two zlib header bytes: deflate, a window of at most 32 KiB, the check bits, no preset dictionary.
DG_HD bool tinf_zlib_ok(uint32_t cmf, uint32_t flg) {
  return (cmf & 15u) == 8u && (cmf >> 4) <= 7u && ((cmf << 8) | flg) % 31u == 0u && !(flg & 32u);
}

// Position i (< 19) of the code-length code's lengths in a dynamic header -> its symbol.
DG_HD uint32_t tinf_cl_order(uint32_t i) {
  constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                          10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (uint32_t)((i < 12u ? lo >> (5u * i) : hi >> (5u * (i - 12u))) & 31ull);
}

// Code length of literal/length symbol s in a fixed block.
DG_HD uint32_t tinf_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }

// The low n (<= 16) bits of v, first bit last.
DG_HD uint32_t tinf_rev(uint32_t v, uint32_t n) {
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
  v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
  return v >> (16u - n);
}

// The canonical walk: the code that starts at bit 0 of `bits`, of a length above pb and up to maxlen, as
// length << 16 | symbol; 0 if there is none.  w is the state after pb lengths ({0, 0} with pb 0).
DG_HD uint32_t tinf_walk(uint32_t bits, const uint16_t *cnt, const uint16_t *sym, uint32_t pb, TinfWalk w, uint32_t maxlen) {
  uint32_t code = tinf_rev(bits, pb) << 1, first = w.first, index = w.index;
  bits >>= pb;
  for (uint32_t len = pb + 1u; len <= maxlen; len++) {
    code |= bits & 1u;
    bits >>= 1;
    const uint32_t count = cnt[len];
    if (code - first < count) return (len << 16) | sym[index + (code - first)];
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return 0u;
}
// The walk's state after the pb bits of a primary index.
DG_HD TinfWalk tinf_walk_from(const uint16_t *cnt, uint32_t pb) {
  TinfWalk w = {0u, 0u};
  for (uint32_t len = 1; len <= pb; len++) {
    w.index += cnt[len];
    w.first = (w.first + cnt[len]) << 1;
  }
  return w;
}

// Entries: bits 0-3 code length, 4-7 extra bits, 8-9 kind, 16-31 the literal, base length or base distance.
DG_HD uint32_t tinf_ll_entry(uint32_t s, uint32_t len) {
  if (s < 256u) return len | (kTinfLit << 8) | (s << 16);
  if (s == 256u) return len | (kTinfEob << 8);
  if (s < 265u) return len | (kTinfMatch << 8) | ((s - 254u) << 16);
  if (s < 285u) {
    const uint32_t e = (s - 261u) >> 2;
    return len | (e << 4) | (kTinfMatch << 8) | ((3u + ((4u + ((s - 261u) & 3u)) << e)) << 16);
  }
  if (s == 285u) return len | (kTinfMatch << 8) | (258u << 16);
  return len | (kTinfBad << 8);  // 286 and 287 have codes in a fixed block and no meaning
}
DG_HD uint32_t tinf_dd_entry(uint32_t s, uint32_t len) {
  if (s >= kTinfMaxDd) return len | (kTinfBad << 8);
  if (s < 4u) return len | (kTinfMatch << 8) | ((s + 1u) << 16);
  const uint32_t e = (s >> 1) - 1u;
  return len | (e << 4) | (kTinfMatch << 8) | ((1u + ((2u + (s & 1u)) << e)) << 16);
}
// Entry i of a primary table of pb bits (dist: of the distance code).
DG_HD uint32_t tinf_primary(uint32_t i, const uint16_t *cnt, const uint16_t *sym, uint32_t pb, bool dist) {
  const uint32_t w = tinf_walk(i, cnt, sym, 0u, TinfWalk{0u, 0u}, pb);
  return !w ? 0u : dist ? tinf_dd_entry(w & 0xFFFFu, w >> 16) : tinf_ll_entry(w & 0xFFFFu, w >> 16);
}

// The token that starts at bit 0 of b (64 bits of the stream, first bit lowest).
DG_HD TinfTok tinf_token(uint64_t b, const TinfTabs &T) {
  TinfTok bad = {1u, kTinfBad, 0u, 0u};
  uint32_t e = T.ll[(uint32_t)b & (kTinfLlSize - 1u)];
  if (!e) {
    const uint32_t w = tinf_walk((uint32_t)b & 0x7FFFu, T.lcnt, T.lsym, kTinfLlBits, T.lw, 15u);
    if (!w) return bad;
    e = tinf_ll_entry(w & 0xFFFFu, w >> 16);
  }
  uint32_t nb = e & 15u;
  const uint32_t kind = (e >> 8) & 3u, xb = (e >> 4) & 15u;
  if (kind != kTinfMatch) return TinfTok{nb, kind, e >> 16, 0u};
  b >>= nb;
  const uint32_t len = (e >> 16) + ((uint32_t)b & ((1u << xb) - 1u));
  b >>= xb;
  nb += xb;
  uint32_t d = T.dd[(uint32_t)b & (kTinfDdSize - 1u)];
  if (!d) {
    const uint32_t w = tinf_walk((uint32_t)b & 0x7FFFu, T.dcnt, T.dsym, kTinfDdBits, T.dw, 15u);
    if (!w) return bad;
    d = tinf_dd_entry(w & 0xFFFFu, w >> 16);
  }
  if (((d >> 8) & 3u) != kTinfMatch) return bad;
  const uint32_t dn = d & 15u, dx = (d >> 4) & 15u;
  b >>= dn;
  return TinfTok{nb + dn + dx, kTinfMatch, len, (d >> 16) + ((uint32_t)b & ((1u << dx) - 1u))};
}

// A token of the code-length code at bit 0 of b, from its table (length << 5 | symbol per 7-bit index):
// bits | count of lengths it gives << 8 | symbol << 16; 0 if there is no such code.
DG_HD uint32_t tinf_cl_token(uint32_t b, const uint8_t *tab) {
  const uint32_t e = tab[b & (kTinfClSize - 1u)], len = e >> 5, s = e & 31u;
  if (!len) return 0u;
  b >>= len;
  if (s < 16u) return len | (1u << 8) | (s << 16);
  if (s == 16u) return (len + 2u) | ((3u + (b & 3u)) << 8) | (s << 16);
  if (s == 17u) return (len + 3u) | ((3u + (b & 7u)) << 8) | (s << 16);
  return (len + 7u) | ((11u + (b & 127u)) << 8) | (s << 16);
}

// Byte t of a match of n bytes at distance dist reads byte tinf_src(t, dist, n) from the match's source:
// a distance below the length repeats the last dist bytes.
DG_HD uint32_t tinf_src(uint32_t t, uint32_t dist, uint32_t n) { return dist >= n ? t : dist == 1u ? 0u : t % dist; }

// What a kraft sum leaves open may stay open: zlib takes a code set with no code at all or with a single
// code of length 1 (never for the code-length code).
DG_HD bool tinf_set_ok(int32_t left, uint32_t ncodes, uint32_t ones, bool may_be_open) {
  return left == 0 || (left > 0 && may_be_open && (ncodes == 0u || (ncodes == 1u && ones == 1u)));
}

// Adler-32 over dwords: the four bytes of v at positions i .. i + 3 of n, `keep` of them inside the data;
// w = (n - i) mod 65521.  a and b stay below the modulus.
DG_HD void tinf_adler4(uint32_t v, uint32_t keep, uint32_t w, uint32_t &a, uint32_t &b) {
  if (keep < 4u) v &= (1u << (8u * keep)) - 1u;
  const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24;
  const uint32_t s = b0 + b1 + b2 + b3;
  a = (a + s) % kTinfAdlerMod;
  b = (b + w * s + kTinfAdlerMod - (b1 + 2u * b2 + 3u * b3)) % kTinfAdlerMod;  // byte j weighs n - i - j
}

}  // namespace dg
