// dg_penc_tree.h — the per-image Huffman codes of the PNG re-encoder (context
// option "penc_dynamic"): arithmetic shared by k_penc_tree in dg_penc.hip and
// the CPU form in tests/native/penc_tree_emu.cpp.
//
// From an image's literal/length histogram: length-limited code lengths by
// package-merge (L = 15; L = 7 for the code-length alphabet), canonical codes
// (RFC 1951 3.2.2), the run-length tokens of the lengths, the dynamic block's
// header bit string (3.2.7) and the choice between that block and the fixed
// one.  DESIGN.md "PNG re-encode" states the format; tests/ref_penc_dyn.py
// restates it in Python.
//
// Every function takes (lane, lanes, sync): the workgroup's threads share the
// loops over symbols and list items and meet at sync(); the host runs the same
// code with one lane and a sync that does nothing.  Loop bounds and branches
// around a sync depend only on shared data, so every lane reaches it.
#pragma once
#include "dg_types.h"

namespace dg {

constexpr uint32_t kPtLit = 286;      // literal/length symbols 0..285
constexpr uint32_t kPtCl = 19;        // code-length symbols
constexpr uint32_t kPtItems = 2 * kPtLit;
constexpr uint32_t kPtLevels = 15;
constexpr uint32_t kPtTableWords = 288;  // code table / histogram words per image
constexpr uint32_t kPtHdrWords = 136;    // 14 + 19 * 3 + 287 * 14 = 4089 bits at the most

struct PtWork {
  uint64_t w[2][kPtItems];   // weights of the previous and the current level's list
  uint64_t leafw[kPtLit];    // leaves ascending by (frequency, symbol)
  uint16_t leafsym[kPtLit];
  uint16_t pkgpos[kPtLevels - 1][kPtLit];  // level k = 2..L: position of package j in the level's list
  uint16_t size[kPtLevels + 1];            // items of level k's list
  uint16_t taken[kPtLevels + 1];           // leaves among the items taken from level k
};

struct PtOut {
  uint32_t table[kPtTableWords];  // per literal/length symbol: bit-reversed code | length << 16
  uint32_t hdr[kPtHdrWords];      // header bit string, LSB first, from stream bit 0
  uint16_t tok[kPtLit + 2];       // run-length tokens: symbol | extra value << 5
  uint8_t litlen[kPtTableWords];
  uint8_t cllen[kPtCl];
  uint16_t clcode[kPtCl];  // bit-reversed
  uint32_t clfreq[kPtCl];
  uint32_t ntok, hlit, hclen, hdr_bits, dyn;
  uint64_t dyn_bits, fixed_bits;  // whole blocks: header, tokens, end-of-block
};

// The order in which the code-length code's lengths are sent (RFC 1951 3.2.7).
// 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15, five bits each (no table in memory on the device)
DG_HD uint32_t pt_cl_order(uint32_t i) {
  constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                          6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// extra bits of a length symbol 257..285
DG_HD uint32_t pt_len_extra(uint32_t sym) { return (sym < 265 || sym == 285) ? 0u : (sym - 261) >> 2; }

// bits of a literal/length symbol under the fixed code (RFC 1951 3.2.6)
DG_HD uint32_t pt_fixed_len(uint32_t sym) { return sym < 144 ? 8u : sym < 256 ? 9u : sym < 280 ? 7u : 8u; }

// Optimal code lengths <= L of the symbols with f > 0 (nsym <= 286; L <= 15
// and 2^L >= the number of used symbols), by package-merge:
//   level 1's list is the leaves; level k's list merges the leaves with the
//   pairs (2j, 2j + 1) of level k - 1's list by weight, a leaf before a
//   package of its weight; a symbol's length is the number of the first 2n - 2
//   items of level L's list that contain it.
// Each merge goes by rank: a leaf lands at its index plus the packages lighter
// than it, a package at its index plus the leaves not heavier.  Only which
// items are packages is kept per level (pkgpos); walking back from level L,
// the first m items of a level hold p packages, so 2p items of the level
// below, and m - p leaves, which are the m - p lightest.  64-bit weights.
template <class Sync>
DG_HD void pt_lengths(const uint32_t *f, uint32_t nsym, uint32_t L, uint8_t *len, PtWork &k, uint32_t lane,
                      uint32_t lanes, Sync sync) {
  uint32_t n = 0;
  for (uint32_t s = 0; s < nsym; s++) n += f[s] != 0;
  for (uint32_t s = lane; s < nsym; s += lanes) {
    len[s] = 0;
    if (!f[s]) continue;
    uint32_t r = 0;
    for (uint32_t t = 0; t < nsym; t++) r += f[t] && (f[t] < f[s] || (f[t] == f[s] && t < s));
    k.leafw[r] = f[s];
    k.leafsym[r] = (uint16_t)s;
    k.w[1][r] = f[s];  // level 1
  }
  sync();
  if (n == 0) return;
  if (n == 1) {
    if (lane == 0) len[k.leafsym[0]] = 1;
    sync();
    return;
  }
  uint32_t size = n;
  if (lane == 0) k.size[1] = (uint16_t)n;
  for (uint32_t lv = 2; lv <= L; lv++) {
    const uint64_t *prev = k.w[(lv - 1) & 1];
    uint64_t *cur = k.w[lv & 1];
    const uint32_t np = size >> 1;
    for (uint32_t i = lane; i < n + np; i += lanes) {
      if (i < n) {  // leaf i: packages strictly lighter go before it
        const uint64_t wt = k.leafw[i];
        uint32_t lo = 0, hi = np;
        while (lo < hi) {
          const uint32_t m = (lo + hi) >> 1;
          if (prev[2 * m] + prev[2 * m + 1] < wt) lo = m + 1; else hi = m;
        }
        cur[i + lo] = wt;
      } else {  // package j: leaves not heavier go before it
        const uint32_t j = i - n;
        const uint64_t wt = prev[2 * j] + prev[2 * j + 1];
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
          const uint32_t m = (lo + hi) >> 1;
          if (k.leafw[m] <= wt) lo = m + 1; else hi = m;
        }
        cur[j + lo] = wt;
        k.pkgpos[lv - 2][j] = (uint16_t)(j + lo);
      }
    }
    size = n + np;
    if (lane == 0) k.size[lv] = (uint16_t)size;
    sync();
  }
  if (lane == 0) {
    uint32_t m = 2 * n - 2 < size ? 2 * n - 2 : size;
    for (uint32_t lv = L; lv >= 2; lv--) {
      const uint32_t np = k.size[lv] - n;
      uint32_t lo = 0, hi = np;  // packages among the first m items
      while (lo < hi) {
        const uint32_t c = (lo + hi) >> 1;
        if (k.pkgpos[lv - 2][c] < m) lo = c + 1; else hi = c;
      }
      k.taken[lv] = (uint16_t)(m - lo);
      m = 2 * lo;
    }
    k.taken[1] = (uint16_t)m;
  }
  sync();
  for (uint32_t i = lane; i < n; i += lanes) {
    uint32_t d = 0;
    for (uint32_t lv = 1; lv <= L; lv++) d += i < k.taken[lv];
    len[k.leafsym[i]] = (uint8_t)d;
  }
  sync();
}

// Canonical codes (RFC 1951 3.2.2) of lengths <= 15, bit-reversed: Huffman
// codes go MSB first into the LSB-first stream.  One lane.
template <class Store>
DG_HD void pt_codes(const uint8_t *len, uint32_t nsym, Store store) {
  uint32_t cnt[16], next[16];
  for (uint32_t b = 0; b < 16; b++) cnt[b] = 0;
  for (uint32_t s = 0; s < nsym; s++) cnt[len[s]]++;
  cnt[0] = 0;
  uint32_t code = 0;
  next[0] = 0;
  for (uint32_t b = 1; b < 16; b++) {
    code = (code + cnt[b - 1]) << 1;
    next[b] = code;
  }
  for (uint32_t s = 0; s < nsym; s++) {
    const uint32_t n = len[s];
    uint32_t c = n ? next[n]++ : 0u, r = 0;
    for (uint32_t b = 0; b < n; b++, c >>= 1) r = (r << 1) | (c & 1u);
    store(s, r, n);
  }
}

// Greedy run-length tokens of seq[0..n): zeros as 18 (11..138) while 11 or
// more remain, then 17 (3..10), then themselves; a nonzero length once, then
// 16 (3..6) while 3 or more remain, then itself.  token = symbol | extra << 5.
DG_HD uint32_t pt_rle(const uint8_t *seq, uint32_t n, uint16_t *tok) {
  uint32_t nt = 0, i = 0;
  while (i < n) {
    const uint32_t v = seq[i];
    uint32_t r = 1;
    while (i + r < n && seq[i + r] == v) r++;
    i += r;
    if (v == 0) {
      while (r >= 11) {
        const uint32_t c = r < 138 ? r : 138;
        tok[nt++] = (uint16_t)(18 | (c - 11) << 5);
        r -= c;
      }
      if (r >= 3) {
        tok[nt++] = (uint16_t)(17 | (r - 3) << 5);
        r = 0;
      }
      while (r--) tok[nt++] = 0;
    } else {
      tok[nt++] = (uint16_t)v;
      r--;
      while (r >= 3) {
        const uint32_t c = r < 6 ? r : 6;
        tok[nt++] = (uint16_t)(16 | (c - 3) << 5);
        r -= c;
      }
      while (r--) tok[nt++] = (uint16_t)v;
    }
  }
  return nt;
}

struct PtBits {
  uint32_t *w;
  uint32_t n;
};
DG_HD void pt_put(PtBits &b, uint32_t v, uint32_t nbits) {
  const uint32_t at = b.n & 31u, wi = b.n >> 5;
  b.w[wi] |= v << at;
  if (at + nbits > 32) b.w[wi + 1] |= v >> (32 - at);
  b.n += nbits;
}

// Everything k_penc_tree decides for one image, from its histogram f[0..286)
// (f[256] = 1): o.litlen, o.table, the header bits and the choice o.dyn.
// len_seq: 288 bytes of scratch for the run-length coder's input.
template <class Sync>
DG_HD void pt_build(const uint32_t *f, PtOut &o, PtWork &k, uint8_t *len_seq, uint32_t lane, uint32_t lanes,
                    Sync sync) {
  pt_lengths(f, kPtLit, 15, o.litlen, k, lane, lanes, sync);
  if (lane == 0) {
    uint32_t top = 256;
    for (uint32_t s = 257; s < kPtLit; s++)
      if (o.litlen[s]) top = s;
    o.hlit = top + 1 - 257;
    for (uint32_t s = 0; s <= top; s++) len_seq[s] = o.litlen[s];
    len_seq[top + 1] = 1;  // HDIST = 0: one distance code of one bit
    o.ntok = pt_rle(len_seq, top + 2, o.tok);
    for (uint32_t s = 0; s < kPtCl; s++) o.clfreq[s] = 0;
    for (uint32_t t = 0; t < o.ntok; t++) o.clfreq[o.tok[t] & 31u]++;
  }
  sync();
  pt_lengths(o.clfreq, kPtCl, 7, o.cllen, k, lane, lanes, sync);
  for (uint32_t i = lane; i < kPtHdrWords; i += lanes) o.hdr[i] = 0;
  sync();
  if (lane == 0) {
    pt_codes(o.litlen, kPtLit, [&](uint32_t s, uint32_t r, uint32_t n) { o.table[s] = r | n << 16; });
    o.table[286] = o.table[287] = 0;
    pt_codes(o.cllen, kPtCl, [&](uint32_t s, uint32_t r, uint32_t) { o.clcode[s] = (uint16_t)r; });
    uint32_t last = 0;
    for (uint32_t i = 0; i < kPtCl; i++)
      if (o.cllen[pt_cl_order(i)]) last = i;
    o.hclen = (last + 1 < 4 ? 4 : last + 1) - 4;
    PtBits b = {o.hdr, 0};
    pt_put(b, 1, 1);  // BFINAL
    pt_put(b, 2, 2);  // BTYPE = 10
    pt_put(b, o.hlit, 5);
    pt_put(b, 0, 5);  // HDIST
    pt_put(b, o.hclen, 4);
    for (uint32_t i = 0; i < o.hclen + 4; i++) pt_put(b, o.cllen[pt_cl_order(i)], 3);
    for (uint32_t t = 0; t < o.ntok; t++) {
      const uint32_t s = o.tok[t] & 31u, x = o.tok[t] >> 5;
      pt_put(b, o.clcode[s], o.cllen[s]);
      if (s >= 16) pt_put(b, x, s == 16 ? 2 : s == 17 ? 3 : 7);
    }
    o.hdr_bits = b.n;
    uint64_t dyn = b.n, fix = 3;
    for (uint32_t s = 0; s < kPtLit; s++) {
      const uint64_t x = s > 256 ? pt_len_extra(s) : 0, m = s > 256;
      dyn += (uint64_t)f[s] * (o.litlen[s] + x + m);         // a match: its extra bits and the 1-bit distance
      fix += (uint64_t)f[s] * (pt_fixed_len(s) + x + 5 * m);  // ... the fixed code's 5-bit distance
    }
    o.dyn_bits = dyn;
    o.fixed_bits = fix;
    o.dyn = dyn < fix;
  }
  sync();
}

}  // namespace dg
