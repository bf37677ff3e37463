// dg_jenc_tree.h — the per-image Huffman tables of the JPEG re-encoder
// (context option "jenc_optimize"): arithmetic shared by k_enc_tree in
// dg_enc.hip and the CPU form in tests/native/jenc_tree_emu.cpp.
//
// From one table's symbol counts: libjpeg's jpeg_gen_optimal_table, i.e. T.81
// K.2 (code sizes) and K.3 (the 16-bit limit) with jchuff.c's tie-breaks, then
// HUFFVAL, the canonical codes and the DHT segment.  DESIGN.md "JPEG
// re-encode" states the rule; tests/ref_jenc_opt.py restates it in Python.
//
// Every function takes (lane, lanes, sync, min2): the lanes of one wave share
// the loops over the 257 symbols (a lane owns the symbols lane, lane + lanes,
// ...) and meet at sync(); min2(a, b) replaces every lane's two least keys by
// the two least keys of all lanes.  The host runs the same code with one lane,
// a sync and a min2 that do nothing.  Loop bounds and branches around a sync or
// a min2 depend only on shared data, so every lane reaches them.
#pragma once
#include "dg_types.h"

namespace dg {

constexpr uint32_t kJtSyms = 257;        // symbols 0..255 and the reserved symbol 256
constexpr uint32_t kJtMaxSize = 32;      // K.2 sizes K.3 can take (libjpeg's MAX_CLEN)
constexpr uint64_t kJtNoKey = ~0ull;

// Per image, in front of its scan bit buffer (zeroed per batch with it):
// the histogram, the image's EncTables, its DHT segments.
constexpr uint32_t kJencDcSyms = 16;                        // DC categories 0..11 (the index is masked to 4 bits)
constexpr uint32_t kJencHistPair = kJencDcSyms + 256;       // one table pair: DC counters, then AC counters
constexpr uint32_t kJencHistWords = 2 * kJencHistPair;      // luma pair, chroma pair
constexpr uint32_t kJencTabOff = kJencHistWords * 4;        // EncTables (3072 bytes)
constexpr uint32_t kJencDhtOff = kJencTabOff + 3072;
constexpr uint32_t kJencDhtMax = 2 * (21 + kJencDcSyms) + 2 * (21 + 256);  // 628
constexpr uint32_t kJencOptBytes = 6144;                    // multiple of 256
static_assert(sizeof(EncTables) == 3072, "kJencDhtOff");
static_assert(kJencDhtOff + kJencDhtMax <= kJencOptBytes, "the per-image table region");

struct JtWork {
  uint64_t cnt[kJtSyms];   // K.2: the count of the tree a symbol is the root of, else 0
  uint16_t lab[kJtSyms];   // K.2: the root of the symbol's tree
  uint8_t size[kJtSyms];   // K.2 code size (saturating at 255)
  uint32_t over;           // a size above kJtMaxSize
  uint32_t kbits[kJtMaxSize + 1];
  uint32_t first_rank[17], first_code[17];
};

struct JtOut {
  uint8_t bits[17];   // BITS: codes of length 1..16 (bits[0] unused)
  uint8_t vals[256];  // HUFFVAL
  uint32_t nvals;
  uint32_t fallback;  // 1: a K.2 size above 32 (libjpeg raises an error): nothing else here is valid
};

// K.2 key of a live tree: least count first, the largest index winning ties.
DG_HD uint64_t jt_key(uint64_t cnt, uint32_t s) { return cnt << 9 | (511u - s); }

// One table.  f[s] for s < nf are the counts (the rest are zero); code[s] /
// len[s] receive the code of every symbol 0..255 (0 / 0: unused).
template <class Freq, class Code, class Len, class Sync, class Min2>
DG_HD void jt_build(Freq f, uint32_t nf, JtWork &w, JtOut &o, Code code, Len len, uint32_t lane, uint32_t lanes,
                    Sync sync, Min2 min2) {
  for (uint32_t s = lane; s < kJtSyms; s += lanes) {
    w.cnt[s] = s < nf ? (uint64_t)f[s] : s == 256 ? 1u : 0u;
    w.lab[s] = (uint16_t)s;
    w.size[s] = 0;
  }
  if (lane == 0) w.over = 0;
  // K.2.  A lane reads and writes its own symbols only; c1 and c2 reach every lane through min2.
  for (;;) {
    uint64_t a = kJtNoKey, b = kJtNoKey;
    for (uint32_t s = lane; s < kJtSyms; s += lanes) {
      if (!w.cnt[s]) continue;
      const uint64_t k = jt_key(w.cnt[s], s);
      if (k < a) {
        b = a;
        a = k;
      } else if (k < b) {
        b = k;
      }
    }
    min2(a, b);
    if (b == kJtNoKey) break;  // one tree left
    const uint32_t c1 = 511u - (uint32_t)(a & 511u), c2 = 511u - (uint32_t)(b & 511u);
    for (uint32_t s = lane; s < kJtSyms; s += lanes) {
      if (w.lab[s] != c1 && w.lab[s] != c2) continue;  // jchuff.c walks both chains; the labels name their members
      w.lab[s] = (uint16_t)c1;
      if (w.size[s] < 255) w.size[s]++;
    }
    if (c1 % lanes == lane) w.cnt[c1] = (a >> 9) + (b >> 9);
    if (c2 % lanes == lane) w.cnt[c2] = 0;
  }
  sync();
  bool over = false;
  for (uint32_t s = lane; s < kJtSyms; s += lanes) over |= w.size[s] > kJtMaxSize;
  if (over) w.over = 1;
  sync();
  if (lane == 0) {
    o.fallback = w.over;
    o.nvals = 0;
    for (uint32_t i = 0; i <= 16; i++) o.bits[i] = 0;
  }
  if (w.over) {
    sync();
    return;
  }
  if (lane == 0) {  // K.3
    for (uint32_t i = 0; i <= kJtMaxSize; i++) w.kbits[i] = 0;
    for (uint32_t s = 0; s < kJtSyms; s++) w.kbits[w.size[s]]++;
    w.kbits[0] = 0;
    for (uint32_t i = kJtMaxSize; i > 16; i--) {
      while (w.kbits[i] > 0) {
        uint32_t j = i - 2;
        while (j > 1 && w.kbits[j] == 0) j--;  // (the sizes are a full tree's: a shorter code exists)
        w.kbits[i] -= 2;
        w.kbits[i - 1] += 1;
        w.kbits[j + 1] += 2;
        w.kbits[j] -= 1;
      }
    }
    uint32_t top = 16;
    while (w.kbits[top] == 0) top--;
    w.kbits[top]--;  // the reserved symbol's code
    uint32_t rank = 0, c = 0;
    for (uint32_t i = 1; i <= 16; i++) {
      o.bits[i] = (uint8_t)w.kbits[i];
      w.first_rank[i] = rank;
      w.first_code[i] = c;
      rank += w.kbits[i];
      c = (c + w.kbits[i]) << 1;
    }
    o.nvals = rank;
  }
  sync();
  // HUFFVAL: by K.2 size, then by value; the lengths follow BITS along that order.
  for (uint32_t s = lane; s < 256; s += lanes) {
    const uint32_t z = w.size[s];
    uint32_t c = 0, n = 0;
    if (z) {
      uint32_t r = 0;
      for (uint32_t t = 0; t < 256; t++) {
        const uint32_t y = w.size[t];
        r += y && (y < z || (y == z && t < s));
      }
      n = 1;
      while (r >= w.first_rank[n] + o.bits[n]) n++;
      c = w.first_code[n] + (r - w.first_rank[n]);
      o.vals[r] = (uint8_t)s;
    }
    code[s] = (uint16_t)c;
    len[s] = (uint8_t)n;
  }
  sync();
}

// The DHT segment of one table (class byte cls): FF C4, length, cls, BITS, HUFFVAL; 21 + nvals bytes.
DG_HD uint32_t jt_dht_bytes(const JtOut &o) { return 21u + o.nvals; }
template <class Bytes>
DG_HD void jt_dht(const JtOut &o, uint32_t cls, Bytes dst, uint32_t lane, uint32_t lanes) {
  const uint32_t n = jt_dht_bytes(o), seg = n - 2;
  for (uint32_t i = lane; i < n; i += lanes)
    dst[i] = i == 0 ? 0xFF : i == 1 ? 0xC4 : i == 2 ? (uint8_t)(seg >> 8) : i == 3 ? (uint8_t)seg
           : i == 4 ? (uint8_t)cls : i < 21 ? o.bits[i - 4] : o.vals[i - 21];
}

}  // namespace dg
