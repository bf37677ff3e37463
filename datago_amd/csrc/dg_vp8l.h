// dg_vp8l.h — the lossless WebP (VP8L) decode of option "webp": the lane routines
// and the wave-uniform walk of k_vp8l_decode / k_vp8l_inverse (dg_vp8l.hip), shared
// with the CPU form in tests/native/vp8l_emu.cpp.
//
// What they restate: the VP8L bitstream as libwebp reads it (tests/ref_webp.py is
// the plain restatement the tests compare to, pinned to Pillow).
//
// The walk over the bitstream is serial and wave-uniform: every lane holds the same
// reader state and takes the same branches.  It is written once, here, as templates
// over an environment E that supplies what differs between the wave and its CPU
// emulation: the staged source window, the code-length scratch, the table build
// (lanes over symbols), the wave-wide copy with its cache inserts, and the loads
// that read back what the wave stored.  Every loop is bounded by the chunk's bit
// count and the plane's pixel count: an iteration consumes bits or pixels or ends
// the decode (codes of one symbol read no bits; then the pixel count alone bounds it).
//
// Prefix-code tables, per group and code (green, red, blue, alpha, distance):
//   first[256]   entry for the next 8 stream bits: kVp8lValid | len << 16 | symbol for
//                a code of at most 8 bits (len 0: the code has one symbol), else 0
//   cnt[16]      codes per length, and sorted[]: the symbols in canonical order, for
//                the longer codes (walked bit by bit from the same 15 peeked bits)
// The current group's first[] and cnt[] are kept in LDS; a group change reloads them.
#pragma once
#include "dg_types.h"

namespace dg {

constexpr uint32_t kVp8lMaxGroups = 128;    // prefix-code groups per image the table area holds ("WebP")
constexpr uint32_t kVp8lMaxCache = 11;      // colour cache bits
constexpr uint32_t kVp8lGreen = 256 + 24 + (1u << kVp8lMaxCache);  // largest green alphabet
constexpr uint32_t kVp8lLensBytes = 2336;   // code-length scratch (>= kVp8lGreen, a multiple of 64)
constexpr uint32_t kVp8lWinDwords = 512;    // source window a wave keeps in LDS
constexpr uint32_t kVp8lValid = 0x80000000u;
// a group's table area in u32 words: 5 x first[256], 5 x cnt[16], then the sorted symbols, a word each
constexpr uint32_t kVp8lSortedOff[5] = {0, kVp8lGreen, kVp8lGreen + 256, kVp8lGreen + 512, kVp8lGreen + 768};
constexpr uint32_t kVp8lSortedAll = kVp8lGreen + 768 + 40;
constexpr uint32_t kVp8lGroupWords = 5 * 256 + 5 * 16 + kVp8lSortedAll;  // sorted symbols as whole words

constexpr uint32_t kVp8lPredictor = 0, kVp8lColor = 1, kVp8lGreenT = 2, kVp8lIndex = 3;

// the work arena of a w x h image, in u32 words: two ARGB planes, three sub-image planes
// (predictor, colour, entropy image: blocks are at least 4 x 4), the colour table
DG_HD uint32_t vp8l_sub_words(uint32_t w, uint32_t h) { return ((w + 3u) >> 2) * ((h + 3u) >> 2); }
DG_HD uint64_t vp8l_plane_off(uint32_t w, uint32_t h, uint32_t p) { return (uint64_t)w * h * p; }
DG_HD uint64_t vp8l_sub_off(uint32_t w, uint32_t h, uint32_t k) { return 2ull * w * h + (uint64_t)vp8l_sub_words(w, h) * k; }
DG_HD uint64_t vp8l_pal_off(uint32_t w, uint32_t h) { return vp8l_sub_off(w, h, 3); }
DG_HD uint64_t vp8l_work_words(uint32_t w, uint32_t h) { return vp8l_pal_off(w, h) + 256u; }
DG_HD uint32_t vp8l_groups_cap(uint32_t w, uint32_t h) {
  const uint32_t b = vp8l_sub_words(w, h);
  return b < kVp8lMaxGroups ? b : kVp8lMaxGroups;
}

DG_HD uint32_t vp8l_div_up(uint32_t v, uint32_t bits) { return (v + (1u << bits) - 1u) >> bits; }
DG_HD uint32_t vp8l_index_bits(uint32_t n) { return n > 16u ? 0u : n > 4u ? 1u : n > 2u ? 2u : 3u; }
// a transform as k_vp8l_decode records it: type, block / packing bits, the width it applies to
DG_HD uint32_t vp8l_trans_pack(uint32_t type, uint32_t bits, uint32_t xs) { return type | (bits << 2) | (xs << 8); }

DG_HD uint32_t vp8l_cache_slot(uint32_t argb, uint32_t bits) { return (0x1e35a7bdu * argb) >> (32u - bits); }

// Distance codes 1..120: (y << 4) | (8 - x) of the neighbour, nearest first.
DG_HD uint32_t vp8l_plane_code(uint32_t i) {
  static constexpr uint8_t m[120] = {
      0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
      0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
      0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
      0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
      0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
      0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
  return m[i];
}
// The pixel distance of distance code `code` (>= 1) on rows of `width`: below 1 it becomes 1.
DG_HD uint32_t vp8l_distance(uint32_t width, uint32_t code) {
  if (code > 120u) return code - 120u;
  const uint32_t m = vp8l_plane_code(code - 1u);
  const int32_t d = (int32_t)((m >> 4) * width) + 8 - (int32_t)(m & 15u);
  return d >= 1 ? (uint32_t)d : 1u;
}
// Length / distance prefix symbol: extra bits to read, and the value with them.
DG_HD uint32_t vp8l_prefix_extra(uint32_t sym) { return sym < 4u ? 0u : (sym - 2u) >> 1; }
DG_HD uint32_t vp8l_prefix_value(uint32_t sym, uint32_t extra) {
  if (sym < 4u) return sym + 1u;
  return ((2u + (sym & 1u)) << ((sym - 2u) >> 1)) + extra + 1u;
}
// Pixel t of a copy of distance d to position pos: a distance under the length repeats by period.
DG_HD uint32_t vp8l_copy_src(uint32_t pos, uint32_t d, uint32_t t) { return pos - d + (t < d ? t : t % d); }

DG_HD uint32_t vp8l_rev(uint32_t c, uint32_t n) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < n; i++) r |= ((c >> i) & 1u) << (n - 1u - i);
  return r;
}
// cnt[1..15] of a length list: 0 invalid (empty, incomplete, over-subscribed), 1 one symbol, 2 complete
DG_HD uint32_t vp8l_code_kind(const uint32_t cnt[16]) {
  uint32_t total = 0;
  int32_t left = 1;
  for (uint32_t l = 1; l < 16; l++) {
    total += cnt[l];
    left = 2 * left - (int32_t)cnt[l];
    if (left < 0 && total != 1u) return 0u;
  }
  if (total == 1u) return 1u;
  return (total && left == 0) ? 2u : 0u;
}

// ------------------------------------------------------------ pixel arithmetic (ARGB in a u32, per byte mod 256)

DG_HD uint32_t vp8l_add(uint32_t a, uint32_t b) {
  return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}
DG_HD uint32_t vp8l_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
DG_HD int32_t vp8l_abs(int32_t v) { return v < 0 ? -v : v; }
DG_HD uint32_t vp8l_clip(int32_t v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }
DG_HD uint32_t vp8l_select(uint32_t L, uint32_t T, uint32_t TL) {
  int32_t pl = 0, pt = 0;
  for (uint32_t s = 0; s < 32; s += 8) {
    const int32_t l = (L >> s) & 255, t = (T >> s) & 255, tl = (TL >> s) & 255;
    pl += vp8l_abs(t - tl);
    pt += vp8l_abs(l - tl);
  }
  return pl < pt ? L : T;
}
DG_HD uint32_t vp8l_clamp_full(uint32_t L, uint32_t T, uint32_t TL) {
  uint32_t r = 0;
  for (uint32_t s = 0; s < 32; s += 8)
    r |= vp8l_clip((int32_t)((L >> s) & 255) + (int32_t)((T >> s) & 255) - (int32_t)((TL >> s) & 255)) << s;
  return r;
}
DG_HD uint32_t vp8l_clamp_half(uint32_t A, uint32_t TL) {
  uint32_t r = 0;
  for (uint32_t s = 0; s < 32; s += 8) {
    const int32_t a = (A >> s) & 255, b = (TL >> s) & 255;
    r |= vp8l_clip(a + (a - b) / 2) << s;  // C division: towards zero
  }
  return r;
}
// Predictor modes 0..13; 14 and 15 act as mode 0.
DG_HD uint32_t vp8l_predict(uint32_t mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (mode) {
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return vp8l_avg2(vp8l_avg2(L, TR), T);
    case 6: return vp8l_avg2(L, TL);
    case 7: return vp8l_avg2(L, T);
    case 8: return vp8l_avg2(TL, T);
    case 9: return vp8l_avg2(T, TR);
    case 10: return vp8l_avg2(vp8l_avg2(L, TL), vp8l_avg2(T, TR));
    case 11: return vp8l_select(L, T, TL);
    case 12: return vp8l_clamp_full(L, T, TL);
    case 13: return vp8l_clamp_half(vp8l_avg2(L, T), TL);
    default: return 0xff000000u;
  }
}
DG_HD int32_t vp8l_delta(uint32_t t, uint32_t c) { return ((int32_t)(int8_t)t * (int32_t)(int8_t)c) >> 5; }
// inverse colour transform of pixel p with the block's element m (r2b << 16 | g2b << 8 | g2r)
DG_HD uint32_t vp8l_color_inv(uint32_t m, uint32_t p) {
  const uint32_t g = (p >> 8) & 255u;
  const uint32_t r = ((p >> 16) + (uint32_t)vp8l_delta(m & 255u, g)) & 255u;
  const uint32_t b = (p + (uint32_t)vp8l_delta((m >> 8) & 255u, g) + (uint32_t)vp8l_delta((m >> 16) & 255u, r)) & 255u;
  return (p & 0xff00ff00u) | (r << 16) | b;
}
DG_HD uint32_t vp8l_green_inv(uint32_t p) {
  const uint32_t g = (p >> 8) & 255u;
  return (p & 0xff00ff00u) | ((((p >> 16) + g) & 255u) << 16) | ((p + g) & 255u);
}
// colour index of pixel x from its packed pixel (8 >> bits bits per index, in the green byte)
DG_HD uint32_t vp8l_index_of(uint32_t packed, uint32_t x, uint32_t bits) {
  const uint32_t bpp = 8u >> bits;
  return (((packed >> 8) & 255u) >> ((x & ((1u << bits) - 1u)) * bpp)) & ((1u << bpp) - 1u);
}

// ------------------------------------------------------------ the bit reader

// LSB-first over dwords of the 4-byte-aligned window E::src_dword serves (zeros past the end).
struct Vp8lBits {
  uint64_t buf;
  uint32_t nb;     // bits in buf
  uint32_t next;   // next dword of the source
  uint32_t used;   // bits consumed
  uint32_t nbits;  // bits the chunk holds
};
template <class E>
DG_HD void vp8l_fill(E &e, Vp8lBits &b) {
  if (b.nb <= 32u) {
    b.buf |= (uint64_t)e.src_dword(b.next++) << b.nb;
    b.nb += 32u;
  }
}
template <class E>
DG_HD void vp8l_open(E &e, Vp8lBits &b, uint32_t skip_bytes, uint32_t nbytes) {
  b.buf = 0;
  b.nb = 0;
  b.next = 0;
  b.used = 0;
  b.nbits = nbytes * 8u;
  vp8l_fill(e, b);
  b.buf >>= 8u * skip_bytes;
  b.nb -= 8u * skip_bytes;
}
DG_HD void vp8l_drop(Vp8lBits &b, uint32_t n) {
  b.buf >>= n;
  b.nb -= n;
  b.used += n;
}
template <class E>
DG_HD uint32_t vp8l_read(E &e, Vp8lBits &b, uint32_t n) {  // n <= 24
  vp8l_fill(e, b);
  const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
  vp8l_drop(b, n);
  return v;
}
DG_HD bool vp8l_past(const Vp8lBits &b) { return b.used > b.nbits; }

// One symbol of code k (0..4 of the current group, 5: the code-length code).
template <class E>
DG_HD uint32_t vp8l_symbol(E &e, Vp8lBits &b, uint32_t k) {
  vp8l_fill(e, b);
  const uint32_t peek = (uint32_t)b.buf;
  const uint32_t ent = e.first(k, peek & 255u);
  if (ent & kVp8lValid) {
    vp8l_drop(b, (ent >> 16) & 15u);
    return ent & 0xffffu;
  }
  int32_t code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len < 16u; len++) {
    code |= (int32_t)((peek >> (len - 1u)) & 1u);
    const int32_t count = (int32_t)e.cnt(k, len);
    if (code - count < first) {
      vp8l_drop(b, len);
      return e.sorted(k, (uint32_t)(index + (code - first)));
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  vp8l_drop(b, 15u);  // not reached with a complete code
  return 0u;
}

// Reads the description of code k over `alphabet` symbols and builds its table (group `grp`'s area).
template <class E>
DG_HD uint32_t vp8l_read_code(E &e, Vp8lBits &b, uint32_t k, uint32_t alphabet, uint32_t grp) {
  e.lens_fill(0u, alphabet, 0u);
  if (vp8l_read(e, b, 1)) {  // simple: one or two symbols
    const uint32_t n = vp8l_read(e, b, 1) + 1u;
    const uint32_t s0 = vp8l_read(e, b, vp8l_read(e, b, 1) ? 8u : 1u);
    const uint32_t s1 = n == 2u ? vp8l_read(e, b, 8) : s0;
    if (s0 >= alphabet || s1 >= alphabet) return kVp8lFailCode;
    e.lens_fill(s0, 1u, 1u);
    e.lens_fill(s1, 1u, 1u);
  } else {
    static constexpr uint8_t order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    const uint32_t n = 4u + vp8l_read(e, b, 4);
    for (uint32_t i = 0; i < n; i++) e.lens_fill(order[i], 1u, vp8l_read(e, b, 3));
    if (vp8l_past(b)) return kVp8lFailBits;
    if (!e.build(5u, 19u, 0u)) return kVp8lFailCode;
    e.lens_fill(0u, 64u, 0u);
    uint32_t max_symbol = alphabet;
    if (vp8l_read(e, b, 1)) {
      const uint32_t nb = 2u + 2u * vp8l_read(e, b, 3);
      max_symbol = 2u + vp8l_read(e, b, nb);
      if (max_symbol > alphabet) return kVp8lFailCode;
    }
    uint32_t s = 0, prev = 8u;
    while (s < alphabet && max_symbol) {
      max_symbol--;
      if (vp8l_past(b)) return kVp8lFailBits;
      const uint32_t c = vp8l_symbol(e, b, 5u);
      if (c < 16u) {
        if (c) {
          e.lens_fill(s, 1u, c);
          prev = c;
        }
        s++;
      } else {
        const uint32_t rep = vp8l_read(e, b, c == 16u ? 2u : c == 17u ? 3u : 7u) + (c == 18u ? 11u : 3u);
        if (s + rep > alphabet) return kVp8lFailCode;
        if (c == 16u) e.lens_fill(s, rep, prev);
        s += rep;
      }
    }
  }
  if (vp8l_past(b)) return kVp8lFailBits;
  return e.build(k, alphabet, grp) ? 0u : kVp8lFailCode;
}

DG_HD uint32_t vp8l_alphabet(uint32_t k, uint32_t cache_bits) {
  return k == 0u ? 280u + (cache_bits ? 1u << cache_bits : 0u) : k == 4u ? 40u : 256u;
}

template <class E>
DG_HD uint32_t vp8l_read_cache_bits(E &e, Vp8lBits &b, uint32_t &bits) {
  bits = 0;
  if (!vp8l_read(e, b, 1)) return 0u;
  bits = vp8l_read(e, b, 4);
  return (bits < 1u || bits > kVp8lMaxCache) ? kVp8lFailCache : 0u;
}

template <class E>
DG_HD uint32_t vp8l_read_groups(E &e, Vp8lBits &b, uint32_t n, uint32_t cache_bits) {
  for (uint32_t g = 0; g < n; g++) {
    for (uint32_t k = 0; k < 5u; k++) {
      const uint32_t f = vp8l_read_code(e, b, k, vp8l_alphabet(k, cache_bits), g);
      if (f) return f;
    }
    e.save(g);
  }
  return 0u;
}

// The entropy-coded pixels of a w x h image into the plane at word offset `dst` of the work arena.
// meta: word offset of the entropy image (group = bits 8..23 of its pixels), or ~0 for one group.
// lax_end (see vp8l_walk): the end of the data is looked for before each pixel or copy only, so the symbols
// of the last one may read past it (zeros).
template <class E>
DG_HD uint32_t vp8l_pixels(E &e, Vp8lBits &b, uint64_t dst, uint32_t w, uint32_t h, uint32_t cache_bits, uint64_t meta,
                           uint32_t meta_bits, bool lax_end = false) {
  const uint32_t n = w * h;
  const bool grouped = meta != ~0ull;
  const uint32_t mw = grouped ? vp8l_div_up(w, meta_bits) : 0u;
  uint32_t pos = 0, x = 0, y = 0, blk = ~0u;
  if (cache_bits) e.cache_clear(cache_bits);
  if (!grouped) e.select(0u);
  while (pos < n) {
    if (vp8l_past(b)) return kVp8lFailBits;
    if (grouped) {
      const uint32_t nb = (y >> meta_bits) * mw + (x >> meta_bits);
      if (nb != blk) {
        blk = nb;
        e.select((e.meta_load(meta + nb) >> 8) & 0xffffu);
      }
    }
    const uint32_t s = vp8l_symbol(e, b, 0u);
    uint32_t adv = 1u;
    if (s < 256u) {
      const uint32_t r = vp8l_symbol(e, b, 1u);
      const uint32_t bl = vp8l_symbol(e, b, 2u);
      const uint32_t a = vp8l_symbol(e, b, 3u);
      const uint32_t p = (a << 24) | (r << 16) | (s << 8) | bl;
      e.work_store(dst + pos, p);
      if (cache_bits) e.cache_put(vp8l_cache_slot(p, cache_bits), p);
    } else if (s < 280u) {
      const uint32_t ls = s - 256u;
      const uint32_t len = vp8l_prefix_value(ls, vp8l_read(e, b, vp8l_prefix_extra(ls)));
      const uint32_t ds = vp8l_symbol(e, b, 4u);
      const uint32_t dist = vp8l_distance(w, vp8l_prefix_value(ds, vp8l_read(e, b, vp8l_prefix_extra(ds))));
      if (vp8l_past(b) && !lax_end) return kVp8lFailBits;
      if (dist > pos || len > n - pos) return kVp8lFailCopy;
      e.copy(dst, pos, dist, len, cache_bits);
      adv = len;
    } else {
      if (!cache_bits || s - 280u >= (1u << cache_bits)) return kVp8lFailCache;
      const uint32_t p = e.cache_get(s - 280u);
      e.work_store(dst + pos, p);
      e.cache_put(vp8l_cache_slot(p, cache_bits), p);
    }
    pos += adv;
    x += adv;
    if (x >= w) {
      y += x / w;
      x %= w;
    }
  }
  return (vp8l_past(b) && !lax_end) ? kVp8lFailBits : 0u;
}

// A sub-image (transform data, entropy image, colour table): its own cache, one group, no prefix image.
template <class E>
DG_HD uint32_t vp8l_sub_image(E &e, Vp8lBits &b, uint64_t dst, uint32_t w, uint32_t h) {
  uint32_t cb;
  uint32_t f = vp8l_read_cache_bits(e, b, cb);
  if (f) return f;
  f = vp8l_read_groups(e, b, 1u, cb);
  if (f) return f;
  return vp8l_pixels(e, b, dst, w, h, cb, ~0ull, 0u);
}

struct Vp8lWalk {
  uint32_t ntrans;
  uint32_t trans[4];  // vp8l_trans_pack, in the order read
  uint32_t xsize;     // width of the decoded (packed) image in plane 0
  uint32_t npal;
};

// The whole stream after the 5-byte header: transforms, then the image into plane 0.
// alph: the stream of an ALPH chunk (option "webp_alpha").  libwebp decodes such a stream through a path of
// its own when the image is what its encoder writes for few alpha levels (colour indexing as the only
// transform, no colour cache, one-symbol red, blue and alpha codes in every group), and that path looks for
// the end of the data after each pixel or copy only while pixels are missing: vp8l_pixels' lax_end.
template <class E>
DG_HD uint32_t vp8l_walk(E &e, Vp8lBits &b, uint32_t w, uint32_t h, uint32_t groups_cap, Vp8lWalk &o, bool alph = false) {
  o.ntrans = 0;
  o.npal = 0;
  o.xsize = w;
  for (uint32_t i = 0; i < 4u; i++) o.trans[i] = 0u;
  uint32_t xs = w, seen = 0, f;
  while (vp8l_read(e, b, 1)) {
    if (vp8l_past(b)) return kVp8lFailBits;
    const uint32_t t = vp8l_read(e, b, 2);
    if (seen & (1u << t)) return kVp8lFailTransform;
    seen |= 1u << t;
    uint32_t bits = 0;
    if (t == kVp8lPredictor || t == kVp8lColor) {
      bits = vp8l_read(e, b, 3) + 2u;
      f = vp8l_sub_image(e, b, vp8l_sub_off(w, h, t), vp8l_div_up(xs, bits), vp8l_div_up(h, bits));
      if (f) return f;
    } else if (t == kVp8lIndex) {
      o.npal = vp8l_read(e, b, 8) + 1u;
      bits = vp8l_index_bits(o.npal);
      f = vp8l_sub_image(e, b, vp8l_pal_off(w, h), o.npal, 1u);
      if (f) return f;
      e.pal_delta(vp8l_pal_off(w, h), o.npal);
    }
    o.trans[o.ntrans++] = vp8l_trans_pack(t, bits, xs);
    if (t == kVp8lIndex) xs = vp8l_div_up(xs, bits);
  }
  o.xsize = xs;
  uint32_t cb;
  f = vp8l_read_cache_bits(e, b, cb);
  if (f) return f;
  uint64_t meta = ~0ull;
  uint32_t mbits = 0, ngroups = 1;
  if (vp8l_read(e, b, 1)) {
    mbits = vp8l_read(e, b, 3) + 2u;
    meta = vp8l_sub_off(w, h, 2u);
    const uint32_t mn = vp8l_div_up(xs, mbits) * vp8l_div_up(h, mbits);
    f = vp8l_sub_image(e, b, meta, vp8l_div_up(xs, mbits), vp8l_div_up(h, mbits));
    if (f) return f;
    ngroups = e.max_group(meta, mn) + 1u;
  }
  if (vp8l_past(b)) return kVp8lFailBits;
  if (ngroups > groups_cap) return kVp8lFailGroups;
  f = vp8l_read_groups(e, b, ngroups, cb);
  if (f) return f;
  bool lax_end = alph && o.ntrans == 1u && (o.trans[0] & 3u) == kVp8lIndex && !cb;
  for (uint32_t g = 0; lax_end && g < ngroups; g++) {
    e.select(g);
    for (uint32_t k = 1; k < 4u; k++) {
      const uint32_t ent = e.first(k, 0u);  // a one-symbol code: every entry valid with no bits
      if (!(ent & kVp8lValid) || ((ent >> 16) & 15u)) lax_end = false;
    }
  }
  return vp8l_pixels(e, b, 0ull, xs, h, cb, meta, mbits, lax_end);
}

// ------------------------------------------------------------ the predictor's wavefront

// Strips of 64 rows: lane r owns row y0 + r and stands at x = t - 2r in step t, so the
// pixel to its left is its own last value and TL, T, TR are the last three values
// of lane r - 1.  Steps of a strip on rows of w pixels:
DG_HD uint32_t vp8l_strip_steps(uint32_t w) { return w + 126u; }

}  // namespace dg
