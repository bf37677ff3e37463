// dg_vp8.h — the lossy WebP (VP8 key frame) decode of option "webp_lossy": the
// wave-uniform walk of k_vp8_parse and the lane routines of k_vp8_recon, k_vp8_filter
// and k_vp8_rgb (dg_vp8.hip), shared with the CPU form in tests/native/vp8_emu.cpp.
//
// What they restate: the VP8 key-frame bitstream (RFC 6386) as libwebp decodes it
// (tests/ref_vp8.py is the plain restatement the tests compare to, pinned to Pillow).
//
// Everything is written once, here, as templates over an environment E that supplies
// what differs between a wave and its CPU emulation:
//   e.lanes(f)        runs f(lane) for the 64 lanes, ordered against what comes before
//                     and after it (LDS and the arena alike)
//   e.src8 / src_be32 bytes of the VP8 chunk (offsets below the chunk's length only)
//   e.r8 / r16 / w8 / w32   the image's work arena, by byte offset
// The parse state (probabilities, contexts, the block buffer, the partition readers)
// is one struct, Vp8ParseState, that the kernel keeps in LDS; statements outside
// e.lanes are wave-uniform: every lane computes and stores the same values.
//
// Every loop is bounded by MB counts, block positions or tree depths; a reader that
// runs out of bytes takes zeros and is marked (libwebp's end-of-partition rule), and
// the frame is refused once the walk is through.  No wave waits on another.
#pragma once
#include "dg_types.h"
#include "dg_vp8_tables.h"

namespace dg {

constexpr uint32_t kVp8RecBytes = 32;    // per-MB record
constexpr uint32_t kVp8CoefBytes = 768;  // per-MB coefficients: 24 blocks x 16 int16
constexpr uint32_t kVp8MaxMbw = 1024;    // 14-bit widths
constexpr uint32_t kVp8ReconWaves = 4;   // waves of a k_vp8_recon / k_vp8_filter workgroup

// per-MB record, bytes
constexpr uint32_t kVp8RecI4 = 16, kVp8RecUv = 17, kVp8RecSeg = 18, kVp8RecInner = 19, kVp8RecLimit = 20,
                   kVp8RecIlevel = 21, kVp8RecHev = 22, kVp8RecSkip = 23, kVp8RecNzY = 24, kVp8RecNzUv = 25;

enum { VP8_DC_PRED = 0, VP8_TM_PRED, VP8_V_PRED, VP8_H_PRED };
enum { VP8_B_DC = 0, VP8_B_TM, VP8_B_VE, VP8_B_HE, VP8_B_RD, VP8_B_VR, VP8_B_LD, VP8_B_VL, VP8_B_HD, VP8_B_HU };

// The work arena of a w x h frame, sized from width and height alone (byte offsets, 256-aligned areas):
// per-MB records, coefficients, the Y / U / V planes padded to whole MBs, the coefficient probabilities.
struct Vp8Layout {
  uint32_t mbw, mbh;
  uint64_t rec, coef, y, u, v, prob, bytes;
};
DG_HD uint64_t vp8_up256(uint64_t v) { return (v + 255ull) & ~255ull; }
DG_HD Vp8Layout layout_vp8(uint32_t w, uint32_t h) {
  Vp8Layout l;
  l.mbw = (w + 15u) >> 4;
  l.mbh = (h + 15u) >> 4;
  const uint64_t nmb = (uint64_t)l.mbw * l.mbh;
  l.rec = 0;
  l.coef = vp8_up256(l.rec + nmb * kVp8RecBytes);
  l.y = vp8_up256(l.coef + nmb * kVp8CoefBytes);
  l.u = vp8_up256(l.y + nmb * 256u);
  l.v = vp8_up256(l.u + nmb * 64u);
  l.prob = vp8_up256(l.v + nmb * 64u);
  l.bytes = l.prob + 1280u;
  return l;
}

// ------------------------------------------------------------ the format's tables

DG_HD uint32_t vp8_coef0(uint32_t i) {
  static constexpr uint8_t t[1056] = {VP8_COEF0};
  return t[i];
}
DG_HD uint32_t vp8_upd(uint32_t i) {
  static constexpr uint8_t t[1056] = {VP8_UPD};
  return t[i];
}
DG_HD uint32_t vp8_bmode_prob(uint32_t i) {
  static constexpr uint8_t t[900] = {VP8_BMODES};
  return t[i];
}
DG_HD uint32_t vp8_dcq(int32_t q, int32_t cap) {
  static constexpr uint8_t t[128] = {VP8_DC};
  return t[q < 0 ? 0 : q > cap ? cap : q];
}
DG_HD uint32_t vp8_acq(int32_t q) {
  static constexpr uint16_t t[128] = {VP8_AC};
  return t[q < 0 ? 0 : q > 127 ? 127 : q];
}
DG_HD int32_t vp8_bmode_tree(uint32_t i) {
  static constexpr int8_t t[18] = {-VP8_B_DC, 1, -VP8_B_TM, 2, -VP8_B_VE, 3, 4, 6, -VP8_B_HE, 5, -VP8_B_RD, -VP8_B_VR,
                                   -VP8_B_LD, 7, -VP8_B_VL, 8, -VP8_B_HD, -VP8_B_HU};
  return t[i];
}
// zigzag {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15} and bands {0, 1, 2, 3, 6, 4, 5, 6 x 8, 7} as
// nibbles of a constant: the token walk asks per coefficient, and a register shift costs no load
DG_HD uint32_t vp8_zigzag(uint32_t i) { return (uint32_t)(0xfeb7adc963258410ull >> (4u * i)) & 15u; }
DG_HD uint32_t vp8_band(uint32_t i) {  // position 16 is asked for, never used
  return i < 16u ? (uint32_t)(0x7666666665463210ull >> (4u * i)) & 15u : 0u;
}
DG_HD uint32_t vp8_cat_prob(uint32_t cat, uint32_t i) {  // DCT categories 3..6: extra-bit probabilities, 0 ends
  static constexpr uint8_t t[4][12] = {{173, 148, 140, 0},
                                       {176, 155, 140, 135, 0},
                                       {180, 157, 141, 134, 130, 0},
                                       {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0}};
  return t[cat][i];
}

DG_HD int32_t vp8_i16(int32_t v) { return (int32_t)(int16_t)(uint16_t)(uint32_t)v; }  // stored as int16, as libwebp does
DG_HD int32_t vp8_clip8(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
DG_HD int32_t vp8_abs(int32_t v) { return v < 0 ? -v : v; }

// ------------------------------------------------------------ the bool reader

// libwebp's reader: value holds the bits loaded and not yet decided, `bits` of them below the
// decision point.  Loads take four bytes while four remain, then single bytes; one byte past
// the end is a zero and marks the reader.
struct Vp8Bool {
  uint64_t value;
  uint32_t range;  // range - 1
  int32_t bits;
  uint32_t pos, end;  // chunk offsets
  uint32_t eof;
};
template <class E>
DG_HD void vp8_load(E &e, Vp8Bool &b) {
  if (b.pos + 4u <= b.end) {
    b.value = (b.value << 32) | e.src_be32(b.pos);
    b.pos += 4u;
    b.bits += 32;
  } else if (b.pos < b.end) {
    b.value = (b.value << 8) | e.src8(b.pos);
    b.pos += 1u;
    b.bits += 8;
  } else if (!b.eof) {
    b.value <<= 8;
    b.bits += 8;
    b.eof = 1u;
  } else {
    b.bits = 0;
  }
}
template <class E>
DG_HD void vp8_open(E &e, Vp8Bool &b, uint32_t start, uint32_t end) {
  b.value = 0;
  b.range = 254u;
  b.bits = -8;
  b.pos = start;
  b.end = end;
  b.eof = 0u;
  vp8_load(e, b);
}
template <class E>
DG_HD uint32_t vp8_bit(E &e, Vp8Bool &b, uint32_t prob) {
  uint32_t range = b.range;
  if (b.bits < 0) vp8_load(e, b);
  const uint32_t pos = (uint32_t)b.bits;
  const uint32_t split = (range * prob) >> 8;
  const uint64_t value = b.value >> pos;
  uint32_t bit;
  if (value > split) {
    range -= split;
    b.value -= (uint64_t)(split + 1u) << pos;
    bit = 1u;
  } else {
    range = split + 1u;
    bit = 0u;
  }
  const uint32_t shift = 7u ^ (31u - (uint32_t)__builtin_clz(range));
  range <<= shift;
  b.bits -= (int32_t)shift;
  b.range = range - 1u;
  return bit;
}
template <class E>
DG_HD uint32_t vp8_get(E &e, Vp8Bool &b, uint32_t n) {
  uint32_t v = 0;
  while (n-- > 0u) v |= vp8_bit(e, b, 128u) << n;
  return v;
}
template <class E>
DG_HD int32_t vp8_signed(E &e, Vp8Bool &b, uint32_t n) {
  const int32_t v = (int32_t)vp8_get(e, b, n);
  return vp8_get(e, b, 1u) ? -v : v;
}
template <class E>
DG_HD int32_t vp8_opt_signed(E &e, Vp8Bool &b, uint32_t n) {
  return vp8_get(e, b, 1u) ? vp8_signed(e, b, n) : 0;
}

// ------------------------------------------------------------ the parse (k_vp8_parse)

struct Vp8ParseState {
  uint8_t prob[1056];           // [type][band][ctx][11]
  uint16_t qm[4][6];            // per segment: y1 dc, ac, y2 dc, ac, uv dc, ac
  uint32_t fs[4][2];            // per segment and (16x16, B_PRED): limit | ilevel << 8 | hev threshold << 16
  int32_t seg_q[4], seg_f[4];   // the header's per-segment values
  int16_t blk[400];             // the MB's 24 blocks, then the 16 luma DCs
  uint8_t top_nz[kVp8MaxMbw], top_dc[kVp8MaxMbw];
  uint8_t top_modes[4 * kVp8MaxMbw];
  Vp8Bool parts[8];
};

constexpr uint32_t kVp8FailBits = 1;   // a partition ends before the image is complete
constexpr uint32_t kVp8FailParts = 2;  // the token-partition table (or the last partition's start) past the chunk

struct Vp8Frame {  // what the later kernels need from the header
  uint32_t filter_type;  // 0 none, 1 simple, 2 normal
};

// One block's tokens from position n into S.blk[at..at+16), dequantised; returns 1 + the last non-zero position.
template <class E>
DG_HD uint32_t vp8_coeffs(E &e, Vp8Bool &b, uint32_t type, uint32_t ctx, uint32_t dq_dc, uint32_t dq_ac, uint32_t n,
                          uint32_t at) {
  Vp8ParseState &S = e.s;
  const uint8_t *p = &S.prob[((type * 8u + vp8_band(n)) * 3u + ctx) * 11u];
  for (; n < 16u; n++) {
    if (!vp8_bit(e, b, p[0])) return n;
    while (!vp8_bit(e, b, p[1])) {
      n++;
      p = &S.prob[((type * 8u + vp8_band(n)) * 3u) * 11u];
      if (n == 16u) return 16u;
    }
    int32_t v;
    uint32_t nc;
    if (!vp8_bit(e, b, p[2])) {
      v = 1;
      nc = 1u;
    } else {
      nc = 2u;
      if (!vp8_bit(e, b, p[3])) {
        if (!vp8_bit(e, b, p[4]))
          v = 2;
        else
          v = 3 + (int32_t)vp8_bit(e, b, p[5]);
      } else if (!vp8_bit(e, b, p[6])) {
        if (!vp8_bit(e, b, p[7])) {
          v = 5 + (int32_t)vp8_bit(e, b, 159u);
        } else {
          v = 7 + 2 * (int32_t)vp8_bit(e, b, 165u);
          v += (int32_t)vp8_bit(e, b, 145u);
        }
      } else {
        const uint32_t b1 = vp8_bit(e, b, p[8]);
        const uint32_t b0 = vp8_bit(e, b, p[9u + b1]);
        const uint32_t cat = 2u * b1 + b0;
        v = 0;
        for (uint32_t i = 0; i < 11u && vp8_cat_prob(cat, i); i++) v += v + (int32_t)vp8_bit(e, b, vp8_cat_prob(cat, i));
        v += 3 + (8 << cat);
      }
    }
    if (vp8_bit(e, b, 128u)) v = -v;
    S.blk[at + vp8_zigzag(n)] = (int16_t)vp8_i16(v * (int32_t)(n > 0u ? dq_ac : dq_dc));
    p = &S.prob[((type * 8u + vp8_band(n + 1u)) * 3u + nc) * 11u];
  }
  return 16u;
}

// Output k of the inverse WHT of dc[16].
DG_HD int32_t vp8_wht_tmp(const int16_t *dc, uint32_t r, uint32_t c) {
  const int32_t a0 = dc[c] + dc[12 + c], a1 = dc[4 + c] + dc[8 + c], a2 = dc[4 + c] - dc[8 + c], a3 = dc[c] - dc[12 + c];
  return r == 0u ? a0 + a1 : r == 1u ? a3 + a2 : r == 2u ? a0 - a1 : a3 - a2;
}
DG_HD int32_t vp8_wht_out(const int16_t *dc, uint32_t k) {
  // the second pass of row i reads tmp[4 i + c], c = 0..3, which the first pass made from column c
  const uint32_t i = k >> 2, j = k & 3u;
  const int32_t t0 = vp8_wht_tmp(dc, i, 0) + 3, t1 = vp8_wht_tmp(dc, i, 1), t2 = vp8_wht_tmp(dc, i, 2), t3 = vp8_wht_tmp(dc, i, 3);
  const int32_t a0 = t0 + t3, a1 = t1 + t2, a2 = t1 - t2, a3 = t0 - t3;
  return vp8_i16((j == 0u ? a0 + a1 : j == 1u ? a3 + a2 : j == 2u ? a0 - a1 : a3 - a2) >> 3);
}

// The whole frame: header, then per MB row its modes (first partition) and tokens (partition row mod n).
// Writes the records, the coefficients and the probabilities to the arena.
template <class E>
DG_HD uint32_t vp8_parse(E &e, uint32_t w, uint32_t h, uint32_t nbytes, uint32_t part0, Vp8Frame &fr) {
  Vp8ParseState &S = e.s;
  const Vp8Layout L = layout_vp8(w, h);
  fr.filter_type = 0;
  Vp8Bool br;
  vp8_open(e, br, 10u, 10u + part0);
  vp8_get(e, br, 2u);  // colour space, clamping type: neither changes what libwebp decodes
  const uint32_t use_seg = vp8_get(e, br, 1u);
  uint32_t update_map = 0, abs_delta = 1;
  uint32_t seg_p[3] = {255u, 255u, 255u};
  for (uint32_t i = 0; i < 4u; i++) S.seg_q[i] = S.seg_f[i] = 0;
  if (use_seg) {
    update_map = vp8_get(e, br, 1u);
    if (vp8_get(e, br, 1u)) {
      abs_delta = vp8_get(e, br, 1u);
      for (uint32_t i = 0; i < 4u; i++) S.seg_q[i] = vp8_opt_signed(e, br, 7u);
      for (uint32_t i = 0; i < 4u; i++) S.seg_f[i] = vp8_opt_signed(e, br, 6u);
    }
    if (update_map)
      for (uint32_t i = 0; i < 3u; i++) seg_p[i] = vp8_get(e, br, 1u) ? vp8_get(e, br, 8u) : 255u;
  }
  const uint32_t simple = vp8_get(e, br, 1u);
  const int32_t level = (int32_t)vp8_get(e, br, 6u);
  const int32_t sharp = (int32_t)vp8_get(e, br, 3u);
  const uint32_t use_lf = vp8_get(e, br, 1u);
  int32_t ref_lf0 = 0, mode_lf0 = 0;
  if (use_lf && vp8_get(e, br, 1u)) {
    for (uint32_t i = 0; i < 4u; i++) {
      const int32_t v = vp8_opt_signed(e, br, 6u);
      if (i == 0u) ref_lf0 = v;
    }
    for (uint32_t i = 0; i < 4u; i++) {
      const int32_t v = vp8_opt_signed(e, br, 6u);
      if (i == 0u) mode_lf0 = v;
    }
  }
  fr.filter_type = level == 0 ? 0u : simple ? 1u : 2u;
  const uint32_t nparts = 1u << vp8_get(e, br, 2u);
  // the token partitions: 3-byte sizes after the first partition; a size past the chunk is cut to it
  const uint32_t tab = 10u + part0;
  if ((uint64_t)tab + 3u * (nparts - 1u) > nbytes) return kVp8FailParts;
  {
    uint32_t start = tab + 3u * (nparts - 1u);
    for (uint32_t p = 0; p < nparts; p++) {
      const uint32_t left = nbytes - start;
      uint32_t sz = left;
      if (p + 1u < nparts) {
        sz = e.src8(tab + 3u * p) | (e.src8(tab + 3u * p + 1u) << 8) | (e.src8(tab + 3u * p + 2u) << 16);
        sz = sz < left ? sz : left;
      } else if (sz == 0u) {
        return kVp8FailParts;
      }
      Vp8Bool t;
      vp8_open(e, t, start, start + sz);
      S.parts[p] = t;
      start += sz;
    }
  }
  const int32_t base_q = (int32_t)vp8_get(e, br, 7u);
  int32_t dq[5];  // y1 dc, y2 dc, y2 ac, uv dc, uv ac
  for (uint32_t i = 0; i < 5u; i++) dq[i] = vp8_opt_signed(e, br, 4u);
  vp8_get(e, br, 1u);  // refresh entropy probabilities: nothing follows a key frame here
  e.lanes([&](uint32_t lane) {
    for (uint32_t i = lane; i < 1056u; i += 64u) S.prob[i] = (uint8_t)vp8_coef0(i);
    if (lane < 4u) {  // the segment's quantisers
      const int32_t q = use_seg ? S.seg_q[lane] + (abs_delta ? 0 : base_q) : base_q;
      const uint32_t y2ac = (vp8_acq(q + dq[2]) * 101581u) >> 16;  // x 155 / 100
      S.qm[lane][0] = (uint16_t)vp8_dcq(q + dq[0], 127);
      S.qm[lane][1] = (uint16_t)vp8_acq(q);
      S.qm[lane][2] = (uint16_t)(vp8_dcq(q + dq[1], 127) * 2u);
      S.qm[lane][3] = (uint16_t)(y2ac < 8u ? 8u : y2ac);
      S.qm[lane][4] = (uint16_t)vp8_dcq(q + dq[3], 117);
      S.qm[lane][5] = (uint16_t)vp8_acq(q + dq[4]);
    } else if (lane < 12u) {  // the segment's filter strengths, for 16x16 and B_PRED MBs
      const uint32_t s = (lane - 4u) >> 1, i4 = lane & 1u;
      int32_t lv = use_seg ? S.seg_f[s] + (abs_delta ? 0 : level) : level;
      if (use_lf) lv += ref_lf0 + (i4 ? mode_lf0 : 0);
      lv = lv < 0 ? 0 : lv > 63 ? 63 : lv;
      uint32_t v = 0;
      if (lv > 0) {
        int32_t il = lv;
        if (sharp > 0) {
          il >>= sharp > 4 ? 2 : 1;
          if (il > 9 - sharp) il = 9 - sharp;
        }
        if (il < 1) il = 1;
        v = (uint32_t)(2 * lv + il) | ((uint32_t)il << 8) | ((lv >= 40 ? 2u : lv >= 15 ? 1u : 0u) << 16);
      }
      S.fs[s][i4] = v;
    }
  });
  for (uint32_t i = 0; i < 1056u; i++)
    if (vp8_bit(e, br, vp8_upd(i))) S.prob[i] = (uint8_t)vp8_get(e, br, 8u);
  const uint32_t use_skip = vp8_get(e, br, 1u);
  const uint32_t skip_p = use_skip ? vp8_get(e, br, 8u) : 0u;
  e.lanes([&](uint32_t lane) {
    for (uint32_t i = lane; i < 264u; i += 64u) {
      const uint8_t *q = &S.prob[4u * i];
      e.w32(L.prob + 4u * i, q[0] | (q[1] << 8) | (q[2] << 16) | ((uint32_t)q[3] << 24));
    }
    for (uint32_t i = lane; i < L.mbw; i += 64u) {
      S.top_nz[i] = S.top_dc[i] = 0;
      for (uint32_t k = 0; k < 4u; k++) S.top_modes[4u * i + k] = VP8_B_DC;
    }
  });

  for (uint32_t my = 0; my < L.mbh; my++) {
    const uint32_t pi = my & (nparts - 1u);
    Vp8Bool tb = S.parts[pi];
    uint32_t left_modes[4] = {VP8_B_DC, VP8_B_DC, VP8_B_DC, VP8_B_DC};
    uint32_t left_nz = 0, left_dc = 0;
    for (uint32_t mx = 0; mx < L.mbw; mx++) {
      const uint32_t mb = my * L.mbw + mx;
      // ---- modes
      uint32_t seg = 0;
      if (update_map) seg = vp8_bit(e, br, seg_p[0]) ? 2u + vp8_bit(e, br, seg_p[2]) : vp8_bit(e, br, seg_p[1]);
      uint32_t skip = use_skip ? vp8_bit(e, br, skip_p) : 0u;
      const uint32_t i4 = vp8_bit(e, br, 145u) ? 0u : 1u;
      uint32_t rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (!i4) {
        const uint32_t ym = vp8_bit(e, br, 156u) ? (vp8_bit(e, br, 128u) ? VP8_TM_PRED : VP8_H_PRED)
                                                 : (vp8_bit(e, br, 163u) ? VP8_V_PRED : VP8_DC_PRED);
        rec[0] = ym;
        for (uint32_t k = 0; k < 4u; k++) {
          S.top_modes[4u * mx + k] = (uint8_t)ym;
          left_modes[k] = ym;
        }
      } else {
        for (uint32_t yy = 0; yy < 4u; yy++) {
          uint32_t m = left_modes[yy];
          for (uint32_t xx = 0; xx < 4u; xx++) {
            const uint32_t pb = ((uint32_t)S.top_modes[4u * mx + xx] * 10u + m) * 9u;
            int32_t i = vp8_bmode_tree(vp8_bit(e, br, vp8_bmode_prob(pb)));
            for (uint32_t depth = 0; depth < 9u && i > 0; depth++)
              i = vp8_bmode_tree(2u * (uint32_t)i + vp8_bit(e, br, vp8_bmode_prob(pb + (uint32_t)i)));
            m = (uint32_t)(-i);
            S.top_modes[4u * mx + xx] = (uint8_t)m;
            rec[yy] |= m << (8u * xx);
          }
          left_modes[yy] = m;
        }
      }
      const uint32_t uvm = !vp8_bit(e, br, 142u)   ? VP8_DC_PRED
                           : !vp8_bit(e, br, 114u) ? VP8_V_PRED
                           : vp8_bit(e, br, 183u)  ? VP8_TM_PRED
                                                   : VP8_H_PRED;
      // ---- tokens
      e.lanes([&](uint32_t lane) {
        for (uint32_t i = lane; i < 200u; i += 64u) S.blk[2u * i] = S.blk[2u * i + 1u] = 0;
      });
      uint32_t nzy = 0, nzuv = 0;
      if (skip) {
        left_nz = 0;
        S.top_nz[mx] = 0;
        if (!i4) {
          left_dc = 0;
          S.top_dc[mx] = 0;
        }
      } else {
        const uint16_t *q = S.qm[seg];
        uint32_t first = 0, type = 3;
        if (!i4) {
          const uint32_t nz = vp8_coeffs(e, tb, 1u, S.top_dc[mx] + left_dc, q[2], q[3], 0u, 384u);
          left_dc = nz > 0u ? 1u : 0u;
          S.top_dc[mx] = (uint8_t)left_dc;
          e.lanes([&](uint32_t lane) {  // the inverse WHT into the 16 luma DCs (one coefficient: the same values)
            if (lane < 16u) S.blk[16u * lane] = (int16_t)vp8_wht_out(&S.blk[384], lane);
          });
          first = 1;
          type = 0;
        }
        uint32_t tnz = S.top_nz[mx] & 15u, lnz = left_nz & 15u;
        for (uint32_t yy = 0; yy < 4u; yy++) {
          uint32_t l = lnz & 1u;
          for (uint32_t xx = 0; xx < 4u; xx++) {
            const uint32_t at = (4u * yy + xx) * 16u;
            const uint32_t nz = vp8_coeffs(e, tb, type, l + (tnz & 1u), q[0], q[1], first, at);
            l = nz > first ? 1u : 0u;
            tnz = (tnz >> 1) | (l << 7);
            nzy |= (nz > 1u || S.blk[at] != 0) ? 1u : 0u;
          }
          tnz >>= 4;
          lnz = (lnz >> 1) | (l << 7);
        }
        uint32_t out_t = tnz, out_l = lnz >> 4;
        for (uint32_t ch = 0; ch < 4u; ch += 2u) {
          tnz = (uint32_t)S.top_nz[mx] >> (4u + ch);
          lnz = left_nz >> (4u + ch);
          for (uint32_t yy = 0; yy < 2u; yy++) {
            uint32_t l = lnz & 1u;
            for (uint32_t xx = 0; xx < 2u; xx++) {
              const uint32_t at = (16u + 2u * ch + 2u * yy + xx) * 16u;
              const uint32_t nz = vp8_coeffs(e, tb, 2u, l + (tnz & 1u), q[4], q[5], 0u, at);
              l = nz > 0u ? 1u : 0u;
              tnz = (tnz >> 1) | (l << 3);
              nzuv |= (nz > 1u || S.blk[at] != 0) ? 1u : 0u;
            }
            tnz >>= 2;
            lnz = (lnz >> 1) | (l << 5);
          }
          out_t |= (tnz << 4) << ch;
          out_l |= (lnz & 0xf0u) << ch;
        }
        S.top_nz[mx] = (uint8_t)out_t;
        left_nz = out_l & 0xffu;
        skip = (nzy | nzuv) ? 0u : 1u;
      }
      const uint32_t f = S.fs[seg][i4];
      rec[4] = i4 | (uvm << 8) | (seg << 16) | (((i4 || !skip) ? 1u : 0u) << 24);
      rec[5] = (f & 0xffu) | (((f >> 8) & 0xffu) << 8) | (((f >> 16) & 0xffu) << 16) | (skip << 24);
      rec[6] = nzy | (nzuv << 8);
      e.lanes([&](uint32_t lane) {  // the record and the MB's 384 coefficients, whole lines
        if (lane < 8u) {
          uint32_t v = 0;
          for (uint32_t k = 0; k < 8u; k++) v = lane == k ? rec[k] : v;
          e.w32(L.rec + (uint64_t)mb * kVp8RecBytes + 4u * lane, v);
        }
        for (uint32_t i = lane; i < 192u; i += 64u)
          e.w32(L.coef + (uint64_t)mb * kVp8CoefBytes + 4u * i,
                (uint32_t)(uint16_t)S.blk[2u * i] | ((uint32_t)(uint16_t)S.blk[2u * i + 1u] << 16));
      });
    }
    S.parts[pi] = tb;
  }
  uint32_t eof = br.eof;
  for (uint32_t p = 0; p < nparts; p++) eof |= S.parts[p].eof;
  return eof ? kVp8FailBits : 0u;
}

// ------------------------------------------------------------ reconstruction (k_vp8_recon)

// A wave's staging of one MB: the luma with its border (row -1: top-left, 16 above, 4 above-right;
// column -1: left), and the two chroma blocks with theirs.  Index [r + 1][c + 1].
struct Vp8ReconBuf {
  uint8_t y[17][24];
  uint8_t u[9][12];
  uint8_t v[9][12];
};

DG_HD int32_t vp8_mul1(int32_t a) { return ((a * 20091) >> 16) + a; }
DG_HD int32_t vp8_mul2(int32_t a) { return (a * 35468) >> 16; }
// The residual of pixel (row i, column j) of the block whose coefficients are c[16] (row-major).
DG_HD int32_t vp8_idct_px(const int16_t *c, uint32_t i, uint32_t j) {
  int32_t t[4];  // the vertical pass's output i of column k
  for (uint32_t k = 0; k < 4u; k++) {
    const int32_t a = c[k] + c[8 + k], b = c[k] - c[8 + k];
    const int32_t cc = vp8_mul2(c[4 + k]) - vp8_mul1(c[12 + k]), d = vp8_mul1(c[4 + k]) + vp8_mul2(c[12 + k]);
    t[k] = i == 0u ? a + d : i == 1u ? b + cc : i == 2u ? b - cc : a - d;
  }
  const int32_t dc = t[0] + 4, a = dc + t[2], b = dc - t[2];
  const int32_t cc = vp8_mul2(t[1]) - vp8_mul1(t[3]), d = vp8_mul1(t[1]) + vp8_mul2(t[3]);
  return (j == 0u ? a + d : j == 1u ? b + cc : j == 2u ? b - cc : a - d) >> 3;
}

DG_HD int32_t vp8_avg3(int32_t a, int32_t b, int32_t c) { return (a + 2 * b + c + 2) >> 2; }
DG_HD int32_t vp8_avg2(int32_t a, int32_t b) { return (a + b + 1) >> 1; }
// Pixel (x, y) of a 4x4 sub-block from its edge E[13]: L K J I (left, bottom up), X (corner), A..H (above).
DG_HD int32_t vp8_pred4_px(uint32_t mode, uint32_t x, uint32_t y, const uint8_t *E) {
  switch (mode) {
    case VP8_B_DC: return (E[0] + E[1] + E[2] + E[3] + E[5] + E[6] + E[7] + E[8] + 4) >> 3;
    case VP8_B_TM: return vp8_clip8(E[5 + x] + E[3 - y] - E[4]);
    case VP8_B_VE: return vp8_avg3(E[4 + x], E[5 + x], E[6 + x]);
    case VP8_B_HE: return y < 3u ? vp8_avg3(E[4 - y], E[3 - y], E[2 - y]) : vp8_avg3(E[1], E[0], E[0]);
    case VP8_B_RD: {
      const uint32_t i = 3u - y + x;
      return vp8_avg3(E[i], E[i + 1], E[i + 2]);
    }
    case VP8_B_LD: {
      const uint32_t i = x + y;
      return vp8_avg3(E[5 + i], E[6 + i], E[i == 6u ? 12 : 7 + i]);
    }
    case VP8_B_VR: {
      if (x == 0u && y >= 2u) return y == 2u ? vp8_avg3(E[2], E[3], E[4]) : vp8_avg3(E[1], E[2], E[3]);
      const uint32_t xx = y >= 2u ? x - 1u : x;
      return (y & 1u) ? vp8_avg3(E[3 + xx], E[4 + xx], E[5 + xx]) : vp8_avg2(E[4 + xx], E[5 + xx]);
    }
    case VP8_B_VL: {
      if (x == 3u && y >= 2u) return y == 2u ? vp8_avg3(E[9], E[10], E[11]) : vp8_avg3(E[10], E[11], E[12]);
      const uint32_t i = 5u + x + (y >> 1);
      return (y & 1u) ? vp8_avg3(E[i], E[i + 1], E[i + 2]) : vp8_avg2(E[i], E[i + 1]);
    }
    case VP8_B_HD: {
      if (y == 0u && x >= 2u) return x == 2u ? vp8_avg3(E[4], E[5], E[6]) : vp8_avg3(E[5], E[6], E[7]);
      const uint32_t yy = x >= 2u ? y - 1u : y;
      return (x & 1u) ? vp8_avg3(E[3 - yy], E[4 - yy], E[5 - yy]) : vp8_avg2(E[3 - yy], E[4 - yy]);
    }
    default: {  // VP8_B_HU
      const uint32_t i = x + 2u * y, k = i >> 1;
      if (i >= 6u) return E[0];
      if (i & 1u) return vp8_avg3(E[3 - k], E[2 - k], E[k == 2u ? 0 : 1 - k]);
      return vp8_avg2(E[3 - k], E[2 - k]);
    }
  }
}

// Pixel (x, y) of an n x n block (16 or 8) from the buffer whose [0][0] is the corner; mx, my: the MB's
// place in the frame (the DC mode leaves out what lies outside it).  stride: the buffer's.
DG_HD int32_t vp8_pred_px(uint32_t mode, uint32_t n, uint32_t x, uint32_t y, const uint8_t *buf, uint32_t stride,
                          uint32_t mx, uint32_t my) {
  const uint8_t *top = buf + 1, *left = buf + stride;
  if (mode == VP8_V_PRED) return top[x];
  if (mode == VP8_H_PRED) return left[y * stride];
  if (mode == VP8_TM_PRED) return vp8_clip8(top[x] + left[y * stride] - buf[0]);
  const uint32_t sh = n == 16u ? 4u : 3u;
  int32_t st = 0, sl = 0;
  for (uint32_t k = 0; k < n; k++) {
    st += top[k];
    sl += left[k * stride];
  }
  if (mx && my) return (st + sl + (int32_t)n) >> (sh + 1u);
  if (my) return (st + (int32_t)(n >> 1)) >> sh;
  if (mx) return (sl + (int32_t)(n >> 1)) >> sh;
  return 128;
}

// One MB by one wave: the borders into B, prediction plus residual there, then out to the planes.
template <class E>
DG_HD void vp8_recon_mb(E &e, Vp8ReconBuf &B, const Vp8Layout &L, uint32_t mx, uint32_t my) {
  const uint32_t ys = L.mbw * 16u, uvs = L.mbw * 8u;
  const uint32_t mb = my * L.mbw + mx;
  const uint64_t rec = L.rec + (uint64_t)mb * kVp8RecBytes, coef = L.coef + (uint64_t)mb * kVp8CoefBytes;
  const uint32_t i4 = e.r8(rec + kVp8RecI4), uvm = e.r8(rec + kVp8RecUv);
  e.lanes([&](uint32_t lane) {
    for (uint32_t t = lane; t < 71u; t += 64u) {
      if (t < 21u) {  // the row above the luma: corner, 16, above-right 4
        const int32_t c = (int32_t)t - 1;
        uint32_t v = 127u;
        if (my) {
          const uint64_t r = L.y + (uint64_t)(16u * my - 1u) * ys + 16u * mx;
          if (c < 0)
            v = mx ? e.r8(r - 1u) : 129u;
          else if (c < 16 || mx + 1u < L.mbw)
            v = e.r8(r + (uint32_t)c);
          else
            v = e.r8(r + 15u);
        }
        B.y[0][t] = (uint8_t)v;
      } else if (t < 37u) {
        const uint32_t j = t - 21u;
        B.y[j + 1u][0] = (uint8_t)(mx ? e.r8(L.y + (uint64_t)(16u * my + j) * ys + 16u * mx - 1u) : 129u);
      } else {
        const uint32_t k = t - 37u, pl = k / 17u, q = k % 17u;  // per chroma plane: 9 above, 8 left
        const uint64_t P = pl ? L.v : L.u;
        uint8_t(*b)[12] = pl ? B.v : B.u;
        if (q < 9u) {
          uint32_t v = 127u;
          if (my) {
            const uint64_t r = P + (uint64_t)(8u * my - 1u) * uvs + 8u * mx;
            v = q ? e.r8(r + q - 1u) : mx ? e.r8(r - 1u) : 129u;
          }
          b[0][q] = (uint8_t)v;
        } else {
          const uint32_t j = q - 9u;
          b[j + 1u][0] = (uint8_t)(mx ? e.r8(P + (uint64_t)(8u * my + j) * uvs + 8u * mx - 1u) : 129u);
        }
      }
    }
  });
  if (i4) {
    e.lanes([&](uint32_t lane) {  // sub-block rows 1..3 see the MB's own above-right pixels
      if (lane < 12u) B.y[4u * (lane >> 2) + 4u][17u + (lane & 3u)] = B.y[0][17u + (lane & 3u)];
    });
    for (uint32_t d = 0; d < 10u; d++)  // sub-block (x, y) after (x-1, y), (x, y-1), (x+1, y-1): x + 2y = d
      e.lanes([&](uint32_t lane) {
        const uint32_t which = lane >> 4, px = lane & 3u, py = (lane >> 2) & 3u;
        const uint32_t y0 = d >= 3u ? (d - 2u) >> 1 : 0u;  // the first sub-block row on the diagonal
        const uint32_t by = y0 + which, bx = d - 2u * by;
        if (lane >= 32u || by > 3u || bx > 3u || 2u * by > d) return;
        const uint32_t k = 4u * by + bx;
        uint8_t ed[13];
        for (uint32_t i = 0; i < 4u; i++) ed[i] = B.y[4u * by + 4u - i][4u * bx];
        for (uint32_t i = 0; i < 9u; i++) ed[4u + i] = B.y[4u * by][4u * bx + i];
        int16_t c[16];
        for (uint32_t i = 0; i < 16u; i++) c[i] = (int16_t)e.r16(coef + 32u * k + 2u * i);
        const int32_t p = vp8_pred4_px(e.r8(rec + k), px, py, ed);
        B.y[4u * by + py + 1u][4u * bx + px + 1u] = (uint8_t)vp8_clip8(p + vp8_idct_px(c, py, px));
      });
  } else {
    const uint32_t ym = e.r8(rec);
    e.lanes([&](uint32_t lane) {  // the prediction reads the border only, so every pixel is free of the others
      for (uint32_t r = 0; r < 4u; r++) {
        const uint32_t i = lane + 64u * r, x = i & 15u, y = i >> 4, k = 4u * (y >> 2) + (x >> 2);
        int16_t c[16];
        for (uint32_t q = 0; q < 16u; q++) c[q] = (int16_t)e.r16(coef + 32u * k + 2u * q);
        const int32_t p = vp8_pred_px(ym, 16u, x, y, &B.y[0][0], 24u, mx, my);
        B.y[y + 1u][x + 1u] = (uint8_t)vp8_clip8(p + vp8_idct_px(c, y & 3u, x & 3u));
      }
    });
  }
  e.lanes([&](uint32_t lane) {
    for (uint32_t pl = 0; pl < 2u; pl++) {
      const uint32_t x = lane & 7u, y = lane >> 3, k = 16u + 4u * pl + 2u * (y >> 2) + (x >> 2);
      int16_t c[16];
      for (uint32_t q = 0; q < 16u; q++) c[q] = (int16_t)e.r16(coef + 32u * k + 2u * q);
      uint8_t(*b)[12] = pl ? B.v : B.u;
      const int32_t p = vp8_pred_px(uvm, 8u, x, y, &b[0][0], 12u, mx, my);
      b[y + 1u][x + 1u] = (uint8_t)vp8_clip8(p + vp8_idct_px(c, y & 3u, x & 3u));
    }
  });
  e.lanes([&](uint32_t lane) {  // out: a luma row is four lanes' dwords, a chroma row two
    {
      const uint32_t y = lane >> 2, x = 4u * (lane & 3u);
      const uint8_t *p = &B.y[y + 1u][x + 1u];
      e.w32(L.y + (uint64_t)(16u * my + y) * ys + 16u * mx + x, p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24));
    }
    if (lane < 32u) {
      const uint32_t pl = lane >> 4, y = (lane >> 1) & 7u, x = 4u * (lane & 1u);
      const uint8_t *p = pl ? &B.v[y + 1u][x + 1u] : &B.u[y + 1u][x + 1u];
      e.w32((pl ? L.v : L.u) + (uint64_t)(8u * my + y) * uvs + 8u * mx + x,
            p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24));
    }
  });
}

// The MBs of anti-diagonal d (x + 2y = d) of an mbw x mbh frame: rows y0 .. y0 + n - 1.
DG_HD uint32_t vp8_diag_count(uint32_t mbw, uint32_t mbh) { return mbw + 2u * (mbh - 1u); }
DG_HD void vp8_diag_rows(uint32_t mbw, uint32_t mbh, uint32_t d, uint32_t &y0, uint32_t &n) {
  y0 = d >= mbw ? (d - mbw + 2u) >> 1 : 0u;
  const uint32_t y1 = (d >> 1) < mbh - 1u ? (d >> 1) : mbh - 1u;
  n = y1 >= y0 ? y1 - y0 + 1u : 0u;
}

// ------------------------------------------------------------ the loop filter (k_vp8_filter)

DG_HD int32_t vp8_sc1(int32_t v) { return v < -128 ? -128 : v > 127 ? 127 : v; }
DG_HD int32_t vp8_sc2(int32_t v) { return v < -16 ? -16 : v > 15 ? 15 : v; }

// One position of an edge: p is the arena offset of q0, s the step across the edge.
// kind 0: simple filter, 1: MB edge, 2: inner edge.
template <class E>
DG_HD void vp8_filter_at(E &e, uint64_t p, uint32_t s, uint32_t kind, int32_t thresh, int32_t ithresh, int32_t hevt) {
  const int32_t p1 = e.r8(p - 2u * s), p0 = e.r8(p - s), q0 = e.r8(p), q1 = e.r8(p + s);
  if (4 * vp8_abs(p0 - q0) + vp8_abs(p1 - q1) > 2 * thresh + 1) return;
  if (kind == 0u) {
    const int32_t a = 3 * (q0 - p0) + vp8_sc1(p1 - q1);
    e.w8(p - s, (uint32_t)vp8_clip8(p0 + vp8_sc2((a + 3) >> 3)));
    e.w8(p, (uint32_t)vp8_clip8(q0 - vp8_sc2((a + 4) >> 3)));
    return;
  }
  const int32_t p3 = e.r8(p - 4u * s), p2 = e.r8(p - 3u * s), q2 = e.r8(p + 2u * s), q3 = e.r8(p + 3u * s);
  if (vp8_abs(p3 - p2) > ithresh || vp8_abs(p2 - p1) > ithresh || vp8_abs(p1 - p0) > ithresh || vp8_abs(q3 - q2) > ithresh ||
      vp8_abs(q2 - q1) > ithresh || vp8_abs(q1 - q0) > ithresh)
    return;
  if (vp8_abs(p1 - p0) > hevt || vp8_abs(q1 - q0) > hevt) {
    const int32_t a = 3 * (q0 - p0) + vp8_sc1(p1 - q1);
    e.w8(p - s, (uint32_t)vp8_clip8(p0 + vp8_sc2((a + 3) >> 3)));
    e.w8(p, (uint32_t)vp8_clip8(q0 - vp8_sc2((a + 4) >> 3)));
  } else if (kind == 1u) {
    const int32_t a = vp8_sc1(3 * (q0 - p0) + vp8_sc1(p1 - q1));
    const int32_t a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
    e.w8(p - 3u * s, (uint32_t)vp8_clip8(p2 + a3));
    e.w8(p - 2u * s, (uint32_t)vp8_clip8(p1 + a2));
    e.w8(p - s, (uint32_t)vp8_clip8(p0 + a1));
    e.w8(p, (uint32_t)vp8_clip8(q0 - a1));
    e.w8(p + s, (uint32_t)vp8_clip8(q1 - a2));
    e.w8(p + 2u * s, (uint32_t)vp8_clip8(q2 - a3));
  } else {
    const int32_t a = 3 * (q0 - p0);
    const int32_t a1 = vp8_sc2((a + 4) >> 3), a2 = vp8_sc2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
    e.w8(p - 2u * s, (uint32_t)vp8_clip8(p1 + a3));
    e.w8(p - s, (uint32_t)vp8_clip8(p0 + a2));
    e.w8(p, (uint32_t)vp8_clip8(q0 - a1));
    e.w8(p + s, (uint32_t)vp8_clip8(q1 - a3));
  }
}

// One MB by one wave, in libwebp's order: left MB edge, inner vertical edges, top MB edge, inner
// horizontal edges; an edge's positions go to lanes 0..15 (luma), 16..23 (U), 24..31 (V).
template <class E>
DG_HD void vp8_filter_mb(E &e, const Vp8Layout &L, uint32_t filter_type, uint32_t mx, uint32_t my) {
  const uint32_t ys = L.mbw * 16u, uvs = L.mbw * 8u;
  const uint64_t rec = L.rec + (uint64_t)(my * L.mbw + mx) * kVp8RecBytes;
  const int32_t limit = (int32_t)e.r8(rec + kVp8RecLimit), ilevel = (int32_t)e.r8(rec + kVp8RecIlevel);
  const int32_t hevt = (int32_t)e.r8(rec + kVp8RecHev);
  const uint32_t inner = e.r8(rec + kVp8RecInner);
  if (limit == 0) return;
  const bool simple = filter_type == 1u;
  const uint64_t yp = L.y + (uint64_t)16u * my * ys + 16u * mx;
  const uint64_t up = L.u + (uint64_t)8u * my * uvs + 8u * mx, vp = L.v + (uint64_t)8u * my * uvs + 8u * mx;
  for (uint32_t step = 0; step < 8u; step++) {
    const bool horiz = step < 4u;       // the filter runs across a vertical edge
    const uint32_t k = step & 3u;       // 0: the MB edge, 1..3: inner edges at 4 k
    if (k == 0u ? (horiz ? mx == 0u : my == 0u) : !inner) continue;
    const int32_t th = k == 0u ? limit + 4 : limit;
    const uint32_t kind = simple ? 0u : k == 0u ? 1u : 2u;
    e.lanes([&](uint32_t lane) {
      if (lane < 16u) {
        const uint64_t p = horiz ? yp + 4u * k + (uint64_t)lane * ys : yp + (uint64_t)4u * k * ys + lane;
        vp8_filter_at(e, p, horiz ? 1u : ys, kind, th, ilevel, hevt);
      } else if (lane < 32u && !simple && k < 2u) {
        const uint32_t i = lane & 7u;
        const uint64_t b = lane < 24u ? up : vp;
        const uint64_t p = horiz ? b + 4u * k + (uint64_t)i * uvs : b + (uint64_t)4u * k * uvs + i;
        vp8_filter_at(e, p, horiz ? 1u : uvs, kind, th, ilevel, hevt);
      }
    });
  }
}

// ------------------------------------------------------------ upsampling and colour (k_vp8_rgb)

DG_HD uint32_t vp8_yuv_clip(int32_t v) { return (v & ~16383) == 0 ? (uint32_t)(v >> 6) : v < 0 ? 0u : 255u; }
// libwebp's fancy upsampling: 9-3-3-1 over the nearest and the next chroma sample each way, rounded in two stages
DG_HD int32_t vp8_up(int32_t a, int32_t b, int32_t c, int32_t d) { return (((a + 3 * b + 3 * c + d + 8) >> 3) + a) >> 1; }
// Pixel (x, y) of a w x h frame as R | G << 8 | B << 16.
template <class E>
DG_HD uint32_t vp8_rgb_px(E &e, const Vp8Layout &L, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
  const uint32_t ys = L.mbw * 16u, uvs = L.mbw * 8u, cw = (w + 1u) >> 1, ch = (h + 1u) >> 1;
  const uint32_t nr = y >> 1, nc = x >> 1;
  const uint32_t fr = (y & 1u) ? (nr + 1u < ch ? nr + 1u : ch - 1u) : (nr ? nr - 1u : 0u);
  const uint32_t fc = (x & 1u) ? (nc + 1u < cw ? nc + 1u : cw - 1u) : (nc ? nc - 1u : 0u);
  const uint64_t a = (uint64_t)nr * uvs + nc, b = (uint64_t)nr * uvs + fc, c = (uint64_t)fr * uvs + nc, d = (uint64_t)fr * uvs + fc;
  const int32_t u = vp8_up(e.r8(L.u + a), e.r8(L.u + b), e.r8(L.u + c), e.r8(L.u + d));
  const int32_t v = vp8_up(e.r8(L.v + a), e.r8(L.v + b), e.r8(L.v + c), e.r8(L.v + d));
  const int32_t yy = ((int32_t)e.r8(L.y + (uint64_t)y * ys + x) * 19077) >> 8;
  const uint32_t R = vp8_yuv_clip(yy + ((v * 26149) >> 8) - 14234);
  const uint32_t G = vp8_yuv_clip(yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708);
  const uint32_t Bl = vp8_yuv_clip(yy + ((u * 33050) >> 8) - 17685);
  return R | (G << 8) | (Bl << 16);
}

}  // namespace dg
