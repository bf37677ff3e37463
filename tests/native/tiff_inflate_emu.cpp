// tiff_inflate_emu.cpp — the admitting TIFF header walk and the lane routines of dg_tiff_inflate.h on the CPU:
// the 64 lanes of a token step and of a code-length round one after the other, the rest serially.
//   tiff_inflate_emu in.tif out.raw   prints "status tokens steps | why"; writes a decoded file's pixels to out.raw
// A segment that does not decode gives status 2 and the kTiffFail* code in the text, as the kernel reports it.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "dg_tiff.h"
#include "dg_tiff_inflate.h"
#include "host/tiff_header.h"

using namespace dg;
typedef std::vector<uint8_t> Bytes;
static unsigned long g_tokens, g_steps;

struct Src {
  const uint8_t *s;
  uint32_t nbytes;
  uint64_t fetch(uint32_t bp) const {  // 64 bits from bit bp; bytes past the end read as zero
    unsigned __int128 v = 0;
    for (uint32_t k = 0; k < 9; k++) v |= (unsigned __int128)((bp >> 3) + k < nbytes ? s[(bp >> 3) + k] : 0) << (8 * k);
    return (uint64_t)(v >> (bp & 7));
  }
};
struct Code {
  uint16_t cnt[16], sym[320];
  uint32_t ncodes;
  int32_t left;
  void build(const uint8_t *lens, uint32_t n) {  // canonical form, as tinf_build leaves it
    memset(cnt, 0, sizeof(cnt));
    for (uint32_t s = 0; s < n; s++) cnt[lens[s]]++;
    cnt[0] = 0, ncodes = 0, left = 1;
    for (uint32_t l = 1; l < 16 && left >= 0; l++) left = (left << 1) - cnt[l];
    for (uint32_t l = 1; l < 16; l++)
      for (uint32_t s = 0; s < n; s++)
        if (lens[s] == l) sym[ncodes++] = (uint16_t)s;
  }
};

// One Deflate segment: 0, or the kTiffFail* the kernel reports.
static uint32_t inflate_seg(const uint8_t *s, uint32_t nbytes, Bytes &out) {
  const Src in{s, nbytes};
  const uint32_t nbits = nbytes * 8u, dec = (uint32_t)out.size();
  std::vector<uint32_t> ll(kTinfLlSize), dd(kTinfDdSize);
  Code lc, dc, cc;
  uint8_t lens[320], cllens[19], cltab[kTinfClSize];
  TinfTabs T = {ll.data(), dd.data(), lc.cnt, lc.sym, dc.cnt, dc.sym, {0, 0}, {0, 0}};
  uint32_t bitpos = 16, o = 0, bfinal = 0, trailer = 0xFFFFFFFFu;
  bool in_block = false, exact = false;
  if (nbytes < 2) return kTiffFailShort;
  if (!tinf_zlib_ok(s[0], s[1])) return kTiffFailStream;
  while (o < dec) {
    if (!in_block) {
      if (bfinal || bitpos + 3 > nbits) return kTiffFailShort;
      const uint32_t hb = (uint32_t)in.fetch(bitpos), type = (hb >> 1) & 3;
      bfinal = hb & 1, bitpos += 3;
      if (type == 3) return kTiffFailStream;
      if (type == 0) {
        const uint32_t k = (bitpos + 7) >> 3;
        if (k + 4 > nbytes) return kTiffFailShort;
        const uint32_t len = s[k] | (s[k + 1] << 8), nlen = s[k + 2] | (s[k + 3] << 8);
        if (len != (nlen ^ 0xFFFFu)) return kTiffFailStream;
        const uint32_t want = len < dec - o ? len : dec - o;
        if (k + 4 + want > nbytes) return kTiffFailShort;
        memcpy(out.data() + o, s + k + 4, want);
        o += want, bitpos = 8 * (k + 4 + len);
        if (o == dec && want == len && bfinal) trailer = k + 4 + len;
        continue;
      }
      uint32_t nl = 288, nd = 32;
      if (type == 1) {
        for (uint32_t i = 0; i < 320; i++) lens[i] = (uint8_t)(i < 288 ? tinf_fixed_len(i) : 5);
      } else {
        if (bitpos + 14 > nbits) return kTiffFailShort;
        const uint32_t hd = (uint32_t)in.fetch(bitpos), ncl = 4 + ((hd >> 10) & 15);
        nl = 257 + (hd & 31), nd = 1 + ((hd >> 5) & 31), bitpos += 14;
        if (nl > kTinfMaxLl || nd > kTinfMaxDd) return kTiffFailStream;
        if (bitpos + 3 * ncl > nbits) return kTiffFailShort;
        memset(cllens, 0, sizeof(cllens));
        for (uint32_t i = 0; i < ncl; i++) cllens[tinf_cl_order(i)] = (uint8_t)(in.fetch(bitpos + 3 * i) & 7);
        bitpos += 3 * ncl;
        cc.build(cllens, 19);
        if (cc.left != 0) return kTiffFailStream;
        for (uint32_t i = 0; i < kTinfClSize; i++) {
          const uint32_t w = tinf_walk(i, cc.cnt, cc.sym, 0, TinfWalk{0, 0}, kTinfClBits);
          cltab[i] = (uint8_t)(w ? ((w >> 16) << 5) | (w & 31) : 0);
        }
        for (uint32_t n = 0, prev = 0, total = nl + nd; n < total;) {  // rounds of 64 bit offsets
          uint32_t tk[64], cur = 0;
          for (uint32_t lane = 0; lane < 64; lane++) tk[lane] = tinf_cl_token((uint32_t)in.fetch(bitpos + lane), cltab);
          for (; cur < 64 && n < total;) {
            const uint32_t t = tk[cur], nb = t & 255, rep = (t >> 8) & 255, sy = t >> 16;
            if (bitpos + cur + nb > nbits) return kTiffFailShort;
            if (!t || (sy == 16 && n == 0) || n + rep > total) return kTiffFailStream;
            const uint32_t v = sy < 16 ? sy : sy == 16 ? prev : 0;
            memset(lens + n, (int)v, rep);
            n += rep, prev = v, cur += nb;
          }
          bitpos += cur;
        }
        if (lens[256] == 0) return kTiffFailStream;
      }
      lc.build(lens, nl);
      dc.build(lens + nl, nd);
      if (!tinf_set_ok(lc.left, lc.ncodes, lc.cnt[1], true) || !tinf_set_ok(dc.left, dc.ncodes, dc.cnt[1], true)) return kTiffFailStream;
      for (uint32_t i = 0; i < kTinfLlSize; i++) ll[i] = tinf_primary(i, lc.cnt, lc.sym, kTinfLlBits, false);
      for (uint32_t i = 0; i < kTinfDdSize; i++) dd[i] = tinf_primary(i, dc.cnt, dc.sym, kTinfDdBits, true);
      T.lw = tinf_walk_from(lc.cnt, kTinfLlBits), T.dw = tinf_walk_from(dc.cnt, kTinfDdBits);
      in_block = true;
      continue;
    }
    // ---- a token step: 64 lanes decode, the starts are found by hopping, the taken tokens run in order
    TinfTok t[64];
    for (uint32_t lane = 0; lane < 64; lane++) {
      t[lane] = tinf_token(in.fetch(bitpos + lane), T);
      if (bitpos + lane + t[lane].nb > nbits) t[lane].kind = kTinfPast;
    }
    g_steps++;
    uint32_t cur = 0, end = bitpos;
    for (; cur < 64 && o < dec; cur += t[cur].nb) {
      const TinfTok &k = t[cur];
      if (k.kind == kTinfPast) return kTiffFailShort;
      if (k.kind == kTinfBad || (k.kind == kTinfMatch && k.dist > o)) return kTiffFailStream;
      if (k.kind == kTinfEob) break;
      const uint32_t n = k.kind == kTinfLit ? 1 : k.val, cl = n < dec - o ? n : dec - o;
      for (uint32_t q = 0; q < cl; q++) out[o + q] = k.kind == kTinfLit ? (uint8_t)k.val : out[o - k.dist + tinf_src(q, k.dist, cl)];
      exact = o + n == dec;
      o += cl, end = bitpos + cur + k.nb, g_tokens++;
    }
    bitpos = end;
    if (o < dec && cur < 64) bitpos += t[cur].nb, in_block = false;  // (only an end-of-block code stops a step short of the last byte)
  }
  if (in_block && bfinal && exact) {
    const TinfTok k = tinf_token(in.fetch(bitpos), T);
    if (k.kind == kTinfEob && bitpos + k.nb <= nbits) trailer = (bitpos + k.nb + 7) >> 3;
  }
  if (trailer != 0xFFFFFFFFu && trailer + 4 <= nbytes) {
    uint32_t a = 0, b = 0;
    for (uint32_t i = 0; i < dec; i += 4) {
      uint32_t v = 0;
      for (uint32_t q = 0; q < 4 && i + q < dec; q++) v |= (uint32_t)out[i + q] << (8 * q);
      tinf_adler4(v, dec - i, (dec - i) % kTinfAdlerMod, a, b);
    }
    const uint32_t sum = (((dec + b) % kTinfAdlerMod) << 16) | ((1 + a) % kTinfAdlerMod);
    const uint8_t *tp = s + trailer;
    if (sum != (((uint32_t)tp[0] << 24) | (tp[1] << 16) | (tp[2] << 8) | tp[3])) return kTiffFailSum;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  Bytes f(1 << 24);  // (the tests' files are far smaller)
  FILE *fp = fopen(argv[1], "rb");
  f.resize(fp ? fread(f.data(), 1, f.size(), fp) : 0);
  if (fp) fclose(fp);
  TiffHeader h;
  parse_tiff_header(f.data(), f.size(), h, true);
  int status = h.status;
  char text[64];
  const char *why = h.why;
  const uint32_t spp = (uint32_t)h.out_c;
  if (!status && h.compression != TIFF_DEFLATE) status = 1, why = "not a Deflate TIFF";
  std::vector<Bytes> dec(h.segs.size());
  for (size_t s = 0; s < h.segs.size() && !status; s++) {
    dec[s].assign(h.segs[s].dec, 0);
    if (const uint32_t fl = inflate_seg(f.data() + h.segs[s].off, h.segs[s].nbytes, dec[s])) {
      snprintf(text, sizeof(text), "segment does not decode: fail %u", fl);
      status = 2, why = text;
    }
  }
  FILE *fo = status ? nullptr : fopen(argv[2], "wb");
  if (fo) {  // rows and tiles in place, predictor 2 undone
    Bytes pix((size_t)h.width * h.height * spp);
    for (uint32_t pc = 0; pc < h.height * h.across; pc++) {
      const TiffPiece p = tiff_piece(pc, h.width, spp, h.seg_w, h.seg_h, h.across);
      const uint8_t *src = dec[p.seg].data() + p.off;
      uint8_t *dst = pix.data() + ((size_t)p.y * h.width + p.px0) * spp;
      for (uint32_t k = 0; k < p.npx * spp; k++) dst[k] = (uint8_t)(src[k] + (h.predictor == 2 && k >= spp ? dst[k - spp] : 0));
      for (uint32_t k = 0; h.invert && k < p.npx * spp; k++) dst[k] ^= 0xFF;
    }
    fwrite(pix.data(), 1, pix.size(), fo);
    fclose(fo);
  }
  printf("%d %lu %lu | %s\n", status, g_tokens, g_steps, why);
  return 0;
}
