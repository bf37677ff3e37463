// tiff_emu.cpp — the TIFF header walk (host/tiff_header.cpp) and the lane routines of dg_tiff.h on the CPU,
// one code, header or pixel group at a time.  A stand-alone program:
//   tiff_emu in.tif out.raw   prints "status | why" and, for a file that decodes, writes its pixels to out.raw
// A segment that does not decode gives the status the kernels give: 2, or 1 for a table that stays full.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dg_tiff.h"
#include "host/tiff_header.h"

using namespace dg;
typedef std::vector<uint8_t> Bytes;

// One LZW segment: 0, or the kTiffFail* the kernel reports.
static uint32_t lzw(const uint8_t *s, uint32_t nbytes, Bytes &out) {
  std::vector<uint32_t> tpos(kGifMaxCodes), tlen(kGifMaxCodes);
  uint32_t bitpos = 0, nf = kTiffFirst, pv = 0, ppos = 0, plen = 0, o = 0, fullc = 0;
  for (const uint32_t n = (uint32_t)out.size(); o < n;) {
    const uint32_t w = tiff_width(nf), k = bitpos >> 3;
    if (bitpos + w > nbytes * 8u) return kTiffFailShort;
    const uint32_t c = tiff_code(s[k], k + 1 < nbytes ? s[k + 1] : 0u, k + 2 < nbytes ? s[k + 2] : 0u, bitpos, w);
    bitpos += w;
    if (c == kTiffEnd) return kTiffFailShort;
    if (c == kTiffClear) {
      nf = kTiffFirst, pv = 0, fullc = 0;
      continue;
    }
    const uint32_t a = pv ? 0u : 1u;
    if (gif_code_bad(c, nf, 0, a)) return kTiffFailCode;
    if (nf == kGifMaxCodes && ++fullc > kTiffFullCodes) return kTiffFailFull;
    const bool lit = c < kTiffClear, kw = !lit && c == nf;
    const uint32_t L = lit ? 1u : kw ? plen + 1u : tlen[c], S = kw ? ppos : lit ? 0u : tpos[c];
    for (uint32_t t = 0; t < L && o + t < n; t++) out[o + t] = lit ? (uint8_t)c : out[S + gif_copy_index(t, L, kw)];
    if (pv && nf < kGifMaxCodes) tpos[nf] = ppos, tlen[nf] = plen + 1u;
    nf = gif_lane_nf(nf, a, 1);
    pv = 1, ppos = o, plen = L, o += L;
  }
  return 0;
}

static uint32_t packbits(const uint8_t *s, uint32_t nbytes, Bytes &out) {
  for (uint32_t pos = 0, o = 0, n = (uint32_t)out.size(); o < n;) {
    if (pos >= nbytes || pos + tiff_pb_size(s[pos]) > nbytes) return kTiffFailShort;
    const uint32_t h = s[pos], c = tiff_pb_out(h);
    for (uint32_t t = 0; t < c && o + t < n; t++) out[o + t] = h > 128u ? s[pos + 1] : s[pos + 1 + t];
    o += c, pos += tiff_pb_size(h);
  }
  return 0;
}

// One row piece, four pixels at a time as a lane of k_tiff_expand takes them.
static void row(const uint8_t *src, uint8_t *dst, uint32_t npx, uint32_t spp, bool pred, uint32_t inv) {
  for (uint32_t x0 = 0, carry = 0; x0 < npx; x0 += 4) {
    const uint32_t nb = (npx - x0 < 4u ? npx - x0 : 4u) * spp;
    uint32_t v[4] = {0, 0, 0, 0}, p[4];
    for (uint32_t k = 0; k < nb; k++) v[k >> 2] |= (uint32_t)src[x0 * spp + k] << (8 * (k & 3));
    for (uint32_t t = 0; t < 4; t++) {
      p[t] = tiff_px(v, t, spp);
      if (pred) carry = p[t] = tiff_badd(p[t], carry);
      p[t] ^= inv;
    }
    for (uint32_t k = 0; k < nb; k++) dst[x0 * spp + k] = (uint8_t)(tiff_pack(p, k >> 2, spp) >> (8 * (k & 3)));
  }
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  Bytes f;
  if (FILE *fp = fopen(argv[1], "rb")) {
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), fp)) > 0;) f.insert(f.end(), buf, buf + k);
    fclose(fp);
  }
  TiffHeader h;
  parse_tiff_header(f.data(), f.size(), h);
  int status = h.status;
  const char *why = h.why;
  const uint32_t spp = (uint32_t)h.out_c, inv = h.invert ? 0xFFu : 0u;
  std::vector<Bytes> dec(h.segs.size());
  for (size_t s = 0; s < h.segs.size() && !status; s++) {
    const TiffSegment &g = h.segs[s];
    dec[s].assign(g.dec, 0);
    uint32_t fl = 0;
    if (h.compression == TIFF_NONE)
      memcpy(dec[s].data(), f.data() + g.off, g.dec);
    else
      fl = h.compression == TIFF_LZW ? lzw(f.data() + g.off, g.nbytes, dec[s]) : packbits(f.data() + g.off, g.nbytes, dec[s]);
    if (fl) status = fl == kTiffFailFull ? 1 : 2, why = "segment does not decode";
  }
  if (!status) {
    Bytes pix((size_t)h.width * h.height * spp);
    for (uint32_t pc = 0; pc < h.height * h.across; pc++) {
      const TiffPiece p = tiff_piece(pc, h.width, spp, h.seg_w, h.seg_h, h.across);
      row(dec[p.seg].data() + p.off, pix.data() + ((size_t)p.y * h.width + p.px0) * spp, p.npx, spp, h.predictor == 2, inv);
    }
    if (FILE *fo = fopen(argv[2], "wb")) {
      fwrite(pix.data(), 1, pix.size(), fo);
      fclose(fo);
    }
  }
  printf("%d | %s\n", status, why);
  return 0;
}
