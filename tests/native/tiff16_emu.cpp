// tiff16_emu.cpp — the TIFF header walk with deep = true (option "tiff16") and the tiff16_* lane routines of
// dg_tiff.h on the CPU, one group of four pixels at a time.  A stand-alone program:
//   tiff16_emu in.tif out.raw   prints "status | why"; a file that decodes leaves native-endian uint16 in out.raw
#define main tiff_emu_main  // the segment decoders of the 8-bit program (lzw, packbits), as they are
#include "tiff_emu.cpp"
#undef main

// One row piece as the lanes of k_tiff_expand16 take it: four pixels = 2 x spp dwords, two samples to a dword.
static void row16(const uint8_t *src, uint16_t *dst, uint32_t npx, uint32_t spp, bool pred, bool swap) {
  uint32_t carry[2] = {0, 0};
  for (uint32_t x0 = 0; x0 < npx; x0 += 4) {
    const uint32_t ns = (npx - x0 < 4u ? npx - x0 : 4u) * spp;
    const uint8_t *b = src + 2 * (size_t)x0 * spp;
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, p[4][2];
    for (uint32_t j = 0; j < ns; j++) v[j >> 1] |= ((uint32_t)b[2 * j] | (uint32_t)b[2 * j + 1] << 8) << (16 * (j & 1));
    for (uint32_t k = 0; swap && k < 2 * spp; k++) v[k] = tiff16_swap(v[k]);
    for (uint32_t t = 0; pred && t < 4; t++)
      for (uint32_t k = 0; k < 2; k++) p[t][k] = k < (spp + 1) / 2 ? carry[k] = tiff16_hadd(tiff16_px(v, t, k, spp), carry[k]) : 0u;
    for (uint32_t m = 0; pred && m < 2 * spp; m++) v[m] = tiff16_pack(p, m, spp);
    for (uint32_t j = 0; j < ns; j++) dst[x0 * spp + j] = (uint16_t)tiff16_at(v, j);
  }
}

int main(int argc, char **argv) {
  Bytes f;
  FILE *fp = argc == 3 ? fopen(argv[1], "rb") : nullptr;
  if (!fp) return 2;
  for (int c; (c = fgetc(fp)) != EOF;) f.push_back((uint8_t)c);
  fclose(fp);
  TiffHeader h;
  parse_tiff_header(f.data(), f.size(), h, false, true);
  int status = h.status ? h.status : h.bits != 16;
  const uint32_t spp = (uint32_t)h.out_c;
  std::vector<uint16_t> pix(status ? 0 : (size_t)h.width * h.height * spp);
  std::vector<Bytes> dec(status ? 0 : h.segs.size());
  for (size_t s = 0; s < dec.size() && !status; s++) {
    const TiffSegment &g = h.segs[s];
    dec[s].assign(f.data() + g.off, f.data() + g.off + (h.compression == TIFF_NONE ? g.dec : 0));
    dec[s].resize(g.dec);
    if (h.compression != TIFF_NONE && (h.compression == TIFF_LZW ? lzw : packbits)(f.data() + g.off, g.nbytes, dec[s])) status = 2;
  }
  for (uint32_t pc = 0; !status && pc < h.height * h.across; pc++) {
    const TiffPiece p = tiff_piece(pc, h.width, 2 * spp, h.seg_w, h.seg_h, h.across);
    row16(dec[p.seg].data() + p.off, pix.data() + ((size_t)p.y * h.width + p.px0) * spp, p.npx, spp, h.predictor == 2, h.swap);
  }
  if (FILE *fo = status ? nullptr : fopen(argv[2], "wb")) fwrite(pix.data(), 2, pix.size(), fo), fclose(fo);
  printf("%d | %s\n", status, h.status ? h.why : status ? "TIFF: segment does not decode" : "");
  return 0;
}
