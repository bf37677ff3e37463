// tiff_g4_emu.cpp — the TIFF header walk with bilevel = true (option "tiff_bilevel") and the lane routines of
// dg_tiff_g4.h on the CPU: the 64 lanes of a step decode their tokens one after the other, then the real tokens
// are resolved one at a time (no batched V0 path: that is the kernel's own).  A stand-alone program:
//   tiff_g4_emu in.tif out.raw   prints "status tokens steps | why"; a file that decodes leaves L8 of 0 / 255 in out.raw
#define main tiff_emu_main  // the segment decoders of the 8-bit program (lzw, packbits), as they are
#include "tiff_emu.cpp"
#undef main
#include "dg_tiff_g4.h"

static unsigned long g_tokens, g_steps;

// The first changing element of `ref` at or right of `from` (sel as in the kernel's g4_find); W if there is none.
static uint32_t find(const uint32_t *ref, uint32_t nwords, uint32_t W, uint32_t from, uint32_t sel) {
  for (uint32_t i = from >> 5; i < nwords; i++) {
    const uint32_t r = ref[i], t = g4_trans(r, ref[(int)i - 1]);
    uint32_t m = sel == 0 ? t : sel == 1 ? t & r : t & ~r;
    if (i == from >> 5) m &= ~0u << (from & 31);
    if (m) return 32 * i + g4_nth(m, 0) < W ? 32 * i + g4_nth(m, 0) : W;
  }
  return W;
}

// One Group 4 segment into rows of ceil(W / 8) bytes: false where the kernel gives kTiffFailG4.
static bool g4(const uint8_t *s, uint32_t nbytes, uint32_t W, Bytes &out) {
  std::vector<uint16_t> tab(kG4TabSize, 0);
  for (uint32_t i = 0; i < kG4Codes; i++) g4_fill(&tab[0], &tab[kG4WhiteSize], &tab[kG4WhiteSize + kG4Black1Size], i);
  const G4Tabs T = {&tab[0], &tab[kG4WhiteSize], &tab[kG4WhiteSize + kG4Black1Size]};
  auto byte = [&](uint32_t k) -> uint32_t { return k < nbytes ? s[k] : 0u; };
  auto peek = [&](uint32_t pos) -> uint64_t {
    uint32_t d[3];
    for (uint32_t k = 0; k < 3; k++) d[k] = byte((pos >> 3) + 4 * k) | byte((pos >> 3) + 4 * k + 1) << 8 | byte((pos >> 3) + 4 * k + 2) << 16 | byte((pos >> 3) + 4 * k + 3) << 24;
    return g4_window(d[0], d[1], d[2], pos & 7);
  };
  const uint32_t nwords = (W + 31) / 32, rowb = (W + 7) / 8, nrows = (uint32_t)out.size() / rowb, nbits = nbytes * 8;
  std::vector<uint32_t> rows[2] = {std::vector<uint32_t>(nwords + 2, 0), std::vector<uint32_t>(nwords + 2, 0)};
  uint32_t bitpos = 0, a0 = 0, colour = 0, rdone = 0, cb = 0;
  bool start = true;
  while (rdone < nrows) {
    G4Tok tok[64];
    for (uint32_t j = 0; j < 64; j++) tok[j] = g4_token(T, peek(bitpos + j));
    g_steps++;
    uint32_t p = 0;
    while (p < 64 && rdone < nrows) {
      uint32_t *cur = &rows[cb][1];
      const uint32_t *ref = &rows[cb ^ 1][1];
      const uint32_t from = start ? 0 : a0 + 1, md = tok[p].mode, kind = md & 15;
      uint32_t used = (md >> 4) & 15, x0 = a0, x1 = a0;
      if (kind == kG4Bad || bitpos + p + used > nbits) return false;
      if (kind == kG4V) {
        const int a1 = (int)find(ref, nwords, W, from, colour ? 2 : 1) + (int)(md >> 8) - 3;
        if (a1 < (int)a0 || a1 > (int)W) return false;
        x1 = colour ? (uint32_t)a1 : a0;
        a0 = (uint32_t)a1;
        colour ^= 1;
      } else if (kind == kG4P) {
        const uint32_t b1 = find(ref, nwords, W, from, colour ? 2 : 1);
        if (b1 >= W) return false;
        const uint32_t b2 = find(ref, nwords, W, b1 + 1, 0);
        x1 = colour ? b2 : a0;
        a0 = b2;
      } else {
        uint32_t hy = tok[p].h[colour], r1 = hy & 4095, r2 = (hy >> 12) & 4095;
        used = (hy >> 24) & 127;
        if (hy == kG4Slow) {
          uint32_t pos = bitpos + p + 3;
          if (!g4_run_slow(T, peek, &pos, colour, &r1) || !g4_run_slow(T, peek, &pos, colour ^ 1, &r2)) hy = 0;
          used = pos - bitpos - p;
        }
        if (hy == 0 || bitpos + p + used > nbits || a0 + r1 + r2 > W) return false;
        x0 = colour ? a0 : a0 + r1;
        x1 = colour ? a0 + r1 : a0 + r1 + r2;
        a0 += r1 + r2;
      }
      start = false;
      for (uint32_t i = x0 >> 5; x1 > x0 && i <= (x1 - 1) >> 5; i++) cur[i] |= g4_span(i, x0, x1);
      p += used;
      g_tokens++;
      if (a0 < W) continue;
      for (uint32_t k = 0; k < rowb; k++) out[(size_t)rdone * rowb + k] = (uint8_t)(g4_out(cur[k >> 2]) >> (8 * (k & 3)));
      cb ^= 1;
      std::fill(rows[cb].begin(), rows[cb].end(), 0u);
      a0 = 0, colour = 0, start = true, rdone++;
    }
    bitpos += p;
  }
  return true;
}

int main(int argc, char **argv) {
  Bytes f;
  FILE *fp = argc == 3 ? fopen(argv[1], "rb") : nullptr;
  if (!fp) return 2;
  for (int c; (c = fgetc(fp)) != EOF;) f.push_back((uint8_t)c);
  fclose(fp);
  TiffHeader h;
  parse_tiff_header(f.data(), f.size(), h, false, false, true);
  int status = h.status ? h.status : h.bits != 1;
  const char *why = h.status ? h.why : "";
  const uint32_t rowb = (h.seg_w + 7) / 8, inv = h.invert ? ~0u : 0u;
  std::vector<Bytes> dec(status ? 0 : h.segs.size());
  for (size_t s = 0; s < dec.size() && !status; s++) {
    const TiffSegment &g = h.segs[s];
    dec[s].assign(f.data() + g.off, f.data() + g.off + (h.compression == TIFF_NONE ? g.dec : 0));
    dec[s].resize(g.dec);
    if (h.compression == TIFF_G4) {
      if (!g4(f.data() + g.off, g.nbytes, h.seg_w, dec[s])) status = 1, why = "TIFF: irregular Group 4 stream";
    } else if (h.compression != TIFF_NONE && (h.compression == TIFF_LZW ? lzw : packbits)(f.data() + g.off, g.nbytes, dec[s])) {
      status = 2, why = "TIFF: segment does not decode";
    }
  }
  Bytes pix(status ? 0 : (size_t)h.width * h.height);
  for (uint32_t pc = 0; !status && pc < h.height * h.across; pc++) {  // a row piece as k_tiff_expand1 takes it, four pixels at a time
    const TiffPiece p = tiff_piece(pc, h.width, 1, h.seg_w, h.seg_h, h.across);
    const uint8_t *row = dec[p.seg].data() + (size_t)(p.y % h.seg_h) * rowb;
    for (uint32_t x = 0; x < p.npx; x++)
      pix[(size_t)p.y * h.width + p.px0 + x] = (uint8_t)((tiff1_spread(row[x >> 3] >> (x & 4 ? 0 : 4)) ^ inv) >> (8 * (x & 3)));
  }
  if (FILE *fo = status ? nullptr : fopen(argv[2], "wb")) fwrite(pix.data(), 1, pix.size(), fo), fclose(fo);
  printf("%d %lu %lu | %s\n", status, g_tokens, g_steps, why);
  return 0;
}
