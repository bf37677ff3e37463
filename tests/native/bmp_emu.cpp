// bmp_emu.cpp — the step logic of k_bmp_rle and the lane work of k_bmp_expand (dg_bmp.hip) on the CPU:
// the same per-lane routines (dg_bmp.h) driven 64 lanes at a time, with loops in place of the wave's
// ballots, shuffles and prefix sum, behind host/bmp_header.cpp.  tests/test_bmp_cpu.py compares it to
// tests/ref_bmp.py, and builds it with its own main (-DBMP_MAIN) under AddressSanitizer and UBSan.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dg_bmp.h"
#include "host/bmp_header.h"

using namespace dg;

namespace {

uint64_t below(uint32_t k) { return k >= 64u ? ~0ull : (1ull << k) - 1ull; }

// The aligned dword at offset `ad` of a buffer of `end` bytes; bytes at or past `end` read as zero.
// (ad may lie up to three bytes in front of the stream: `base` is the file, which starts well before it.)
uint32_t ld32(const uint8_t *base, uint64_t ad, uint64_t end) {
  uint32_t v = 0;
  for (uint32_t q = 0; q < 4; q++)
    if (ad + q < end) v |= (uint32_t)base[ad + q] << (8u * q);
  return v;
}

// k_bmp_rle: src = the stream (len bytes), out = the index plane (w * h bytes).  Returns kBmpFail* or 0.
uint32_t emu_rle(const uint8_t *src, uint32_t len, uint32_t W, uint32_t H, uint32_t rle4, uint8_t *out, uint64_t *steps,
                 uint64_t *hops) {
  const uint32_t npix = W * H, ppu = bmp_ppu(rle4);
  BmpRle s = {0u, 0u, 0u, 0u, 0u};
  uint32_t fail = 0;
  const uint32_t max_steps = len / (2u * kBmpStepUnits) + 2u;
  for (uint32_t step = 0; step < max_steps && s.o < npix; step++) {
    if (steps) ++*steps;
    uint32_t a[64], b[64], kind[64], q[64], c[64], o[64], f[64], blk_left[64], blk_base[64];
    bool inb[64], done[64];
    uint64_t absm = 0;
    for (uint32_t l = 0; l < 64; l++) {
      const uint32_t bp = s.pos + 2u * l;
      inb[l] = bp + 2u <= len && bp + 2u > bp;
      a[l] = inb[l] ? src[bp] : 0u;
      b[l] = inb[l] ? src[bp + 1u] : 0u;
      kind[l] = bmp_unit_kind(a[l], b[l]);
      q[l] = bmp_unit_pixels(a[l], b[l]);
      if (inb[l] && kind[l] == kBmpAbs) absm |= 1ull << l;
      blk_left[l] = s.data_left;
      blk_base[l] = 0;
    }
    const uint32_t first = s.data_units < kBmpStepUnits ? s.data_units : kBmpStepUnits;
    uint64_t data = below(first);
    uint32_t carry_units = s.data_units - first, carry_left = carry_units ? s.data_left - kBmpStepUnits * ppu : 0u;
    uint64_t rest = absm & ~data;
    while (rest) {
      if (hops) ++*hops;
      const uint32_t m = (uint32_t)__builtin_ctzll(rest);
      const uint32_t n = q[m];
      const uint32_t lo = m + 1u, hi = lo + bmp_abs_units(n, rle4);
      const uint64_t cov = below(hi) & ~below(lo);
      for (uint32_t l = lo; l < hi && l < 64u; l++) {
        blk_left[l] = n;
        blk_base[l] = lo;
      }
      data |= cov;
      if (hi > kBmpStepUnits) {
        carry_units = hi - kBmpStepUnits;
        carry_left = n - (kBmpStepUnits - lo) * ppu;
      }
      rest &= ~(cov | (1ull << m));
    }
    uint32_t total = 0;
    for (uint32_t l = 0; l < 64; l++) {
      const bool isdata = (data >> l) & 1ull;
      c[l] = isdata ? bmp_data_count(blk_left[l], l - blk_base[l], rle4) : kind[l] == kBmpRun ? q[l] : 0u;
      if (!inb[l]) c[l] = 0u;
      o[l] = s.o + total;
      total += c[l];
    }
    const uint64_t starts = ~data;
    uint32_t ke = kBmpStepUnits;
    for (uint32_t l = 0; l < 64; l++) {
      const bool isdata = (data >> l) & 1ull;
      const uint64_t before = starts & below(l);
      const bool prev_eol = before ? kind[63u - (uint32_t)__builtin_clzll(before)] == kBmpEol : s.prev_eol != 0u;
      done[l] = o[l] >= npix;
      f[l] = !inb[l] ? kBmpFailShort : !isdata ? bmp_cmd_fail(kind[l], q[l], o[l], W, prev_eol) : 0u;
      if (ke == kBmpStepUnits && (done[l] || f[l])) ke = l;
    }
    if (ke < kBmpStepUnits && !done[ke]) {
      fail = f[ke];
      break;
    }
    for (uint32_t l = 0; l < ke; l++) {
      const bool isdata = (data >> l) & 1ull;
      for (uint32_t t = 0; t < c[l]; t++) {
        if (o[l] + t >= npix) return 99u;  // (never: a command that keeps the row order ends inside the bitmap)
        out[o[l] + t] = (uint8_t)(isdata ? bmp_data_pixel(a[l], b[l], t, rle4) : bmp_run_pixel(b[l], t, rle4));
      }
    }
    if (ke < kBmpStepUnits) {
      s.o = npix;
    } else {
      s.pos += 2u * kBmpStepUnits;
      s.o += total;
      s.data_units = carry_units;
      s.data_left = carry_left;
      if (starts) s.prev_eol = kind[63u - (uint32_t)__builtin_clzll(starts)] == kBmpEol ? 1u : 0u;
    }
  }
  if (!fail && s.o < npix) fail = kBmpFailShort;
  return fail;
}

const char *fail_text(uint32_t f) {
  return f == kBmpFailRow     ? "BMP: RLE run or absolute block passes its row's end"
         : f == kBmpFailDelta ? "BMP: RLE delta, early end-of-line or end-of-bitmap leaves pixels unwritten"
         : f == kBmpFailShort ? "BMP: RLE data ends before the bitmap is complete"
         : f == kBmpFailPalette ? "BMP: pixel index past the colour table"
                                : "BMP: decode failed";
}

}  // namespace

extern "C" {

// fields: status, header_size, width, height, top_down, bits, compression, stride, data_off, data_len, out_c,
// pos r / g / b / a, npal
int bmp_parse(const uint8_t *d, size_t n, int64_t *f, uint8_t *pal, const char **why) {
  BmpHeader h;
  parse_bmp_header(d, n, h);
  const int64_t v[16] = {h.status, h.header_size, h.width,  h.height, h.top_down, h.bits,   h.compression, h.stride,
                         h.data_off, (int64_t)h.data_len, h.out_c, h.pos[0], h.pos[1], h.pos[2], h.pos[3], h.npal};
  memcpy(f, v, sizeof(v));
  if (pal) memcpy(pal, h.pal, 1024);
  *why = h.why;
  return h.status;
}

// The whole path.  pix: width x height x out_c bytes (cap checked).  Returns 0 / 1 (unsupported) / 2 (corrupt).
int bmp_decode(const uint8_t *d, size_t n, uint8_t *pix, size_t cap, const char **why, uint64_t *steps, uint64_t *hops) {
  BmpHeader h;
  parse_bmp_header(d, n, h);
  *why = h.why;
  if (steps) *steps = 0;
  if (hops) *hops = 0;
  if (h.status != BH_OK) return h.status;
  const uint32_t W = h.width, H = h.height, C = (uint32_t)h.out_c;
  const uint32_t rle = h.compression == BMP_RLE8 ? 1u : h.compression == BMP_RLE4 ? 2u : 0u;
  std::vector<uint8_t> idx;
  if (rle) {
    idx.assign((size_t)W * H, 0);
    const uint32_t f = emu_rle(d + h.data_off, (uint32_t)h.data_len, W, H, rle == 2u ? 1u : 0u, idx.data(), steps, hops);
    if (f) {
      *why = fail_text(f);
      return f == 99u ? -2 : 1;
    }
  }
  if ((size_t)W * H * C > cap) return -1;
  // k_bmp_expand: a lane per group of four pixels of a row
  const uint32_t bits = rle ? 8u : (uint32_t)h.bits, stride = rle ? W : h.stride;
  const uint8_t *base = rle ? idx.data() : d;
  const uint64_t org = rle ? 0u : h.data_off, end = rle ? (uint64_t)W * H : (uint64_t)h.data_off + h.data_len;
  const uint32_t pr = (uint32_t)h.pos[0], pg = (uint32_t)h.pos[1], pb = (uint32_t)h.pos[2];
  const uint32_t pa = h.pos[3] < 0 ? 4u : (uint32_t)h.pos[3];
  const uint32_t gpr = bmp_row_groups(W);
  bool past = false;
  for (uint32_t grp = 0; grp < gpr * H; grp++) {
    const uint32_t y = grp / gpr, gx = grp - y * gpr, x0 = 4u * gx;
    const uint32_t cnt = W - x0 < 4u ? W - x0 : 4u;
    const uint64_t A = org + (uint64_t)bmp_src_row(y, H, rle ? 0u : (uint32_t)h.top_down) * stride + bmp_group_off(x0, bits);
    const uint64_t last = A + bmp_group_bytes(x0, cnt, bits);
    const uint64_t A0 = A & ~3ull;
    const uint32_t sh = (uint32_t)(A & 3ull) * 8u;
    uint32_t r[5], v[4];
    for (uint32_t k = 0; k < 5; k++) r[k] = A0 + 4u * k < last ? ld32(base, A0 + 4u * k, end) : 0u;
    for (uint32_t k = 0; k < 4; k++) v[k] = sh ? (r[k] >> sh) | (r[k + 1] << (32u - sh)) : r[k];
    for (uint32_t t = 0; t < cnt; t++) {
      uint8_t p[4] = {0, 0, 0, 255};
      if (bits <= 8u) {
        const uint32_t i = bmp_index_at(v, x0, t, bits);
        if (i < (uint32_t)h.npal)
          memcpy(p, h.pal[i], 4);
        else
          past = true;
      } else if (bits == 24u) {
        p[0] = (uint8_t)bmp_byte(v, 3u * t + 2u);
        p[1] = (uint8_t)bmp_byte(v, 3u * t + 1u);
        p[2] = (uint8_t)bmp_byte(v, 3u * t);
      } else {
        p[0] = (uint8_t)(v[t] >> (8u * pr));
        p[1] = (uint8_t)(v[t] >> (8u * pg));
        p[2] = (uint8_t)(v[t] >> (8u * pb));
        if (pa < 4u) p[3] = (uint8_t)(v[t] >> (8u * pa));
      }
      memcpy(pix + ((size_t)y * W + x0 + t) * C, p, C);
    }
  }
  if (past) {
    *why = fail_text(kBmpFailPalette);
    return 1;
  }
  return 0;
}

}  // extern "C"

#ifdef BMP_MAIN
// Every file and every one of its truncations through the parser and the emulator.
int main(int argc, char **argv) {
  uint64_t runs = 0, ok = 0, unsup = 0, corrupt = 0;
  for (int a = 1; a < argc; a++) {
    FILE *fp = fopen(argv[a], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(fp);
    std::vector<size_t> cuts;  // every length; of a large file 64 of them and the whole
    const size_t stride = file.size() <= 1500 ? 1 : file.size() / 64 + 1;
    for (size_t n = 0; n < file.size(); n += stride) cuts.push_back(n);
    cuts.push_back(file.size());
    for (size_t n : cuts) {
      std::vector<uint8_t> cut(file.begin(), file.begin() + n);  // an allocation of exactly n bytes
      BmpHeader h;
      parse_bmp_header(cut.data(), cut.size(), h);
      std::vector<uint8_t> pix(h.status == BH_OK ? (size_t)h.width * h.height * h.out_c : 0);
      const char *why = "";
      const int st = bmp_decode(cut.data(), cut.size(), pix.data(), pix.size(), &why, nullptr, nullptr);
      runs++;
      ok += st == 0;
      unsup += st == 1;
      corrupt += st == 2;
      if (st < 0 || st > 2) return 3;
    }
  }
  printf("ok runs %llu decoded %llu unsupported %llu corrupt %llu\n", (unsigned long long)runs,
         (unsigned long long)ok, (unsigned long long)unsup, (unsigned long long)corrupt);
  return 0;
}
#endif
