// CPU form of the 16-bit PNG filter stage (context option "penc16"): the
// shared header datago_amd/csrc/dg_penc16.h driven the way k_penc_filter16
// drives it -- one "wave" of 64 lanes per row, a lane taking the quads at row
// bytes 4 * lane, 4 * lane + 256, ... -- so tests/test_penc16_cpu.py can hold
// the header's byte order, neighbours, sums and choice against
// tests/ref_penc16.py for equality.
//
//   shared library:  p16e_filter()
//   -DP16_MAIN:      a program of its own (for the sanitizers): reads records
//                    {h, w, spp, shift (uint32 each), h * w * spp uint16} from
//                    the file named on its command line and prints per record
//                    the filter types and the filtered stream in hex
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dg_penc16.h"

using namespace dg;

// px: h x w x spp native-endian samples, tightly packed.  shift (0 or 1): the
// image is placed `shift` samples past a 4-byte boundary, so that the rows'
// alignment classes change places (the encoder's own buffer has shift 0).
// types: h bytes; stream: h * (2 * w * spp + 1) bytes.
extern "C" void p16e_filter(const uint16_t *px, uint32_t h, uint32_t w, uint32_t spp, uint32_t shift, uint8_t *types,
                            uint8_t *stream) {
  const uint32_t n = w * spp, rb = 2 * n;
  std::vector<uint32_t> store(((size_t)h * n + shift) / 2 + 2);  // 4-byte aligned, as the encoder's input buffer is
  uint16_t *base = (uint16_t *)store.data() + shift;
  memcpy(base, px, (size_t)h * n * 2);
  for (uint32_t y = 0; y < h; y++) {
    const uint16_t *cur = base + (size_t)y * n, *up = y ? cur - n : nullptr;
    const bool cal = ((uintptr_t)cur & 3u) == 0, ual = up && ((uintptr_t)up & 3u) == 0;
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (uint32_t lane = 0; lane < 64; lane++)
      for (uint32_t x = 4 * lane; x < rb; x += 256) {
        const uint32_t left = rb - x;
        p16_sums(p16_quad(cur, up, x, n, spp, cal, ual), left < 4u ? left : 4u, sum);
      }
    const uint32_t best = p16_best(sum);
    uint8_t *dst = stream + (size_t)y * (rb + 1);
    types[y] = dst[0] = (uint8_t)best;
    for (uint32_t lane = 0; lane < 64; lane++)
      for (uint32_t x = 4 * lane; x < rb; x += 256) {
        const uint32_t r = p16_apply(best, p16_quad(cur, up, x, n, spp, cal, ual));
        for (uint32_t k = 0; k < 4 && x + k < rb; k++) dst[1 + x + k] = (uint8_t)(r >> (8 * k));
      }
  }
}

#ifdef P16_MAIN
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hd[4];
  while (fread(hd, 4, 4, f) == 4) {
    const size_t ns = (size_t)hd[0] * hd[1] * hd[2];
    std::vector<uint16_t> px(ns);
    if (fread(px.data(), 2, ns, f) != ns) return 3;
    std::vector<uint8_t> types(hd[0]), stream((size_t)hd[0] * (2 * hd[1] * hd[2] + 1));
    p16e_filter(px.data(), hd[0], hd[1], hd[2], hd[3], types.data(), stream.data());
    for (uint8_t t : types) printf("%u", t);
    printf(" ");
    for (uint8_t b : stream) printf("%02x", b);
    printf("\n");
  }
  fclose(f);
  return 0;
}
#endif
