// Stand-alone driver of the entropy emulator (emu.cpp) for sanitizer builds:
//   emu_main FILE SUB_BITS [LEAD_BITS]
// decodes FILE's coefficients once and prints the status and the emulator's
// consistency counters.  Exit status 0 when the decode ran and was consistent.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" void emu_set_lead(uint32_t lead);
extern "C" int64_t emu_two_mismatch();
extern "C" int64_t emu_multi_mismatch();
extern "C" int emu_decode_coefs(const uint8_t *data, size_t len, uint32_t sub_bits, int16_t *out, size_t cap_blocks,
                                size_t *nblocks, int64_t *stats);

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s FILE SUB_BITS [LEAD_BITS]\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> data;
  uint8_t buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
  fclose(f);
  emu_set_lead(argc > 3 ? (uint32_t)strtoul(argv[3], nullptr, 10) : 0u);
  const size_t cap = (size_t)1 << 16;
  std::vector<int16_t> out(cap * 64);
  size_t nb = 0;
  int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int r = emu_decode_coefs(data.data(), data.size(), (uint32_t)strtoul(argv[2], nullptr, 10), out.data(), cap,
                                 &nb, st);
  const long long two = (long long)emu_two_mismatch(), multi = (long long)emu_multi_mismatch();
  printf("status %d blocks %zu decoded %lld write_mismatch %lld two_mismatch %lld multi_mismatch %lld\n", r, nb,
         (long long)st[6], (long long)st[5], two, multi);
  return (r == 0 && st[5] == 0 && two == 0 && multi == 0 && (size_t)st[6] >= nb) ? 0 : 1;
}
