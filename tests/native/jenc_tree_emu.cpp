// jenc_tree_emu.cpp — a C ABI over datago_amd/csrc/dg_jenc_tree.h for
// tests/test_jenc_opt_cpu.py: the code the kernel k_enc_tree runs per table,
// with one lane, a sync and a min2 that do nothing.  With -DJT_MAIN it is a
// program of its own (for a sanitizer build): it reads histograms from a text
// file and prints what the library form returns.
//   build cls f0 .. f255  -> fallback, nvals, sizes, BITS, HUFFVAL, codes, lengths, DHT bytes
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "dg_jenc_tree.h"

namespace {
struct NoSync {
  void operator()() const {}
};
struct NoMin2 {
  void operator()(uint64_t &, uint64_t &) const {}
};
}  // namespace

extern "C" {

// f: 256 counts.  sizes: 257 K.2 sizes; bits: 17; vals, code, len: 256; info: nvals, fallback;
// dht: 21 + 256 bytes at the most.  Returns the DHT segment's length (0 on fallback).
uint32_t jte_build(const uint32_t *f, uint32_t cls, uint8_t *sizes, uint8_t *bits, uint8_t *vals, uint16_t *code,
                   uint8_t *len, uint32_t *info, uint8_t *dht) {
  auto w = std::make_unique<dg::JtWork>();
  auto o = std::make_unique<dg::JtOut>();
  dg::jt_build(f, 256u, *w, *o, code, len, 0, 1, NoSync(), NoMin2());
  memcpy(sizes, w->size, dg::kJtSyms);
  info[0] = o->nvals;
  info[1] = o->fallback;
  if (o->fallback) return 0;
  memcpy(bits, o->bits, 17);
  memcpy(vals, o->vals, o->nvals);
  dg::jt_dht(*o, cls, dht, 0, 1);
  return dg::jt_dht_bytes(*o);
}

}  // extern "C"

#ifdef JT_MAIN
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *in = fopen(argv[1], "r");
  if (!in) return 2;
  char word[16];
  while (fscanf(in, "%15s", word) == 1) {
    if (strcmp(word, "build")) return 3;
    unsigned cls;
    if (fscanf(in, "%u", &cls) != 1) return 3;
    // exactly sized, on the heap: the sanitizer sees any write past an end
    std::vector<uint32_t> f(256), info(2);
    std::vector<uint8_t> sizes(dg::kJtSyms), bits(17), vals(256), len(256), dht(21 + 256);
    std::vector<uint16_t> code(256);
    for (unsigned i = 0; i < 256; i++)
      if (fscanf(in, "%u", &f[i]) != 1) return 3;
    const uint32_t n = jte_build(f.data(), cls, sizes.data(), bits.data(), vals.data(), code.data(), len.data(),
                                 info.data(), dht.data());
    printf("build %u %u", info[1], info[0]);
    if (!info[1]) {
      for (unsigned i = 0; i < dg::kJtSyms; i++) printf(" %u", sizes[i]);
      for (unsigned i = 0; i < 17; i++) printf(" %u", bits[i]);
      for (unsigned i = 0; i < info[0]; i++) printf(" %u", vals[i]);
      for (unsigned i = 0; i < 256; i++) printf(" %u", code[i]);
      for (unsigned i = 0; i < 256; i++) printf(" %u", len[i]);
      for (unsigned i = 0; i < n; i++) printf(" %u", dht[i]);
    }
    printf("\n");
  }
  fclose(in);
  return 0;
}
#endif
