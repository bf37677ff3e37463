// penc_tree_emu.cpp — a C ABI over datago_amd/csrc/dg_penc_tree.h for
// tests/test_penc_dyn_cpu.py: the code the kernel k_penc_tree runs, with one
// lane and a sync that does nothing.  With -DPT_MAIN it is a program of its
// own (for a sanitizer build): it reads histograms from a text file and prints
// what the library form returns.
//   len L n f0 .. f(n-1)     -> the n code lengths
//   build f0 .. f285         -> lengths, codes, tokens, header words, choice
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "dg_penc_tree.h"

namespace {
struct NoSync {
  void operator()() const {}
};
}  // namespace

extern "C" {

int pte_lengths(const uint32_t *f, uint32_t nsym, uint32_t L, uint8_t *len) {
  if (nsym > dg::kPtLit || L > dg::kPtLevels || L < 1) return 0;
  auto k = std::make_unique<dg::PtWork>();
  dg::pt_lengths(f, nsym, L, len, *k, 0, 1, NoSync());
  return 1;
}

// info: ntok, hlit, hclen, hdr_bits, dyn; bits: dynamic, fixed
void pte_build(const uint32_t *f, uint8_t *litlen, uint32_t *table, uint8_t *cllen, uint16_t *tok, uint32_t *info,
               uint32_t *hdr, uint64_t *bits) {
  auto k = std::make_unique<dg::PtWork>();
  auto o = std::make_unique<dg::PtOut>();
  uint8_t seq[dg::kPtTableWords];
  dg::pt_build(f, *o, *k, seq, 0, 1, NoSync());
  memcpy(litlen, o->litlen, dg::kPtLit);
  memcpy(table, o->table, dg::kPtLit * 4);
  memcpy(cllen, o->cllen, dg::kPtCl);
  memcpy(tok, o->tok, o->ntok * 2);
  const uint32_t i5[5] = {o->ntok, o->hlit, o->hclen, o->hdr_bits, o->dyn};
  memcpy(info, i5, sizeof(i5));
  memcpy(hdr, o->hdr, sizeof(o->hdr));
  bits[0] = o->dyn_bits;
  bits[1] = o->fixed_bits;
}

}  // extern "C"

#ifdef PT_MAIN
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *in = fopen(argv[1], "r");
  if (!in) return 2;
  char word[16];
  while (fscanf(in, "%15s", word) == 1) {
    if (!strcmp(word, "len")) {
      unsigned L, n;
      if (fscanf(in, "%u %u", &L, &n) != 2 || n > dg::kPtLit) return 3;
      std::vector<uint32_t> f(n);
      std::vector<uint8_t> len(n);
      for (unsigned i = 0; i < n; i++)
        if (fscanf(in, "%u", &f[i]) != 1) return 3;
      if (!pte_lengths(f.data(), n, L, len.data())) return 3;
      printf("len");
      for (unsigned i = 0; i < n; i++) printf(" %u", len[i]);
      printf("\n");
    } else if (!strcmp(word, "build")) {
      std::vector<uint32_t> f(dg::kPtLit), table(dg::kPtLit), hdr(dg::kPtHdrWords);
      std::vector<uint8_t> litlen(dg::kPtLit), cllen(dg::kPtCl);
      std::vector<uint16_t> tok(dg::kPtLit + 2);
      uint32_t info[5];
      uint64_t bits[2];
      for (unsigned i = 0; i < dg::kPtLit; i++)
        if (fscanf(in, "%u", &f[i]) != 1) return 3;
      pte_build(f.data(), litlen.data(), table.data(), cllen.data(), tok.data(), info, hdr.data(), bits);
      printf("build");
      for (unsigned i = 0; i < dg::kPtLit; i++) printf(" %u", litlen[i]);
      for (unsigned i = 0; i < dg::kPtLit; i++) printf(" %u", table[i]);
      for (unsigned i = 0; i < dg::kPtCl; i++) printf(" %u", cllen[i]);
      for (unsigned i = 0; i < 5; i++) printf(" %u", info[i]);
      for (unsigned i = 0; i < info[0]; i++) printf(" %u", tok[i]);
      for (unsigned i = 0; i < (info[3] + 31) / 32; i++) printf(" %u", hdr[i]);
      printf(" %llu %llu\n", (unsigned long long)bits[0], (unsigned long long)bits[1]);
    } else {
      return 3;
    }
  }
  fclose(in);
  return 0;
}
#endif
