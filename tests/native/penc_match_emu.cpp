// penc_match_emu.cpp — a program over pm_build of datago_amd/csrc/dg_penc_tree.h
// for tests/test_penc_match_cpu.py: the code k_penc_mtree runs for the match
// tokens, with one lane and a sync that does nothing.  Each line of the input
// file holds 286 literal/length counts and 30 distance counts; the answer is
//   the 286 + 30 code lengths, the header's bit count, the dynamic and the
//   fixed block's bits, the header's words
#include <stdint.h>
#include <stdio.h>

#include <memory>

#include "dg_penc_tree.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *in = fopen(argv[1], "r");
  if (!in) return 2;
  auto k = std::make_unique<dg::PtWork>();
  auto o = std::make_unique<dg::PmOut>();
  uint32_t fl[dg::kPtLit], fd[dg::kPmDist];
  uint8_t seq[dg::kPmSeq + 4];
  for (;;) {
    unsigned got = 0;
    for (unsigned i = 0; i < dg::kPtLit + dg::kPmDist; i++) got += fscanf(in, "%u", i < dg::kPtLit ? &fl[i] : &fd[i - dg::kPtLit]) == 1;
    if (!got) break;
    if (got != dg::kPtLit + dg::kPmDist) return 3;
    dg::pm_build(fl, fd, *o, *k, seq, 0, 1, [] {});
    for (unsigned i = 0; i < dg::kPtLit; i++) printf("%u ", o->litlen[i]);
    for (unsigned i = 0; i < dg::kPmDist; i++) printf("%u ", o->distlen[i]);
    printf("%u %llu %llu", o->hdr_bits, (unsigned long long)o->dyn_bits, (unsigned long long)dg::pm_fixed_bits(fl, fd));
    for (unsigned i = 0; i < (o->hdr_bits + 31) / 32; i++) printf(" %u", o->hdr[i]);
    printf("\n");
  }
  fclose(in);
  return 0;
}
