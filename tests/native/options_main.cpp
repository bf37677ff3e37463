// options_main.cpp — the option table (datago_amd/csrc/host/options.cpp) driven
// without a GPU (tests/test_options_cpu.py).
//
//   options_main list
//       one line per row: name, the option value a fresh Options holds for it
//       (what dg_ctx_set_option would have to be given to leave it as it is),
//       the row's "after" tag
//   options_main apply KEY V [KEY V ...]
//       each pair goes to apply_option on a fresh Options; one line per pair:
//       status (0 stored, 1 rejected, 2 unknown), the row's field afterwards
//       (- when the key has none), 1 if the Options bytes are unchanged, and
//       the dg_last_error text of a failure
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "host/options.h"

using namespace dg;

static std::string field(const OptRow &r, const Options &o) {
  const void *p = (const char *)&o + r.off;
  switch (r.type) {
    case kOptNone: return "-";
    case kOptBool: return std::to_string((int)*(const bool *)p);
    case kOptInt: return std::to_string(*(const int *)p);
    case kOptU32: return std::to_string(*(const uint32_t *)p);
    case kOptI64: return std::to_string(*(const int64_t *)p);
    case kOptU64: return std::to_string(*(const uint64_t *)p);
    case kOptDouble: return std::to_string((int64_t) * (const double *)p);
  }
  return "?";
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "list")) {
    const Options o;
    for (int i = 0; i < kNumOptions; i++) {
      const OptRow &r = kOptionTable[i];
      std::string v = field(r, o);
      if (r.kind == kOptFlagInv) v = v == "0" ? "1" : "0";
      if (r.shift) v = std::to_string(strtoull(v.c_str(), nullptr, 10) >> r.shift);
      printf("%s\t%s\t%d\n", r.name, v.c_str(), (int)r.after);
    }
    return 0;
  }
  if (argc >= 4 && argc % 2 == 0 && !strcmp(argv[1], "apply")) {
    for (int i = 2; i < argc; i += 2) {
      Options a, b;
      memcpy((void *)&b, (const void *)&a, sizeof(Options));  // the same bytes, padding included
      const int64_t v = strtoll(argv[i + 1], nullptr, 10);
      std::string why;
      const OptResult st = apply_option(b, argv[i], v, &why);
      const OptRow *r = find_option(argv[i]);
      printf("%d\t%s\t%d\t%s\n", (int)st, r ? field(*r, b).c_str() : "-", !memcmp(&a, &b, sizeof(Options)),
             st == kOptStored ? "" : option_error_text(argv[i], v, why).c_str());
    }
    return 0;
  }
  fprintf(stderr, "usage: options_main list | apply KEY V [KEY V ...]\n");
  return 2;
}
