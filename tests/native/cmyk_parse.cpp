// The header parser's allow_cmyk flag (context option "jpeg_cmyk") beside
// allow_h1v2 (test infrastructure, tests/test_jpeg_cmyk_cpu.py).
#include <stdint.h>
#include <string.h>

#include "host/jpeg_header.h"

// status of parse_jpeg_header with the two flags; its `why` text into why[cap];
// info[0..3] = components, colorspace, hmax, vmax when it is JH_OK
extern "C" int cmyk_parse(const uint8_t *data, size_t len, int allow_cmyk, int allow_h1v2, char *why, size_t cap,
                          int *info) {
  dg::JpegHeader h;
  if (allow_cmyk || allow_h1v2)
    dg::parse_jpeg_header(data, len, h, allow_h1v2 != 0, allow_cmyk != 0);
  else
    dg::parse_jpeg_header(data, len, h);  // the default arguments, as capi.cpp and the tools call it
  if (cap) {
    strncpy(why, h.why, cap - 1);
    why[cap - 1] = 0;
  }
  if (info && h.status == dg::JH_OK) {
    info[0] = h.ncomp;
    info[1] = h.colorspace;
    info[2] = h.hmax;
    info[3] = h.vmax;
  }
  return h.status;
}
