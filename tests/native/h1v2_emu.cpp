// The header parser's allow_h1v2 flag (context option "jpeg_h1v2") and the
// entropy emulator behind it (test infrastructure, tests/test_jpeg_h1v2_cpu.py).
// emu.cpp's entry parses with the default options, under which a 4:4:0 file is
// JH_UNSUPPORTED; it is compiled in here with its one parser call given the
// flag, so the emulated decode itself is emu.cpp's, line for line.
#include <stdint.h>
#include <string.h>

#include "host/jpeg_header.h"

static bool g_allow_h1v2 = false;
#define parse_jpeg_header(d, n, h) parse_jpeg_header(d, n, h, g_allow_h1v2)
#include "emu.cpp"
#undef parse_jpeg_header

extern "C" void h1v2_set_allow(int allow) { g_allow_h1v2 = allow != 0; }

// status of parse_jpeg_header with or without the flag; its `why` text into why[cap]
extern "C" int h1v2_parse(const uint8_t *data, size_t len, int allow, char *why, size_t cap) {
  dg::JpegHeader h;
  if (allow)
    dg::parse_jpeg_header(data, len, h, true);
  else
    dg::parse_jpeg_header(data, len, h);  // the default argument, as capi.cpp and the tools call it
  if (cap) {
    strncpy(why, h.why, cap - 1);
    why[cap - 1] = 0;
  }
  return h.status;
}
