// gif_header.cpp — GIF container walk (see gif_header.h).
//
// Behaviour restates gif 0.13 as image 0.25's GifDecoder drives it for
// load_from_memory: the first frame composited on the logical screen.  What is
// structurally broken (a file ending inside a header, table, extension or
// sub-block chain; no image descriptor; no colour table) is GH_CORRUPT; what
// is well-formed but outside the GPU path is GH_UNSUPPORTED, so the caller's
// CPU decoder decides.  A structural break wins over an unsupported field.
#include "gif_header.h"

#include <string.h>

namespace dg {

bool is_gif(const uint8_t *d, size_t n) {
  return n >= 6 && (!memcmp(d, "GIF87a", 6) || !memcmp(d, "GIF89a", 6));
}

static void fail(GifHeader &h, int st, const char *why) {
  h.status = st;
  h.why = why;
}

static uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

void parse_gif_header(const uint8_t *d, size_t n, GifHeader &h) {
  h = GifHeader();
  memset(h.pal, 0, sizeof(h.pal));
  if (!is_gif(d, n)) return fail(h, GH_CORRUPT, "not a GIF");
  h.version = d[4] == '7' ? 87 : 89;
  if (n < 13) return fail(h, GH_CORRUPT, "GIF: truncated logical screen descriptor");
  h.width = le16(d + 6);
  h.height = le16(d + 8);
  const char *unsup = nullptr;  // the first well-formed field outside the GPU path
  if (h.width == 0 || h.height == 0) unsup = "GIF: zero logical screen dimension";
  size_t pos = 13;
  const uint8_t *table = nullptr;
  int ntable = 0;
  if (d[10] & 0x80) {
    ntable = 2 << (d[10] & 7);
    if (pos + 3 * (size_t)ntable > n) return fail(h, GH_CORRUPT, "GIF: truncated global colour table");
    table = d + pos;
    pos += 3 * (size_t)ntable;
    h.has_global = 1;
  }
  for (;;) {
    if (pos >= n) return fail(h, GH_CORRUPT, "GIF: no image descriptor");
    const uint8_t b = d[pos++];
    if (b == 0x3B) return fail(h, GH_CORRUPT, "GIF: no image descriptor");
    if (b == 0x2C) break;
    if (b != 0x21) return fail(h, GH_CORRUPT, "GIF: unknown block");
    if (pos >= n) return fail(h, GH_CORRUPT, "GIF: truncated extension");
    const uint8_t label = d[pos++];
    bool first = true;
    for (;;) {  // the extension's sub-blocks
      if (pos >= n) return fail(h, GH_CORRUPT, "GIF: truncated extension");
      const uint32_t len = d[pos++];
      if (!len) break;
      if (pos + len > n) return fail(h, GH_CORRUPT, "GIF: truncated extension");
      if (label == 0xF9 && first && len >= 4) h.transparent = (d[pos] & 1) ? (int)d[pos + 3] : -1;
      first = false;
      pos += len;
    }
  }
  if (pos + 9 > n) return fail(h, GH_CORRUPT, "GIF: truncated image descriptor");
  h.left = le16(d + pos);
  h.top = le16(d + pos + 2);
  h.fw = le16(d + pos + 4);
  h.fh = le16(d + pos + 6);
  const uint8_t packed = d[pos + 8];
  pos += 9;
  h.interlace = (packed & 0x40) ? 1 : 0;
  if (!unsup && (h.fw == 0 || h.fh == 0)) unsup = "GIF: zero frame dimension";
  if (packed & 0x80) {
    ntable = 2 << (packed & 7);
    if (pos + 3 * (size_t)ntable > n) return fail(h, GH_CORRUPT, "GIF: truncated local colour table");
    table = d + pos;
    pos += 3 * (size_t)ntable;
    h.has_local = 1;
  }
  if (pos >= n) return fail(h, GH_CORRUPT, "GIF: truncated image data");
  h.min_code_size = d[pos++];
  if (!unsup && (h.min_code_size < 2 || h.min_code_size > 8)) unsup = "GIF: LZW minimum code size outside 2..8";
  h.data_off = (uint32_t)pos;
  for (;;) {  // the image's sub-block chain: one byte read per block
    if (pos >= n) return fail(h, GH_CORRUPT, "GIF: truncated sub-block chain");
    const uint32_t len = d[pos];
    if (!len) break;
    if (pos + 1 + len > n) return fail(h, GH_CORRUPT, "GIF: truncated sub-block chain");
    if (!h.runs.empty() && h.runs.back().len == len)
      h.runs.back().count++;
    else
      h.runs.push_back({(uint32_t)pos, len, 1});
    h.nbytes += len;
    pos += 1 + len;
    if (pos > 0xFFFFFF00u) return fail(h, GH_CORRUPT, "GIF: file too large");
  }
  // closed form: a run of 255s, then at most one shorter block
  h.closed = h.runs.empty() || (h.runs.size() == 1 && (h.runs[0].len == 255 || h.runs[0].count == 1)) ||
             (h.runs.size() == 2 && h.runs[0].len == 255 && h.runs[1].count == 1);
  if (h.closed) h.runs.clear();
  if (!table) return fail(h, GH_CORRUPT, "GIF: no colour table");
  h.npal = ntable;
  for (int i = 0; i < ntable; i++) {
    h.pal[i][0] = table[3 * i];
    h.pal[i][1] = table[3 * i + 1];
    h.pal[i][2] = table[3 * i + 2];
    h.pal[i][3] = 255;
  }
  if (h.transparent >= 0) h.pal[h.transparent][3] = 0;  // the RGB is kept
  // image's default Limits::max_alloc (512 MiB) covers the Rgba8 screen
  if (!unsup && (uint64_t)h.width * h.height * 4ull > (512ull << 20)) unsup = "GIF: screen over image's allocation limit";
  if (unsup) return fail(h, GH_UNSUPPORTED, unsup);
  h.status = GH_OK;
}

}  // namespace dg
