// bmp_header.cpp — Windows bitmap header walk (see bmp_header.h).
//
// What decodes is what image 0.25's BmpDecoder and Pillow turn into the same
// bytes (DESIGN.md §3 "BMP" has the table).  A file that ends inside a header,
// the masks or the colour table, whose pixel offset lies inside the headers or
// past the file, or whose uncompressed pixel array is cut short is BH_CORRUPT;
// what is well-formed but outside the GPU path is BH_UNSUPPORTED, so the
// caller's CPU decoder decides.  An unsupported field is reported as soon as
// it is read: the layout behind it is not walked.
#include "bmp_header.h"

#include <string.h>

namespace dg {

bool is_bmp(const uint8_t *d, size_t n) { return n >= 2 && d[0] == 'B' && d[1] == 'M'; }

static void fail(BmpHeader &h, int st, const char *why) {
  h.status = st;
  h.why = why;
}

static uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }

// Byte of a byte-aligned 8-bit mask inside the pixel, -1 for any other mask.
static int mask_byte(uint32_t m) {
  for (int k = 0; k < 4; k++)
    if (m == (0xFFu << (8 * k))) return k;
  return -1;
}

void parse_bmp_header(const uint8_t *d, size_t n, BmpHeader &h) {
  h = BmpHeader();
  memset(h.pal, 0, sizeof(h.pal));
  if (!is_bmp(d, n)) return fail(h, BH_CORRUPT, "not a BMP");
  if (n < 14) return fail(h, BH_CORRUPT, "BMP: truncated file header");
  if (n < 18) return fail(h, BH_CORRUPT, "BMP: truncated info header");
  const uint32_t off = le32(d + 10), size = le32(d + 14);
  if (size == 52 || size == 56 || size == 64) return fail(h, BH_UNSUPPORTED, "BMP: OS/2 2.x, V2 or V3 info header");
  if (size != 12 && size != 40 && size != 108 && size != 124) return fail(h, BH_CORRUPT, "BMP: unknown info header size");
  if (n < 14 + (size_t)size) return fail(h, BH_CORRUPT, "BMP: truncated info header");
  h.header_size = (int)size;
  const uint8_t *ih = d + 14;
  int64_t w, ht;
  uint32_t planes, bits, comp = BMP_RGB, clr_used = 0;
  if (size == 12) {
    w = le16(ih + 4);
    ht = le16(ih + 6);
    planes = le16(ih + 8);
    bits = le16(ih + 10);
  } else {
    w = (int32_t)le32(ih + 4);
    ht = (int32_t)le32(ih + 8);
    planes = le16(ih + 12);
    bits = le16(ih + 14);
    comp = le32(ih + 16);
    clr_used = le32(ih + 32);
  }
  h.top_down = ht < 0;
  if (ht < 0) ht = -ht;
  if (planes != 1) return fail(h, BH_UNSUPPORTED, "BMP: planes not 1");
  if (w < 0) return fail(h, BH_UNSUPPORTED, "BMP: negative width");
  if (w == 0 || ht == 0) return fail(h, BH_UNSUPPORTED, "BMP: zero dimension");
  h.width = (uint32_t)w;
  h.height = (uint32_t)ht;
  if (bits == 16) return fail(h, BH_UNSUPPORTED, "BMP: 16 bits per pixel");
  if (bits == 2) return fail(h, BH_UNSUPPORTED, "BMP: 2 bits per pixel");
  if (bits != 1 && bits != 4 && bits != 8 && bits != 24 && !(bits == 32 && size != 12))
    return fail(h, BH_UNSUPPORTED, "BMP: unsupported bits per pixel");
  h.bits = (int)bits;
  if (comp > BMP_BITFIELDS) return fail(h, BH_UNSUPPORTED, "BMP: unsupported compression");
  h.compression = (int)comp;
  if ((comp == BMP_RLE8 && bits != 8) || (comp == BMP_RLE4 && bits != 4) || (comp == BMP_BITFIELDS && bits < 24))
    return fail(h, BH_UNSUPPORTED, "BMP: RLE or bit-field compression on a mismatched depth");
  if ((comp == BMP_RLE8 || comp == BMP_RLE4) && h.top_down) return fail(h, BH_UNSUPPORTED, "BMP: top-down RLE");
  if (comp == BMP_RGB && bits == 32 && size != 40)
    return fail(h, BH_UNSUPPORTED, "BMP: 32-bit BI_RGB under a V4 / V5 header");
  if (bits <= 8 && clr_used > (1u << bits)) return fail(h, BH_UNSUPPORTED, "BMP: colour table larger than the depth allows");
  h.out_c = 3;
  size_t pos = 14 + (size_t)size;  // behind the info header: the masks of a 40-byte header, the colour table
  if (bits >= 24) {
    h.pos[0] = 2, h.pos[1] = 1, h.pos[2] = 0, h.pos[3] = -1;  // B, G, R (, ignored)
    if (comp == BMP_BITFIELDS) {
      uint32_t m[4] = {0, 0, 0, 0};
      if (size == 40) {
        if (n < pos + 12) return fail(h, BH_CORRUPT, "BMP: truncated bit masks");
        for (int k = 0; k < 3; k++) m[k] = le32(d + pos + 4 * k);
        pos += 12;
      } else {
        for (int k = 0; k < 4; k++) m[k] = le32(ih + 40 + 4 * k);
      }
      if (bits == 24) {  // the one set there is: the order of BI_RGB
        if (m[0] != 0xFF0000u || m[1] != 0xFF00u || m[2] != 0xFFu)
          return fail(h, BH_UNSUPPORTED, "BMP: bit masks outside the supported sets");
      } else {
        const int r = mask_byte(m[0]), g = mask_byte(m[1]), b = mask_byte(m[2]), a = m[3] ? mask_byte(m[3]) : -1;
        // Pillow's SUPPORTED[32] without the all-zero set (all byte-aligned)
        static const uint32_t sets[7][4] = {
            {0xFF0000u, 0xFF00u, 0xFFu, 0x0u},         {0xFF000000u, 0xFF0000u, 0xFF00u, 0x0u},
            {0xFF000000u, 0xFF00u, 0xFFu, 0x0u},       {0xFF000000u, 0xFF0000u, 0xFF00u, 0xFFu},
            {0xFFu, 0xFF00u, 0xFF0000u, 0xFF000000u},  {0xFF0000u, 0xFF00u, 0xFFu, 0xFF000000u},
            {0xFF000000u, 0xFF00u, 0xFFu, 0xFF0000u}};
        bool known = false;
        for (int s = 0; s < 7; s++) known = known || !memcmp(sets[s], m, sizeof(m));
        if (!known || r < 0 || g < 0 || b < 0) return fail(h, BH_UNSUPPORTED, "BMP: bit masks outside the supported sets");
        h.pos[0] = r, h.pos[1] = g, h.pos[2] = b, h.pos[3] = a;
        if (a >= 0) h.out_c = 4;
      }
    }
  } else {
    const int entry = size == 12 ? 3 : 4;
    h.npal = clr_used ? (int)clr_used : 1 << bits;
    if (n < pos + (size_t)entry * h.npal) return fail(h, BH_CORRUPT, "BMP: truncated colour table");
    for (int i = 0; i < h.npal; i++) {  // B, G, R (, reserved)
      h.pal[i][0] = d[pos + entry * i + 2];
      h.pal[i][1] = d[pos + entry * i + 1];
      h.pal[i][2] = d[pos + entry * i];
      h.pal[i][3] = 255;
    }
    pos += (size_t)entry * h.npal;
  }
  // image's default Limits::max_alloc (512 MiB) covers the decoded image
  if ((uint64_t)h.width * h.height * (uint64_t)h.out_c > (512ull << 20))
    return fail(h, BH_UNSUPPORTED, "BMP: image over image's allocation limit");
  if (off < pos || off > n) return fail(h, BH_CORRUPT, "BMP: pixel data offset inside the headers or past the file");
  h.data_off = off;
  h.stride = (uint32_t)((((uint64_t)h.width * bits + 31) / 32) * 4);
  if (comp == BMP_RLE8 || comp == BMP_RLE4) {
    h.data_len = n - off;  // biSizeImage is not trusted: the stream ends at its end-of-bitmap code or with the file
  } else {
    h.data_len = (uint64_t)h.stride * h.height;
    if ((uint64_t)off + h.data_len > n) return fail(h, BH_CORRUPT, "BMP: pixel data truncated");
  }
  h.status = BH_OK;
}

}  // namespace dg
