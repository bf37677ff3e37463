// bmp_header.h — host-side Windows bitmap header walker (file header, info
// header, bit masks, colour table), no pixel work.
//
// Replaces the header half of `image::load_from_memory` for BMP (image 0.25's
// BmpDecoder, restated from its published source and pinned to Pillow where
// the two give the same bytes: DESIGN.md §3 "BMP").  The colour table is folded
// into a 256-entry RGBA table the way PLTE is for PNG and a GIF's tables are;
// the RLE decode and the expansion to Rgb8 / Rgba8 run on the GPU (dg_bmp.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dg {

enum BmpStatus { BH_OK = 0, BH_UNSUPPORTED = 1, BH_CORRUPT = 2 };
enum BmpCompression { BMP_RGB = 0, BMP_RLE8 = 1, BMP_RLE4 = 2, BMP_BITFIELDS = 3 };

struct BmpHeader {
  int status = BH_CORRUPT;
  const char *why = "";
  int header_size = 0;               // 12 / 40 / 108 / 124
  uint32_t width = 0, height = 0;    // height = |biHeight|
  int top_down = 0;                  // biHeight < 0
  int bits = 0;                      // 1 / 4 / 8 / 24 / 32
  int compression = 0;               // BMP_*
  uint32_t stride = 0;               // bytes per row of the pixel array: ((width * bits + 31) / 32) * 4
  uint32_t data_off = 0;             // bfOffBits
  uint64_t data_len = 0;             // stride * height, or for RLE what the file holds from data_off on
  int out_c = 0;                     // 3 (Rgb8) or 4 (Rgba8: a bit-field file with an alpha mask)
  int pos[4] = {0, 0, 0, 0};         // 24 / 32 bits: byte of R, G, B, A inside a pixel (A: -1 without a mask)
  int npal = 0;                      // entries of the colour table (1 / 4 / 8 bits)
  uint8_t pal[256][4];               // RGBA, alpha 255; zero past npal
};

bool is_bmp(const uint8_t *d, size_t n);
void parse_bmp_header(const uint8_t *d, size_t n, BmpHeader &h);

}  // namespace dg
