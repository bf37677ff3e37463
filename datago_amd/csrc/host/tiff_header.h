// tiff_header.h — host-side TIFF walker: the header, the first IFD and the
// segment (strip or tile) table, no pixel work.
//
// Replaces the header half of `image::load_from_memory` for TIFF (image 0.25's
// TiffDecoder over the tiff crate, restated from its published source and
// pinned to libtiff as Pillow drives it where the two give the same bytes:
// DESIGN.md §3 "TIFF").  The segments are decoded and placed on the GPU
// (dg_tiff.hip).  Plain C++: it also links into tests/native/tiff_emu.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dg {

enum TiffStatus { TH_OK = 0, TH_UNSUPPORTED = 1, TH_CORRUPT = 2 };
enum TiffCompression { TIFF_NONE = 1, TIFF_G4 = 4, TIFF_LZW = 5, TIFF_DEFLATE = 8, TIFF_PACKBITS = 32773 };  // (32946, the older Deflate code, is stored as 8)
constexpr uint32_t kTiffG4MaxWidth = 16384;  // pixels of a Group 4 row k_tiff_g4 holds (kG4MaxWidth, dg_tiff_g4.h)

// One strip or tile (the layout of TiffSeg, dg_types.h).
struct TiffSegment {
  uint32_t off, nbytes;  // the coded bytes in the file
  uint32_t dec;          // bytes they decode to (rows x segment width x samples x bytes per sample; bilevel: rows x ceil(width / 8))
  uint32_t dst;          // where those lie in the image's decoded arena (a multiple of 16)
};

struct TiffHeader {
  int status = TH_CORRUPT;
  const char *why = "";
  uint32_t width = 0, height = 0;
  int out_c = 0;           // 1 (L8), 2 (La8), 3 (Rgb8), 4 (Rgba8) = SamplesPerPixel
  int compression = 0;     // TIFF_*
  int predictor = 1;       // 1 or 2
  int invert = 0;          // WhiteIsZero
  int bits = 8;            // BitsPerSample of every sample: 8, 16 (L16 / La16 / Rgb16 / Rgba16; only with `deep`) or 1 (L8 of 0 / 255; only with `bilevel`)
  int swap = 0;            // 16-bit samples of an MM file: big-endian in the segments' decoded bytes
  int tiled = 0;
  uint32_t seg_w = 0, seg_h = 0;    // the tile, or width x RowsPerStrip (at most the height)
  uint32_t across = 0, down = 0;    // segments per row of segments (1 for strips) and rows of them
  uint64_t dec_total = 0;           // bytes of the decoded arena
  std::vector<TiffSegment> segs;    // across x down, row-major
};

bool is_tiff(const uint8_t *d, size_t n);
// deflate (option "tiff_deflate"): compression 8 and 32946 pass, with predictor 1 or 2; without it they are TH_UNSUPPORTED.
// deep (option "tiff16"): BitsPerSample 16 for every sample passes, with the other rules unchanged (dec, dec_total and
// the uncompressed length check count two bytes per sample); 16-bit WhiteIsZero is TH_UNSUPPORTED.  Without it
// such a file is TH_UNSUPPORTED "TIFF: samples not 8 bits".
// bilevel (option "tiff_bilevel"): BitsPerSample 1 (or absent) with one sample per pixel passes, under either gray
// photometric, with compression 1, 32773, 5, 8 / 32946 beside `deflate`, and 4 (CCITT Group 4, T6Options absent or 0,
// rows of up to kTiffG4MaxWidth pixels).  A segment's rows are ceil(seg_w / 8) bytes, and dec, dec_total and the
// uncompressed length check count those.  Modified Huffman and Group 3, Group 4's uncompressed mode, predictor 2,
// 2- and 4-bit samples and an extra sample are TH_UNSUPPORTED with texts of their own.  Without it every such file
// is TH_UNSUPPORTED "TIFF: samples not 8 bits".
void parse_tiff_header(const uint8_t *d, size_t n, TiffHeader &h, bool deflate = false, bool deep = false, bool bilevel = false);

}  // namespace dg
