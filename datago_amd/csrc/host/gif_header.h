// gif_header.h — host-side GIF container walker (signature .. first image's
// sub-block chain), no pixel work.
//
// Replaces the header half of `image::load_from_memory` for GIF (image 0.25's
// GifDecoder over gif 0.13): the logical screen, the global colour table, the
// extensions in front of the first image descriptor (the last Graphic Control
// Extension's transparent index is kept, everything else is skipped), the
// descriptor, its local colour table, the LZW minimum code size and the
// positions of the data sub-blocks.  The palette and the transparent index are
// folded into a 256-entry RGBA table the way PLTE + tRNS are for PNG; the LZW
// decode and the expansion to the Rgba8 screen run on the GPU (dg_gif.hip).
// Only the first frame counts: what follows its sub-block chain is not read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dg {

enum GifStatus { GH_OK = 0, GH_UNSUPPORTED = 1, GH_CORRUPT = 2 };

// `count` consecutive sub-blocks of `len` data bytes each; the first one's
// length byte is file byte `off`.
struct GifRun {
  uint32_t off, len, count;
};

struct GifHeader {
  int status = GH_CORRUPT;
  const char *why = "";
  int version = 0;                   // 87 / 89
  uint32_t width = 0, height = 0;    // logical screen
  uint32_t left = 0, top = 0, fw = 0, fh = 0;  // first frame's rectangle
  int interlace = 0;
  int has_global = 0, has_local = 0;
  int npal = 0;                      // entries of the table in use (local over global)
  int transparent = -1;              // the last GCE's transparent index (flag set), else -1
  int min_code_size = 0;
  uint8_t pal[256][4];               // RGBA: alpha 255, 0 at the transparent index; zero past npal
  uint32_t data_off = 0;             // file offset of the first sub-block's length byte
  uint64_t nbytes = 0;               // LZW code bytes (sum of the sub-block lengths)
  // closed = every sub-block but the last holds 255 bytes: code byte k is file
  // byte data_off + 1 + k + k / 255, and `runs` stays empty.  Otherwise the
  // chain as runs of equal lengths, in file order.
  bool closed = true;
  std::vector<GifRun> runs;
};

bool is_gif(const uint8_t *d, size_t n);
// Walks the file once up to the terminator of the first image's sub-block
// chain (one length byte per sub-block).
void parse_gif_header(const uint8_t *d, size_t n, GifHeader &h);

}  // namespace dg
