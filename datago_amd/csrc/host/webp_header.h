// webp_header.h — host-side WebP container walker (RIFF .. the VP8L chunk's
// 5-byte header), no pixel work.
//
// Replaces the header half of `image::load_from_memory` for a still lossless
// WebP (image 0.25's WebPDecoder): the RIFF size, the chunks with their even
// padding, VP8X's canvas size and flags, and the first VP8L chunk's signature,
// size, alpha bit and version.  Nothing past that header is parsed here:
// transform data and prefix codes are interleaved with entropy-coded
// sub-images, so the rest of the stream is k_vp8l_decode's (dg_vp8l.hip).
//
// A simple lossy file (RIFF....WEBPVP8 ) is not named by is_webp: it stays an
// unknown format (DG_ERR_CORRUPT) from every entry point, so the glue's sniff
// keeps lossy files on its CPU path.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dg {

enum WebpStatus { WH_OK = 0, WH_UNSUPPORTED = 1, WH_CORRUPT = 2 };

struct WebpHeader {
  int status = WH_CORRUPT;
  const char *why = "";
  int extended = 0;                      // the file starts with VP8X
  int alpha = 0;                         // Rgba8: VP8X's alpha flag, or the VP8L header's bit in a simple file
  uint32_t canvas_w = 0, canvas_h = 0;   // VP8X
  uint32_t width = 0, height = 0;        // the VP8L header (the VP8X canvas until one is read: animated, lossy)
  uint32_t data_off = 0;                 // file offset of the bitstream after the 5-byte header
  uint64_t nbytes = 0;                   // its bytes
};

// RIFF....WEBP followed by VP8L or VP8X.
bool is_webp(const uint8_t *d, size_t n);
void parse_webp_header(const uint8_t *d, size_t n, WebpHeader &h);

// ---- lossy WebP (option "webp_lossy"): a still file whose image chunk is `VP8 `, simple or behind VP8X.
// The walk is the one above; it ends at the VP8 chunk's 10-byte frame header (frame tag with the
// first partition's size, start code, 14-bit width and height; the scale bits are ignored).  Nothing
// bool-coded is parsed here: the rest is k_vp8_parse's (dg_vp8.hip).
struct Vp8Header {
  int status = WH_CORRUPT;
  const char *why = "";
  int claim = 0;                         // the lossy path answers for this file (0: no WebP, or its image chunk is VP8L)
  int extended = 0;
  uint32_t canvas_w = 0, canvas_h = 0;   // VP8X
  uint32_t width = 0, height = 0;        // the frame header
  uint32_t chunk_off = 0;                // file offset of the VP8 chunk's payload (the frame tag)
  uint32_t chunk_len = 0;                // its bytes
  uint32_t part0 = 0;                    // bytes of the first partition, which follows the 10-byte header
  // the first ALPH chunk before the image chunk (recorded with either setting of "webp_alpha")
  int has_alph = 0;
  int alpha_flag = 0;                    // VP8X's alpha bit
  uint32_t alph_off = 0;                 // file offset of its payload (the header byte)
  uint32_t alph_len = 0;                 // its bytes
  uint32_t alph_hdr = 0;                 // the header byte (0 when the chunk is empty)
};

// RIFF....WEBP followed by `VP8 ` or VP8X.
bool is_webp_lossy(const uint8_t *d, size_t n);
// alpha (option "webp_alpha"): a file with one ALPH chunk before its image chunk is taken, and the chunk
// is held to the rules of dg_alph.h: a header byte of compression and pre-processing 0 or 1 with the reserved bits clear,
// at least 2 bytes, and a raw plane of at least width x height bytes (DG_ERR_CORRUPT otherwise: libwebp
// refuses these); a second ALPH chunk, or one in a file whose VP8X alpha flag is clear, is
// DG_ERR_UNSUPPORTED.  Off, such a file is "WebP: lossy WebP with alpha" as before.
void parse_webp_lossy(const uint8_t *d, size_t n, Vp8Header &h, bool alpha = false);

}  // namespace dg
