// webp_header.cpp — WebP container walk (see webp_header.h).
//
// What is structurally broken (a chunk past the RIFF size or the file, a bad
// VP8L signature or version, no image chunk, a VP8X canvas that differs from
// the VP8L size) is WH_CORRUPT; what is well-formed but outside the GPU path
// (animation, a lossy image chunk) is WH_UNSUPPORTED, so the caller's CPU
// decoder decides.  A structural break met first wins.
#include "webp_header.h"

#include <string.h>

#include "../dg_alph.h"

namespace dg {

bool is_webp(const uint8_t *d, size_t n) {
  return n >= 16 && !memcmp(d, "RIFF", 4) && !memcmp(d + 8, "WEBP", 4) && (!memcmp(d + 12, "VP8L", 4) || !memcmp(d + 12, "VP8X", 4));
}

static void fail(WebpHeader &h, int st, const char *why) {
  h.status = st;
  h.why = why;
}

static uint32_t le(const uint8_t *p, int n) {
  uint32_t v = 0;
  for (int i = 0; i < n; i++) v |= (uint32_t)p[i] << (8 * i);
  return v;
}

void parse_webp_header(const uint8_t *d, size_t n, WebpHeader &h) {
  h = WebpHeader();
  if (!is_webp(d, n)) return fail(h, WH_CORRUPT, "not a WebP");
  const uint64_t riff = le(d + 4, 4);
  if (riff < 4 || 8 + riff > n) return fail(h, WH_CORRUPT, "WebP: truncated chunk");
  const uint64_t end = 8 + riff;
  uint64_t pos = 12;
  bool first = true;
  const char *unsup = nullptr;  // the first well-formed thing outside the GPU path
  for (;;) {
    if (pos + 8 > end) {
      if (unsup) return fail(h, WH_UNSUPPORTED, unsup);
      return fail(h, WH_CORRUPT, pos >= end ? "WebP: no image chunk" : "WebP: truncated chunk");
    }
    const uint8_t *cc = d + pos;
    const uint64_t len = le(d + pos + 4, 4), body = pos + 8;
    if (body + len > end) return fail(h, WH_CORRUPT, "WebP: truncated chunk");
    if (first && !memcmp(cc, "VP8X", 4)) {
      if (len < 10) return fail(h, WH_CORRUPT, "WebP: truncated chunk");
      const uint8_t flags = d[body];
      h.extended = 1;
      h.alpha = (flags & 0x10) ? 1 : 0;
      h.canvas_w = 1 + le(d + body + 4, 3);
      h.canvas_h = 1 + le(d + body + 7, 3);
      h.width = h.canvas_w;  // what dg_probe reports for a file that never reaches a VP8L header
      h.height = h.canvas_h;
      if (flags & 0x02) unsup = "WebP: animated WebP";
    } else if (!memcmp(cc, "ANIM", 4) || !memcmp(cc, "ANMF", 4)) {
      if (!unsup) unsup = "WebP: animated WebP";
    } else if (!memcmp(cc, "VP8 ", 4) || !memcmp(cc, "ALPH", 4)) {
      if (!unsup) unsup = "WebP: lossy WebP";
    } else if (!memcmp(cc, "VP8L", 4)) {
      if (unsup) return fail(h, WH_UNSUPPORTED, unsup);
      if (len < 5) return fail(h, WH_CORRUPT, "WebP: truncated chunk");
      if (d[body] != 0x2f) return fail(h, WH_CORRUPT, "WebP: bad VP8L signature");
      const uint32_t v = le(d + body + 1, 4);
      h.width = 1 + (v & 0x3fff);
      h.height = 1 + ((v >> 14) & 0x3fff);
      if ((v >> 29) & 7) return fail(h, WH_CORRUPT, "WebP: bad VP8L version");
      if (h.extended) {
        if (h.canvas_w != h.width || h.canvas_h != h.height)
          return fail(h, WH_CORRUPT, "WebP: VP8X canvas size differs from the VP8L size");
      } else {
        h.alpha = (int)((v >> 28) & 1);
      }
      h.data_off = (uint32_t)(body + 5);
      h.nbytes = len - 5;
      h.status = WH_OK;
      return;
    }
    first = false;
    pos = body + len + (len & 1);
  }
}

// ---- lossy WebP (option "webp_lossy")

bool is_webp_lossy(const uint8_t *d, size_t n) {
  return n >= 16 && !memcmp(d, "RIFF", 4) && !memcmp(d + 8, "WEBP", 4) && (!memcmp(d + 12, "VP8 ", 4) || !memcmp(d + 12, "VP8X", 4));
}

static void fail8(Vp8Header &h, int st, const char *why) {
  h.status = st;
  h.why = why;
}

// The same walk and the same texts for what is structurally broken; a file whose image chunk is VP8L
// is left to parse_webp_header (claim 0).  ALPH before the image chunk is the alpha plane of option
// "webp_alpha"; without the option the file is refused as before.
void parse_webp_lossy(const uint8_t *d, size_t n, Vp8Header &h, bool alpha) {
  h = Vp8Header();
  if (!is_webp_lossy(d, n)) return fail8(h, WH_CORRUPT, "not a WebP");
  h.claim = 1;
  const uint64_t riff = le(d + 4, 4);
  if (riff < 4 || 8 + riff > n) return fail8(h, WH_CORRUPT, "WebP: truncated chunk");
  const uint64_t end = 8 + riff;
  uint64_t pos = 12;
  bool first = true;
  const char *unsup = nullptr;
  for (;;) {
    if (pos + 8 > end) {
      if (unsup) return fail8(h, WH_UNSUPPORTED, unsup);
      return fail8(h, WH_CORRUPT, pos >= end ? "WebP: no image chunk" : "WebP: truncated chunk");
    }
    const uint8_t *cc = d + pos;
    const uint64_t len = le(d + pos + 4, 4), body = pos + 8;
    if (body + len > end) return fail8(h, WH_CORRUPT, "WebP: truncated chunk");
    if (first && !memcmp(cc, "VP8X", 4)) {
      if (len < 10) return fail8(h, WH_CORRUPT, "WebP: truncated chunk");
      h.extended = 1;
      h.canvas_w = 1 + le(d + body + 4, 3);
      h.canvas_h = 1 + le(d + body + 7, 3);
      h.alpha_flag = (d[body] & 0x10) ? 1 : 0;
      if (d[body] & 0x02) unsup = "WebP: animated WebP";
    } else if (!memcmp(cc, "ANIM", 4) || !memcmp(cc, "ANMF", 4)) {
      if (!unsup) unsup = "WebP: animated WebP";
    } else if (!memcmp(cc, "ALPH", 4)) {
      if (!alpha) {
        if (!unsup) unsup = "WebP: lossy WebP with alpha";
      } else if (h.has_alph) {  // libwebp refuses the file; image-webp's answer is not known here
        if (!unsup) unsup = "WebP: more than one ALPH chunk";
      }
      if (!h.has_alph) {
        h.has_alph = 1;
        h.alph_off = (uint32_t)body;
        h.alph_len = (uint32_t)len;
        h.alph_hdr = len ? d[body] : 0u;
      }
    } else if (!memcmp(cc, "VP8L", 4)) {
      h.claim = 0;
      return fail8(h, WH_CORRUPT, "not a lossy WebP");
    } else if (!memcmp(cc, "VP8 ", 4)) {
      if (unsup) return fail8(h, WH_UNSUPPORTED, unsup);
      if (len < 10) return fail8(h, WH_CORRUPT, "WebP: truncated VP8 frame header");
      const uint32_t bits = le(d + body, 3);
      if (bits & 1) return fail8(h, WH_CORRUPT, "WebP: VP8 frame is not a key frame");
      if (((bits >> 1) & 7) > 3) return fail8(h, WH_CORRUPT, "WebP: VP8 version above 3");
      if (!((bits >> 4) & 1)) return fail8(h, WH_CORRUPT, "WebP: VP8 frame is not shown");
      if (d[body + 3] != 0x9d || d[body + 4] != 0x01 || d[body + 5] != 0x2a) return fail8(h, WH_CORRUPT, "WebP: bad VP8 start code");
      h.width = le(d + body + 6, 2) & 0x3fff;
      h.height = le(d + body + 8, 2) & 0x3fff;
      if (!h.width || !h.height) return fail8(h, WH_CORRUPT, "WebP: VP8 frame of no size");
      if ((bits >> 5) > len - 10) return fail8(h, WH_CORRUPT, "WebP: VP8 first partition reaches past the chunk");
      if (h.extended && (h.canvas_w != h.width || h.canvas_h != h.height))
        return fail8(h, WH_CORRUPT, "WebP: VP8X canvas size differs from the VP8 frame size");
      if (alpha && h.has_alph) {
        // libwebp decodes the plane whatever the flag says; the reference's decoder may not
        if (!h.alpha_flag) return fail8(h, WH_UNSUPPORTED, "WebP: ALPH chunk in a file whose VP8X alpha flag is clear");
        if (h.alph_len < 2) return fail8(h, WH_CORRUPT, "WebP: ALPH chunk of fewer than 2 bytes");
        if (!alph_header_ok(h.alph_hdr)) return fail8(h, WH_CORRUPT, "WebP: bad ALPH header byte");
        if (alph_compression(h.alph_hdr) == kAlphRaw && (uint64_t)h.alph_len - 1 < (uint64_t)h.width * h.height)
          return fail8(h, WH_CORRUPT, "WebP: raw alpha plane shorter than the image");
      }
      h.chunk_off = (uint32_t)body;
      h.chunk_len = (uint32_t)len;
      h.part0 = bits >> 5;
      h.status = WH_OK;
      return;
    }
    first = false;
    pos = body + len + (len & 1);
  }
}

}  // namespace dg
