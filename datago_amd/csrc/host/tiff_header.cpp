// tiff_header.cpp — TIFF header, IFD and segment table walk (see tiff_header.h).
//
// What decodes is what the tiff crate and libtiff turn into the same bytes
// (DESIGN.md §3 "TIFF" has the table).  A broken IFD, a value, an offset or a
// count past the file, a segment table that does not fit the image and an
// uncompressed segment shorter than its rows are TH_CORRUPT; what is well-formed
// but outside the GPU path is TH_UNSUPPORTED, so the caller's CPU decoder
// decides.  Every read is bounds-checked against the file's length.
#include "tiff_header.h"

namespace dg {

bool is_tiff(const uint8_t *d, size_t n) {
  if (n < 4) return false;
  const bool le = d[0] == 'I' && d[1] == 'I' && (d[2] == 42 || d[2] == 43) && d[3] == 0;
  const bool be = d[0] == 'M' && d[1] == 'M' && d[2] == 0 && (d[3] == 42 || d[3] == 43);
  return le || be;
}

static void fail(TiffHeader &h, int st, const char *why) {
  h.status = st;
  h.why = why;
}

namespace {
struct Reader {
  const uint8_t *d;
  size_t n;
  bool be;
  uint32_t u16(size_t p) const { return be ? ((uint32_t)d[p] << 8) | d[p + 1] : ((uint32_t)d[p + 1] << 8) | d[p]; }
  uint32_t u32(size_t p) const { return be ? (u16(p) << 16) | u16(p + 2) : (u16(p + 2) << 16) | u16(p); }
};
// An IFD entry whose values are BYTE, SHORT or LONG and lie inside the file.
struct Entry {
  bool present = false, ok = false;
  uint32_t type = 0, count = 0;
  size_t pos = 0;  // of the first value
  uint32_t get(const Reader &r, uint32_t k) const {
    return type == 1 ? r.d[pos + k] : type == 3 ? r.u16(pos + 2 * (size_t)k) : r.u32(pos + 4 * (size_t)k);
  }
};
}  // namespace

void parse_tiff_header(const uint8_t *d, size_t n, TiffHeader &h, bool deflate, bool deep, bool bilevel) {
  h = TiffHeader();
  if (!is_tiff(d, n)) return fail(h, TH_CORRUPT, "not a TIFF");
  const Reader r{d, n, d[0] == 'M'};
  if (r.u16(2) == 43) return fail(h, TH_UNSUPPORTED, "TIFF: BigTIFF");
  if (n < 8) return fail(h, TH_CORRUPT, "TIFF: truncated header");
  const size_t ifd = r.u32(4);
  if (ifd < 8 || ifd + 2 > n) return fail(h, TH_CORRUPT, "TIFF: IFD offset past the file");
  const size_t cnt = r.u16(ifd);
  if (cnt == 0 || ifd + 2 + 12 * cnt > n) return fail(h, TH_CORRUPT, "TIFF: IFD reaches past the file");
  // the tags the decode depends on
  enum { T_W, T_H, T_BITS, T_COMP, T_PHOTO, T_FILL, T_SOFF, T_SPP, T_RPS, T_SCNT, T_PLANAR, T_PRED, T_TW, T_TH, T_TOFF, T_TCNT, T_EXTRA, T_FMT, T_T6, T_N };
  static const uint32_t ids[T_N] = {256, 257, 258, 259, 262, 266, 273, 277, 278, 279, 284, 317, 322, 323, 324, 325, 338, 339, 293};
  Entry e[T_N];
  for (size_t i = 0; i < cnt; i++) {
    const size_t p = ifd + 2 + 12 * i;
    const uint32_t tag = r.u16(p);
    for (int t = 0; t < T_N; t++) {
      if (ids[t] != tag || e[t].present) continue;
      Entry &x = e[t];
      x.present = true;
      x.type = r.u16(p + 2);
      x.count = r.u32(p + 4);
      const uint64_t sz = (x.type == 1 ? 1u : x.type == 3 ? 2u : 4u) * (uint64_t)x.count;
      x.pos = sz <= 4 ? p + 8 : r.u32(p + 8);
      x.ok = (x.type == 1 || x.type == 3 || x.type == 4) && x.count >= 1 && x.pos + sz <= n && x.pos + sz >= sz;
    }
  }
  for (int t = 0; t < T_N; t++)
    if (e[t].present && !e[t].ok) return fail(h, TH_CORRUPT, "TIFF: tag with a type, count or offset outside the file");
  auto one = [&](int t, uint32_t def) { return e[t].present ? e[t].get(r, 0) : def; };
  if (!e[T_W].present || !e[T_H].present || !e[T_PHOTO].present) return fail(h, TH_CORRUPT, "TIFF: a required tag is missing");
  h.width = one(T_W, 0);
  h.height = one(T_H, 0);
  if (h.width == 0 || h.height == 0) return fail(h, TH_UNSUPPORTED, "TIFF: zero dimension");
  // ---- what the GPU path does not take
  const uint32_t spp = one(T_SPP, 1), photo = one(T_PHOTO, 0), pred = one(T_PRED, 1);
  const uint32_t comp = deflate && one(T_COMP, 1) == 32946u ? (uint32_t)TIFF_DEFLATE : one(T_COMP, 1);  // one zlib stream under either code
  if (spp == 0 || spp > 4) return fail(h, TH_UNSUPPORTED, "TIFF: more than four samples per pixel");
  if (e[T_BITS].present && e[T_BITS].count != spp && !(e[T_BITS].count == 1 && spp == 1))
    return fail(h, TH_UNSUPPORTED, "TIFF: BitsPerSample count differs from SamplesPerPixel");
  const uint32_t bits = e[T_BITS].present ? e[T_BITS].get(r, 0) : 1u;
  for (uint32_t k = 0; k < spp; k++) {
    const uint32_t b = e[T_BITS].present ? e[T_BITS].get(r, k) : 1u;
    if (bilevel && (b == 2u || b == 4u)) return fail(h, TH_UNSUPPORTED, "TIFF: 2- or 4-bit samples");
    if (b != 8u && !(deep && b == 16u) && !(bilevel && b == 1u)) return fail(h, TH_UNSUPPORTED, "TIFF: samples not 8 bits");
    if (b != bits) return fail(h, TH_UNSUPPORTED, "TIFF: mixed BitsPerSample");  // (deep only: 8 and 16 in one pixel)
  }
  const bool bi = bits == 1u;                // (bilevel only) eight pixels to a byte, MSB first, rows padded to whole bytes
  const uint32_t sb = bi ? 1u : bits / 8u;   // bytes per sample in the pixel plane
  if (bi && spp != 1u) return fail(h, TH_UNSUPPORTED, "TIFF: bilevel with an extra sample");
  if (e[T_FMT].present)
    for (uint32_t k = 0; k < e[T_FMT].count; k++)
      if (e[T_FMT].get(r, k) != 1u) return fail(h, TH_UNSUPPORTED, "TIFF: signed or float samples");
  if (photo > 2) return fail(h, TH_UNSUPPORTED, "TIFF: palette, mask, CMYK, YCbCr or CIELab photometric");
  // libtiff (Pillow) returns the stored samples, the tiff crate inverts them
  if (photo == 0 && bits == 16u) return fail(h, TH_UNSUPPORTED, "TIFF: 16-bit WhiteIsZero");
  if (one(T_PLANAR, 1) != 1) return fail(h, TH_UNSUPPORTED, "TIFF: PlanarConfiguration 2");
  if (one(T_FILL, 1) != 1) return fail(h, TH_UNSUPPORTED, "TIFF: FillOrder 2");
  if (pred == 3) return fail(h, TH_UNSUPPORTED, "TIFF: floating-point predictor");
  if (pred != 1 && pred != 2) return fail(h, TH_UNSUPPORTED, "TIFF: unknown predictor");
  if (bi && pred == 2) return fail(h, TH_UNSUPPORTED, "TIFF: predictor 2 on 1-bit samples");  // (libtiff refuses it)
  if (bi && (comp == 2u || comp == 3u)) return fail(h, TH_UNSUPPORTED, "TIFF: Modified Huffman or Group 3 compression");
  if (bi && comp == TIFF_G4) {
    const uint32_t t6 = one(T_T6, 0);
    if (t6 & 2u) return fail(h, TH_UNSUPPORTED, "TIFF: Group 4 uncompressed mode");
    if (t6) return fail(h, TH_UNSUPPORTED, "TIFF: T6Options other than 0");
  }
  if (comp != TIFF_NONE && comp != TIFF_LZW && !(bi && comp == TIFF_G4) && comp != TIFF_PACKBITS && !(deflate && comp == TIFF_DEFLATE))
    return fail(h, TH_UNSUPPORTED, "TIFF: compression other than none, LZW and PackBits");
  // libtiff has no predictor in the raw and PackBits codecs and ignores the tag; the tiff crate applies it.  Its ZIP codec has one.
  if (pred == 2 && comp != TIFF_LZW && comp != TIFF_DEFLATE) return fail(h, TH_UNSUPPORTED, "TIFF: predictor without LZW");
  // samples and the extra one: libtiff (Pillow) and the tiff crate agree on these forms only
  const bool gray = photo < 2;
  const uint32_t colour = gray ? 1u : 3u;
  if (spp < colour || spp > colour + 1) return fail(h, TH_UNSUPPORTED, "TIFF: sample count does not fit the photometric");
  if (spp == colour && e[T_EXTRA].present) return fail(h, TH_UNSUPPORTED, "TIFF: ExtraSamples without an extra sample");
  if (spp > colour) {
    const bool unassoc = e[T_EXTRA].present && e[T_EXTRA].count == 1 && e[T_EXTRA].get(r, 0) == 2;
    if (!unassoc && !(spp == 4 && !e[T_EXTRA].present))
      return fail(h, TH_UNSUPPORTED, "TIFF: extra sample that is not unassociated alpha");
    if (photo == 0) return fail(h, TH_UNSUPPORTED, "TIFF: WhiteIsZero with alpha");
  }
  h.out_c = (int)spp;
  h.compression = (int)comp;
  h.predictor = (int)pred;
  h.invert = photo == 0;
  h.bits = (int)bits;
  h.swap = bits == 16u && r.be;
  // image's default Limits::max_alloc (512 MiB) covers the decoded image
  if ((uint64_t)h.width * h.height * spp * sb > (512ull << 20)) return fail(h, TH_UNSUPPORTED, "TIFF: image over image's allocation limit");
  // ---- the segments
  h.tiled = e[T_TW].present || e[T_TOFF].present;
  const Entry &eo = e[h.tiled ? T_TOFF : T_SOFF], &ec = e[h.tiled ? T_TCNT : T_SCNT];
  if (!eo.present || !ec.present) return fail(h, TH_CORRUPT, "TIFF: segment offsets or byte counts missing");
  if (h.tiled) {
    h.seg_w = one(T_TW, 0);
    h.seg_h = one(T_TH, 0);
    if (h.seg_w == 0 || h.seg_h == 0) return fail(h, TH_CORRUPT, "TIFF: tile size missing");
    if (h.seg_w % 16 || h.seg_h % 16) return fail(h, TH_UNSUPPORTED, "TIFF: tile size not a multiple of 16");
    if ((uint64_t)h.seg_w * h.seg_h * spp * sb >= (1ull << 31)) return fail(h, TH_UNSUPPORTED, "TIFF: tile too large for the GPU path");
  } else {
    const uint32_t rps = one(T_RPS, 0xFFFFFFFFu);
    if (rps == 0) return fail(h, TH_CORRUPT, "TIFF: RowsPerStrip 0");
    h.seg_w = h.width;
    h.seg_h = rps < h.height ? rps : h.height;
  }
  if (comp == TIFF_G4 && h.seg_w > kTiffG4MaxWidth) return fail(h, TH_UNSUPPORTED, "TIFF: Group 4 row wider than 16,384 pixels");
  h.across = (h.width + h.seg_w - 1) / h.seg_w;
  h.down = (h.height + h.seg_h - 1) / h.seg_h;
  const uint64_t nseg = (uint64_t)h.across * h.down;
  if (eo.count != nseg || ec.count != nseg) return fail(h, TH_CORRUPT, "TIFF: segment table does not fit the image");
  h.segs.resize((size_t)nseg);
  const uint64_t rowb = bi ? ((uint64_t)h.seg_w + 7u) / 8u : (uint64_t)h.seg_w * spp * sb;
  for (uint32_t s = 0; s < nseg; s++) {
    TiffSegment &g = h.segs[s];
    g.off = eo.get(r, s);
    g.nbytes = ec.get(r, s);
    if (g.off < 8 || (uint64_t)g.off + g.nbytes > n) return fail(h, TH_CORRUPT, "TIFF: segment past the file");
    const uint32_t sy = s / h.across;
    const uint32_t rows = h.tiled || (uint64_t)(sy + 1) * h.seg_h <= h.height ? h.seg_h : h.height - sy * h.seg_h;
    const uint64_t dec = rowb * rows;
    if (dec >= (1ull << 31) || h.dec_total + dec >= (1ull << 31)) return fail(h, TH_UNSUPPORTED, "TIFF: image too large for the GPU path");
    if (comp == TIFF_NONE && g.nbytes < dec) return fail(h, TH_CORRUPT, "TIFF: uncompressed segment shorter than its rows");
    g.dec = (uint32_t)dec;
    g.dst = (uint32_t)h.dec_total;
    if (comp != TIFF_NONE) h.dec_total += (dec + 15) & ~15ull;
  }
  // libtiff's test for the LZW of TIFF 5.0 and before (LSB-first codes), on the first segment
  if (comp == TIFF_LZW && h.segs[0].nbytes >= 2 && d[h.segs[0].off] == 0 && (d[h.segs[0].off + 1] & 1))
    return fail(h, TH_UNSUPPORTED, "TIFF: old-style LZW (LSB-first codes)");
  h.status = TH_OK;
}

}  // namespace dg
