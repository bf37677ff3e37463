// dg_types.h — POD structures shared by the host planner and the HIP kernels.
//
// One batch = N images.  The host parses headers (host/jpeg_header.cpp),
// chooses buckets (host/buckets.cpp), lays every per-image buffer out in one
// device arena and uploads an array of ImageDesc + per-kernel workgroup lists
// (WgItem).  All device addresses inside these structs are absolute.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define DG_HD __host__ __device__ __forceinline__
#define DG_DEVICE 1
#define DG_GLOBAL __attribute__((address_space(1)))  // global memory: global_load/store, not flat
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
#else
#define DG_HD static inline
#define DG_GLOBAL
#endif

namespace dg {

// Typed pointer to device memory from an address held in a descriptor.
template <class T>
DG_HD DG_GLOBAL T *gp(uint64_t a) {
  return (DG_GLOBAL T *)(uintptr_t)a;
}

// Three per-component counters without dynamic register indexing (which would
// spill to scratch): c in {0,1,2}.
DG_HD int32_t sel3(const int32_t v[3], uint32_t c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }
DG_HD void add3(int32_t v[3], uint32_t c, int32_t d) {
  v[0] += c == 0 ? d : 0;
  v[1] += c == 1 ? d : 0;
  v[2] += c == 2 ? d : 0;
}
// The same for the entropy passes' component count NC (3, or 4 for a batch with a CMYK / YCCK image,
// option "jpeg_cmyk"): c in {0..NC-1}.  NC = 3 is sel3 / add3 exactly.
template <int NC>
DG_HD int32_t seln(const int32_t (&v)[NC], uint32_t c) {
  static_assert(NC == 3 || NC == 4, "three or four components");
  if (NC == 4) return c == 0 ? v[0] : (c == 1 ? v[1] : (c == 2 ? v[2] : v[NC - 1]));
  return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]);
}
template <int NC>
DG_HD void addn(int32_t (&v)[NC], uint32_t c, int32_t d) {
  v[0] += c == 0 ? d : 0;
  v[1] += c == 1 ? d : 0;
  v[2] += c == 2 ? d : 0;
  if (NC == 4) v[NC - 1] += c == 3 ? d : 0;
}
template <int NC>
DG_HD void setn(int32_t (&v)[NC], int32_t x) {
  v[0] = v[1] = v[2] = x;
  if (NC == 4) v[NC - 1] = x;
}
// v = a and v += a over NC components (either side may be a record in global memory)
template <int NC, class V, class A>
DG_HD void cpyn(V &v, const A &a) {
  v[0] = a[0];
  v[1] = a[1];
  v[2] = a[2];
  if (NC == 4) v[NC - 1] = a[NC - 1];
}
template <int NC, class V, class A>
DG_HD void accn(V &v, const A &a) {
  v[0] += a[0];
  v[1] += a[1];
  v[2] += a[2];
  if (NC == 4) v[NC - 1] += a[NC - 1];
}
// v = a - v: a checkpoint's prefix sums turned into its tail
template <int NC, class V, class A>
DG_HD void rsubn(V &v, const A &a) {
  v[0] = a[0] - v[0];
  v[1] = a[1] - v[1];
  v[2] = a[2] - v[2];
  if (NC == 4) v[NC - 1] = a[NC - 1] - v[NC - 1];
}

constexpr int kLutBits = 10;          // Huffman first-level lookup width
constexpr int kMaxSlots = 6;         // Huffman tables per image (DC/AC x 3 components)
constexpr int kSubPerWg = 256;       // entropy subsequences per workgroup (= threads)
constexpr int kDefaultSubBits = 2048; // destuffed bits per subsequence
constexpr int kDestuffChunk = 4096;   // raw bytes per destuff chunk (one wave of k_destuff_count / _write)
constexpr uint32_t kDsWgChunks = 4;   // consecutive chunks per workgroup of k_destuff_count / _write
constexpr uint32_t kInf = 0xFFFFFFFFu;

// Canonical Huffman table for the GPU decoder (built on the host, pooled).
// Two-level lookup: the first kLutBits bits index lut[]; codes longer than
// that (JPEG allows 16) continue in a 7-bit subtable selected by the entry.
//   lut entry: (len << 8) | symbol          for codes of length <= kLutBits
//              0x8000 | subtable index      when the prefix starts a long code
//              0                            invalid prefix / fallback below
constexpr int kSubBits = 16 - kLutBits;   // 6
constexpr int kMaxSubTables = 8;
struct HuffTable {
  uint16_t lut[1 << kLutBits];
  uint16_t sub[kMaxSubTables][1 << kSubBits];  // (len << 8) | symbol, 0 = invalid
  uint32_t lim[17];             // fallback (more long prefixes than subtables)
  int32_t valoff[17];
  uint8_t vals[256];
};

struct QuantTable {
  uint16_t q[64];  // natural (row-major) order
};

// Entropy-decoder state at a subsequence boundary:
//   bit 31 valid | bits 16..23 rel (destuffed bits past the anchor) | 8..15 r (block in MCU) | 0..7 z
DG_HD uint32_t pack_state(uint32_t rel, uint32_t r, uint32_t z) {
  return 0x80000000u | (rel << 16) | (r << 8) | z;
}
DG_HD uint32_t st_rel(uint32_t s) { return (s >> 16) & 0xFFu; }
DG_HD uint32_t st_r(uint32_t s) { return (s >> 8) & 0xFFu; }
DG_HD uint32_t st_z(uint32_t s) { return s & 0xFFu; }

// Per-subsequence record (64 bytes).
struct SubState {
  uint32_t in;      // state used at the subsequence start
  uint32_t out;     // state at the first symbol boundary at/after the next anchor
  uint32_t m;       // RST markers owned (FF byte inside this subsequence)
  uint32_t n;       // blocks started after the last owned marker (or the start)
  int32_t dc[4];    // DC differences summed after the last owned marker, per component
  uint32_t seg;     // exclusive segmented scan: restart segment at start
  uint32_t nin;     //   blocks already started in that segment
  int32_t dcin[4];  //   DC predictors at start
  uint32_t nstart;  // decode-once staging: blocks started in the range (all segments)
  uint32_t nent;    //   staged entries
};
static_assert(sizeof(SubState) == 64, "SubState is one 64-byte record");

// CS_CMYK / CS_YCCK: four-component Adobe files (APP14 transform 0 / 2, option "jpeg_cmyk"); k_cmyk turns their
// planes into the RGB image
enum Colorspace : uint32_t { CS_YCC = 0, CS_RGB = 1, CS_GRAY = 2, CS_CMYK = 3, CS_YCCK = 4 };

// Resize pass along one axis (one half of a fast_image_resize `resize` call).
struct ResizePass {
  uint64_t src, dst;        // device addresses
  uint64_t coef;            // int16 [out_size * ksize]   (written by k_coeffs)
  uint64_t bounds;          // int32 {start, size} [out_size] (written by k_coeffs)
  double in0, in1;          // source box along the axis
  uint32_t in_size, out_size;
  uint32_t ksize;           // coefficient slots per output
  int32_t precision;        // written by k_coeffs
  uint32_t src_stride, dst_stride;  // bytes per row
  uint32_t width, rows;     // output extent of this pass (pixels, rows)
  uint32_t out0;            // first output (of out_size) computed: integral crops fold into the pass
  uint32_t bands;           // band H kernel: kHBandRows-row bands per workgroup (option "hb_bands")
  uint32_t row0;            // H pass: first source row; V pass: source row of temp row 0
  uint32_t C;               // channels
  uint32_t kind;            // 0 none, 1 horizontal, 2 vertical; kR16V / kR16H: the 16-bit resize's passes
                            // (option "resize16", dg_resize16.hip: f32 weights in coef, {left, count} in bounds)
  uint32_t mode;            // H passes: kHFused = source is the YCbCr planes (upsample + colour
                            // in the fill), kHDirect = segment too wide for LDS (legacy kernel)
};
constexpr uint32_t kHFused = 1, kHDirect = 2;
constexpr uint32_t kR16V = 3, kR16H = 4;  // ResizePass::kind of pass[0] / pass[1] of a resized 16-bit PNG
constexpr uint32_t kHVFused = 4;      // pass[0] runs fused with pass[1] in k_resize_hv (its H rows stay in LDS)
// pass[0] of a JPEG runs in k_band_dec (dg_band.hip): IDCT + upsampling + colour + this H pass from the
// coefficients, 16-row strips of kDecCols output columns; kHDecWide: the 640-pixel segment class
constexpr uint32_t kHDecode = 8, kHDecWide = 16;
constexpr uint32_t kDecCols = 128;    // k_band_dec: output columns per workgroup (8 MFMA subtiles of 16)
constexpr uint32_t kDecSeg0 = 320, kDecSeg1 = 640;  // k_band_dec source segment classes (pixels)
constexpr uint32_t kDecStripsDefault = 8;           // k_band_dec: 16-row strips per workgroup (option "dec_strips")
constexpr uint32_t kHVSegPx = 320;    // k_resize_hv: LDS source segment per row (downscales up to ~2.3x)
constexpr uint32_t kHVTapsMax = 24;   // k_resize_hv: V taps (its LDS ring holds 32 rows)
constexpr uint32_t kHVRows = 64;      // k_resize_hv: V output rows per workgroup
constexpr uint32_t kHBandRows = 8;    // rows per workgroup of the band H kernel
constexpr uint32_t kHBandCols = 128;  // output columns per workgroup
constexpr uint32_t kIdctItemStride = 4;  // k_idct_t: L_IDCT items per workgroup (one per wave)

constexpr uint32_t kHSegPx = 640;     // LDS source segment (pixels) per row
constexpr uint32_t kHBandsDefault = 16;  // default ResizePass::bands (8 -> 16: +1.5% overlapped, profiles/r02/bands)

constexpr int kStages = 4;  // R1.H, R1.V, R2.H, R2.V

// ---- PNG (ImageDesc::fmt == kFmtPng)
constexpr uint32_t kFmtJpeg = 0, kFmtPng = 1, kFmtGif = 2, kFmtWebp = 3, kFmtVp8 = 4, kFmtBmp = 5;
// IDAT payloads are gathered into one contiguous zlib stream (k_png_gather),
// inflated into filtered scanlines (k_png_inflate, one wave per image),
// unfiltered (k_png_unfilter, one wave per 64-row band on a diagonal
// wavefront, consecutive bands pipelined across CUs)
// and, for palette / sub-byte / tRNS images, expanded to 8-bit L/LA/RGB/RGBA
// (k_png_expand); 16-bit images (option "png16") always take k_png_expand16
// instead: big-endian -> native u16, tRNS key, Adam7.
struct PngDesc {
  uint64_t zs;        // contiguous zlib stream
  uint64_t raw;       // inflated scanlines: height x (1 + rowbytes)
  uint64_t unf;       // unfiltered scanlines (stride ustride); == pix when expand == 0
  uint64_t pal;       // 256 x RGBA palette (device), 0 if none
  uint32_t zlen;      // zlib bytes
  uint32_t rowbytes;  // bytes per scanline (without the filter byte)
  uint32_t ustride;   // stride of unf
  uint32_t bpp;       // filter unit (bytes): 1-4, or 6 / 8 for 16-bit RGB / RGBA
  uint32_t ctype, depth, expand, has_trns;
  uint32_t trns[3];   // gray / RGB transparency key
  uint32_t chunk0;    // chunked inflate: first InfChunk of this image
  uint32_t nchunks;   // 0: serial inflate (small streams)
  uint32_t serial;    // set by the chunked path when the image must be inflated serially
  uint32_t interlace; // Adam7: raw/unf hold the 7 passes back to back (png_adam7_*)
  uint32_t rawlen;    // inflated bytes expected
  uint32_t uf_flag0;  // k_png_unfilter: first band progress flag of this image
};

// ---- GIF (ImageDesc::fmt == kFmtGif, option "gif"): the first frame on the logical screen as Rgba8.
// The frame's data sub-blocks are one LZW code stream: read through the chain where every block but
// the last holds 255 bytes (blocked), else gathered into a contiguous copy first (k_gif_gather).
// k_gif_lzw (one wave per image, dg_gif.h) decodes it into the fw x fh index plane in stream row order;
// k_gif_expand looks the indices up in the folded RGBA palette and places them on the screen
// (de-interlace, frame offset, clipping, transparent black outside the frame).  Anything irregular
// sets ImageDesc::status = DG_ERR_UNSUPPORTED and GifDesc::fail names it.
struct GifDesc {
  uint64_t src;       // blocked: the first sub-block's length byte in the file; else the gathered code bytes
  uint64_t src_end;   // one past the last source byte the stream occupies (loads stay below it)
  uint64_t idx;       // index plane: fw x fh bytes, rows in stream order
  uint64_t pal;       // 256 x RGBA palette (device)
  uint32_t nbytes;    // LZW code bytes
  uint32_t blocked;   // 1: code byte k is src[1 + k + k / 255]
  uint32_t mcs;       // LZW minimum code size (2..8)
  uint32_t npal;      // entries of the colour table in use
  uint32_t left, top, fw, fh;  // the frame's rectangle on the screen
  uint32_t interlace;
  uint32_t fail;      // kGifFail*: written by k_gif_lzw / k_gif_expand
};
constexpr uint32_t kGifFailCode = 1;     // a code above the next free one, or the next free one straight after a clear
constexpr uint32_t kGifFailShort = 2;    // the data ends (or an end code comes) before fw x fh indices
constexpr uint32_t kGifFailPalette = 3;  // an index at or past the colour table's size

// ---- BMP (ImageDesc::fmt == kFmtBmp, option "bmp"): a Windows bitmap as Rgb8 / Rgba8, top row first.
// An RLE8 / RLE4 stream is decoded by k_bmp_rle (one wave per image, dg_bmp.h) into a width x height
// index plane in stream (bottom-up) row order; k_bmp_expand reads that plane or the file's own pixel
// array and does the row flip, the palette lookup, BGR -> RGB and the mask byte selection.  Anything
// irregular sets ImageDesc::status = DG_ERR_UNSUPPORTED and BmpDesc::fail names it.
struct BmpDesc {
  uint64_t src;       // the pixel array or the RLE stream in the file (any byte alignment)
  uint64_t src_end;   // one past its last byte (loads stay below it)
  uint64_t idx;       // RLE: the index plane, width x height bytes, rows in stream order
  uint64_t pal;       // 256 x RGBA palette (device)
  uint32_t bits;      // 1 / 4 / 8 / 24 / 32
  uint32_t rle;       // 0, 1 = RLE8, 2 = RLE4
  uint32_t stride;    // bytes per row of the pixel array
  uint32_t top_down;
  uint32_t npal;      // entries of the colour table
  uint32_t pos;       // 24 / 32 bits: byte of R | G << 8 | B << 16 | A << 24 inside a pixel
  uint32_t data_len;  // RLE: bytes of the stream
  uint32_t fail;      // kBmpFail*: written by k_bmp_rle / k_bmp_expand
};
constexpr uint32_t kBmpFailRow = 1;      // a run or absolute block that passes (or starts past) its row's end
constexpr uint32_t kBmpFailDelta = 2;    // a delta, an early end-of-line or an end-of-bitmap with pixels unwritten
constexpr uint32_t kBmpFailShort = 3;    // the data ends before the last pixel
constexpr uint32_t kBmpFailPalette = 4;  // an index at or past the colour table's size

// ---- lossless WebP (ImageDesc::fmt == kFmtWebp, option "webp"): a VP8L chunk as Rgb8 / Rgba8.
// k_vp8l_decode (one wave per image, dg_vp8l.h) reads the bitstream after the 5-byte header in place:
// the transform list, their sub-images and the entropy-decoded ARGB plane go to the work arena
// (vp8l_*_off), the prefix-code tables to the table area.  k_vp8l_inverse applies the inverse
// transforms in reverse order of reading, k_vp8l_store writes pix (dec_c 3 drops the alpha).
// A broken stream sets ImageDesc::status and Vp8lDesc::fail (kVp8lFail*) names it.
struct Vp8lDesc {
  uint64_t src;          // the bitstream after the VP8L header, in the file
  uint64_t src_end;      // one past its last byte (loads stay below it)
  uint64_t work;         // work arena: vp8l_work_words(width, height) u32
  uint64_t tabs;         // table area: groups_cap x kVp8lGroupWords u32
  uint32_t nbytes;       // bitstream bytes
  uint32_t groups_cap;   // prefix-code groups the table area holds
  uint32_t fail;         // kVp8lFail*: written by k_vp8l_decode
  uint32_t ntrans;       // written by k_vp8l_decode: transforms read,
  uint32_t trans[4];     // ... each as vp8l_trans_pack, in the order read,
  uint32_t xsize;        // ... the width of the decoded (packed) image in plane 0,
  uint32_t npal;         // ... and the colour table's entries
  uint32_t final_plane;  // written by k_vp8l_inverse: the plane that holds the ARGB image
  uint32_t alph;         // 1: an ALPH chunk's stream (option "webp_alpha"): vp8l_walk's end-of-data rule for it
};
constexpr uint32_t kVp8lFailBits = 1;       // the data ends before the image is complete
constexpr uint32_t kVp8lFailCode = 2;       // a prefix code neither complete nor single-symbol (or its description broken)
constexpr uint32_t kVp8lFailCopy = 3;       // a copy reaching before the first pixel or past the last
constexpr uint32_t kVp8lFailCache = 4;      // a cache index with no cache, or cache bits outside 1..11
constexpr uint32_t kVp8lFailTransform = 5;  // a transform used twice
constexpr uint32_t kVp8lFailGroups = 6;     // more groups than the table area holds (DG_ERR_UNSUPPORTED)

// ---- lossy WebP (ImageDesc::fmt == kFmtVp8, option "webp_lossy"): a VP8 key frame as Rgb8.
// k_vp8_parse (one wave per image, dg_vp8.h) reads the chunk in place: the first partition's header
// and per-MB modes, the token partitions' coefficients; records and coefficients go to the work arena
// (layout_vp8).  k_vp8_recon predicts and adds the residual into unfiltered planes, k_vp8_filter runs
// the loop filter over them, k_vp8_rgb upsamples the chroma and writes pix.
// A broken stream sets ImageDesc::status and Vp8Desc::fail (kVp8Fail*, dg_vp8.h) names it.
// With an ALPH chunk (option "webp_alpha") the image is Rgba8: k_alph_plane (dg_alph.hip) unfilters the
// alpha plane from the chunk's raw bytes or from the green channel of a companion descriptor's VP8L
// plane (fmt kFmtWebp, behind the batch's images: k_vp8l_decode / k_vp8l_inverse decode it through
// their own list), and k_vp8_rgb stores it as the fourth channel.
struct Vp8Desc {
  uint64_t src;          // the VP8 chunk's payload (the frame tag), in the file
  uint64_t work;         // work arena: layout_vp8(width, height).bytes
  uint32_t nbytes;       // the chunk's bytes (loads stay below src + nbytes)
  uint32_t part0;        // bytes of the first partition, after the 10-byte frame header
  uint32_t fail;         // kVp8Fail*: written by k_vp8_parse
  uint32_t filter_type;  // written by k_vp8_parse: 0 no loop filter, 1 simple, 2 normal
  uint64_t alph_src;     // raw alpha: the ALPH payload after its header byte, in the file (0: VP8L-coded)
  uint64_t alph_plane;   // the unfiltered alpha plane, width x height bytes (0: no alpha)
  uint32_t alph_filter;  // kAlph* (dg_alph.h): none, horizontal, vertical, gradient
  uint32_t alph_desc;    // VP8L-coded alpha: index of the companion descriptor
  uint32_t alph_fail;    // written by k_alph_plane: the companion's status, when its stream failed
  uint32_t pad_;
};

// Adam7 pass p of a W x H image (PNG spec 8.2): origin (x0, y0), spacing (dx, dy)
DG_HD uint32_t png_a7(uint32_t p, uint32_t k) {
  // x0, y0, dx, dy of the pass, 4 bits each (no table: no scratch on the device)
  const uint32_t t = p == 0 ? 0x8800u : p == 1 ? 0x8804u : p == 2 ? 0x8440u : p == 3 ? 0x4402u
                   : p == 4 ? 0x4220u : p == 5 ? 0x2201u : 0x2110u;
  return (t >> (4 * k)) & 15u;
}
DG_HD void png_adam7_pass(uint32_t W, uint32_t H, uint32_t p, uint32_t &pw, uint32_t &ph) {
  const uint32_t x0 = png_a7(p, 0), y0 = png_a7(p, 1), dx = png_a7(p, 2), dy = png_a7(p, 3);
  pw = W > x0 ? (W - x0 + dx - 1) / dx : 0;
  ph = H > y0 ? (H - y0 + dy - 1) / dy : 0;
}
// Geometry of pass p of an interlaced image: size, unfiltered row bytes and
// 16-byte-aligned stride, offsets of its rows in raw and unf
struct A7Pass {
  uint32_t pw, ph, rb, us;
  uint64_t raw_off, unf_off;
};
DG_HD A7Pass png_adam7(uint32_t W, uint32_t H, uint32_t bitspp, uint32_t p) {
  A7Pass r = {0, 0, 0, 0, 0, 0};
  for (uint32_t q = 0; q <= p; q++) {
    uint32_t pw, ph;
    png_adam7_pass(W, H, q, pw, ph);
    const uint32_t rb = (uint32_t)(((uint64_t)bitspp * pw + 7) / 8), us = (rb + 15) / 16 * 16;
    if (q == p) {
      r.pw = pw;
      r.ph = ph;
      r.rb = rb;
      r.us = us;
    } else if (pw && ph) {
      r.raw_off += (uint64_t)ph * (rb + 1);
      r.unf_off += (uint64_t)ph * us;
    }
  }
  return r;
}

// Chunk-parallel inflate.  The zlib stream of a large PNG is cut into
// chunks of `span` bytes (option "inf_chunk", default kInfChunk).  k_inf_find looks in each chunk (but the first) for
// the first bit position that parses as a dynamic-Huffman block header with
// complete codes; k_inf_decode decodes, one lane per chunk, from there until
// it reaches a block boundary that another chunk starts at (or the end).  A
// match reaching before the chunk's start yields a marker (256 + index into
// the 32 KiB window preceding the chunk); k_inf_resolve walks the chain of
// chunks that the decode proved consistent and writes the bytes.  Anything
// irregular (no candidate chain, overflow, a decode error) sends the image to
// the serial inflate kernel.
constexpr uint32_t kInfChunk = 32768;          // compressed bytes per chunk
constexpr uint32_t kInfCapPerByte = 8;         // output entries per compressed byte of a chunk
constexpr uint32_t kInfNone = 0xFFFFFFFFu;
struct InfChunk {
  uint64_t out;       // uint16 entries: byte value, or 256 + window index
  uint64_t tab;       // per-chunk Huffman tables (k_inf_decode scratch)
  uint32_t image;     // descriptor index
  uint32_t idx;       // chunk index within the image
  uint32_t cap;       // capacity of out (entries)
  uint32_t start;     // bit position of the chunk's first block (kInfNone: no candidate)
  uint32_t len;       // entries produced
  uint32_t stop;      // chunk index whose start the decode reached (nchunks: end of stream)
  uint32_t status;    // 0 ok, 1 decode error, 2 overflow
  uint32_t span;      // compressed bytes per chunk of this image
};
constexpr uint32_t kInfTabBytes = 4096;        // per-chunk table scratch (see k_inf_decode)
// A gather job: copy `len` bytes (one IDAT payload) from src to dst.  With count != 0 a run of a GIF's
// sub-block chain (k_gif_gather): `count` blocks of `len` data bytes, each behind its length byte, from src
// (the first length byte) to len * count contiguous bytes at dst.
struct GatherJob {
  uint64_t src, dst;
  uint32_t len, count;
};
constexpr uint32_t kGatherPiece = 16384;  // bytes per gather workgroup

// fast_image_resize mul_div_alpha (U8x2 / U8x4): an in-place program over one
// buffer.  prog holds up to three 2-bit ops, lowest first: 1 = multiply
// colour by alpha, 2 = divide by alpha.
struct AlphaOp {
  uint64_t buf;
  uint32_t stride, width, rows, prog;
  uint32_t on_decoded;  // buf is the decoded image (not re-created by a resync round)
  uint32_t pad;
};
constexpr uint32_t kAlphaPoints = 3;  // before call 1, between the calls, after call 2

// ---- JPEG re-encode (pre_encode_images + encode_format jpeg,
// image_processing.rs:374-395): image 0.25's baseline encoder, 1x1 sampling,
// Annex K tables scaled by quality.  Per image: k_enc_fdct (colour + FDCT +
// quantisation per MCU), k_enc_count (bits per block), k_enc_scan (bit
// offsets), k_enc_write (codes OR-ed into a zeroed bit buffer), k_enc_stuff
// (header, 0xFF00 stuffing, padding, EOI).  Option "jenc_optimize": k_enc_hist
// and k_enc_tree after fdct give each image EncTables and DHT segments of its
// own (dg_jenc_tree.h).
struct EncTables {
  uint16_t code[4][256];  // DC luma, AC luma, DC chroma, AC chroma
  uint8_t len[4][256];
};
constexpr uint32_t kPencTabBytes = 1280;  // png, option "penc_dynamic": 288 words of histogram / code table, padded to 256
struct EncDesc {
  uint64_t src;        // the transformed image (C channels, row stride src_stride)
  uint64_t coef;       // int16 [nblocks][64], quantised, zigzag order, MCU-interleaved blocks
  uint64_t bits;       // uint32 [nblocks]: bit length of each block -> exclusive bit offsets
  uint64_t words;      // scan bit buffer (stream bytes in memory order), zeroed per batch
  uint64_t out;        // header | stuffed scan | EOI
  uint64_t hdr;        // header bytes (SOI .. SOS)
  uint64_t tab;        // EncTables; png: 0, or with option "penc_dynamic" the image's 288 words that hold the
                       // literal/length histogram (zeroed per batch) and then, for a dynamic block, its code table
  uint32_t src_stride, C, ncomp, mode;  // C: bytes per pixel (channels; png of 16-bit samples, option "penc16":
                                        // 2 x channels); mode 1: resized LA image read as luma bytes
  uint32_t w, h, nbx, nby;
  uint32_t nblocks, hdr_len, total_bits, enc_bytes;
  uint32_t active, png;  // png: PNG re-encode (dg_penc.hip): coef = filtered stream,
                         // nblocks = 1 KiB pieces, bits = piece bit lengths
  uint32_t hdr_bits;     // png: bits in front of the first token: 3, or the dynamic block's header (k_penc_tree)
  uint16_t dyn, eob_len; // png: 1 = dynamic block (k_penc_tree chose it); bits of the end-of-block code (7 fixed)
                         // jpeg: dyn 1 = the image's own Huffman tables and DHT segments (k_enc_tree)
  uint64_t aux;                  // png: Adler-32 partials per piece (uint32 x 2)
  // jpeg, option "jenc_optimize" (dg_jenc_tree.h): jopt = the image's histogram / EncTables / DHT region (0: option
  // off).  k_enc_tree sets tab, hdr_len, dht_len and dyn = 1 for an image that takes its own tables, and puts
  // tab_std, hdr_std and dyn = 0 back for one that keeps the standard ones.
  uint64_t jopt, tab_std;
  uint32_t hdr_std, dht_len;
  uint16_t hdr_pre, hdr_sos;     // the host's header: bytes in front of its DHT segments; offset of its SOS segment
  uint8_t q[2][64];    // quantisation tables, natural order
};

// ---- non-interleaved baseline JPEG (option "jpeg_multiscan"): a sequential file whose scans each carry one or
// two of the frame's three components.  The image keeps one descriptor, the parent (geometry, planes, resize
// plan, output, one MCU-interleaved coef / ccnt buffer); each scan gets an entropy-only descriptor of its own
// behind the batch's image descriptors (stream, subsequences, tables, restart interval; coef / ccnt are the
// parent's).  A scan decodes its blocks in its own order -- a one-component scan the component's own grid
// ceil(cdsw / 8) x ceil(cdsh / 8) row by row (T.81 A.2.2), an interleaved one the frame's MCU grid with the MCU
// cut down to its components -- and k_huff_write's multiscan instantiation stores block g of the scan at
// ms_index(map, g) of the parent.  The blocks between a component's own grid and the MCU-padded grid are coded
// by no scan: k_ms_zero clears them before the write.
constexpr uint32_t kMsParent = 1, kMsScan = 2;
struct ScanMap {
  uint32_t role;        // 0: an ordinary image, kMsParent, kMsScan
  uint32_t div, recip;  // one component: its own grid width; interleaved: the scan's blocks per MCU.
                        // recip = min(floor(2^32 / div), 2^32 - 1)
  uint32_t mcux, bpm;   // the parent's MCUs per row and blocks per MCU
  uint8_t inter;        // 1: two components, interleaved
  uint8_t lh, lv;       // one component: log2 of its sampling factors (1, 2 or 4)
  uint8_t na;           // interleaved: blocks of the scan's first component per MCU
  uint8_t cf0, cf1;     // first block of the scan's first / second component within the parent's MCU
  uint8_t pad[2];
  uint32_t pad64[9];    // 64 bytes: ImageDesc stays a whole number of 64-byte lines (it was 21 of them), so
                        // every descriptor of the array starts on one, as before
};
static_assert(sizeof(ScanMap) == 64, "ScanMap is one 64-byte line");
DG_HD uint32_t ms_recip(uint32_t div) { return div <= 1u ? 0xFFFFFFFFu : (uint32_t)(0x100000000ull / div); }
// g / div for any g: the multiply-high is the quotient or one below it
DG_HD uint32_t ms_div(uint32_t g, uint32_t div, uint32_t recip, uint32_t &rem) {
  uint32_t q = (uint32_t)(((uint64_t)g * recip) >> 32);
  uint32_t r = g - q * div;
  const bool up = r >= div;
  q += up ? 1u : 0u;
  r -= up ? div : 0u;
  rem = r;
  return q;
}
// Block (by, bx) of a component (first block cf of the MCU, sampling 1 << lh by 1 << lv) in MCU-interleaved order
DG_HD uint32_t ms_block_index(uint32_t mcux, uint32_t bpm, uint32_t cf, uint32_t lh, uint32_t lv, uint32_t by,
                              uint32_t bx) {
  const uint32_t hm = (1u << lh) - 1u, vm = (1u << lv) - 1u;
  return ((by >> lv) * mcux + (bx >> lh)) * bpm + cf + ((by & vm) << lh) + (bx & hm);
}
// Decode index g of a scan -> block index of the parent
DG_HD uint32_t ms_index(const ScanMap &m, uint32_t g) {
  uint32_t r;
  const uint32_t q = ms_div(g, m.div, m.recip, r);
  if (m.inter) return q * m.bpm + (r < m.na ? m.cf0 + r : m.cf1 + (r - m.na));
  return ms_block_index(m.mcux, m.bpm, m.cf0, m.lh, m.lv, q, r);
}

struct ImageDesc {
  // ---- entropy stream
  uint64_t scan;            // device address of the first raw entropy-coded byte
  uint32_t scan_len;        // raw bytes of entropy-coded data (EOI excluded)
  uint32_t nsub;            // subsequences (sized from the raw length)
  uint32_t sub_base;        // first SubState index
  uint32_t sub_bits;        // bits per subsequence (per image: option "sub_density")
  uint32_t ckpt_base;       // first checkpoint record of this image (nsub * num_ckpt(sub_bits) of them)
  uint64_t ds;              // destuffed stream, word-interleaved (ds_word_index), >= 64 zero bytes past its end
  uint64_t mk;              // RST marker positions in ds (bits), ascending
  uint64_t chunk;           // destuff per-chunk records: uint32 {cnt, mkc, off, mkoff}
  uint32_t nchunk;          // raw chunks of kDestuffChunk bytes
  uint32_t ds_state0;       // k_destuff_one: index of chunk 0's state word (batch-wide, list order)
  uint32_t ds_bits;         // destuffed length in bits (written by k_destuff_scan)
  uint32_t nmk;             // RST markers (written by k_destuff_scan)
  uint32_t slotmap;         // Huffman slot of (component c, dc=0/ac=1) at nibble 2c+ac
  uint32_t mk_cap;          // capacity of the marker list
  uint32_t lead_bits;       // k_huff_sync lead-in before each subsequence (lead_in)
  uint32_t ds_lsw;          // log2(32-bit words per subsequence) of the interleaved stream
  uint32_t ckpt;            // 1: k_huff_sync / k_huff_fix record checkpoints for early merging (option "ckpt")
  uint32_t idct_fused;      // 1: k_huff_write turns completed blocks into plane pixels (option "idct_fused")
  uint32_t stage_cap;       // decode-once: staging capacity per subsequence (groups of 4 entries), 0 = off
  uint32_t restart;         // restart interval (MCUs), 0 = none
  uint32_t blocks_per_seg;  // restart * bpm, 0 = unlimited
  uint32_t total_blocks;
  uint32_t bpm;             // blocks per MCU
  uint32_t comp_bits;       // component of block k within an MCU at bits 2k..2k+1
  uint8_t blk_comp[12];     // same, unpacked (host side / IDCT)
  uint16_t hslot[kMaxSlots];  // pool index of Huffman slot s
  uint8_t ncomp, colorspace, dec_c, nslots;  // dec_c: channels of the decoded image
  uint16_t qpool[4];
  uint16_t sem;             // decode semantics: 0 libjpeg-turbo, 1 zune-jpeg (option "decode_semantics")
  uint64_t coef;            // device address of block 0 (int16 zigzag[64] per block, decode order)
  uint64_t stage;           // decode-once staging (dg_entropy.h StageCtx), 0 = off
  // Sparse coefficient blocks (option "sparse_coef"): one byte per block, the
  // mask of the 16-byte zigzag parts k_huff_write stored (its nonzero ones;
  // 0xFF for a block two ranges share); k_idct_t loads only those parts and
  // takes the rest as zero.  0 = dense blocks (every part written and read).
  uint64_t ccnt;
  // ---- geometry
  uint32_t width, height;
  uint32_t mcux, mcuy;
  uint32_t hmax, vmax;
  uint32_t ch[4], cv[4];    // sampling factors
  uint32_t cfirst[4];       // first block of component c within an MCU
  uint32_t cbw[4], cbh[4];  // plane size in blocks
  uint32_t cdsw[4], cdsh[4];// downsampled width/height (libjpeg downsampled_width)
  uint64_t plane[4];        // device address of component planes (stride cbw*8)
  uint64_t pix;             // decoded interleaved RGB image (stride pix_stride), 0 for gray
  uint32_t pix_stride;
  int32_t status;           // set by kernels on corruption
  // ---- resize plan
  ResizePass pass[kStages];
  uint64_t out;             // final output (tight rows)
  uint32_t out_w, out_h, out_c, out_stride;
  uint64_t final_src;       // copy-kernel source (no pass runs, or gray->RGB expansion)
  uint32_t final_src_stride, copy_needed;
  uint32_t final_src_c;
  uint32_t color_fused;     // 1: pass[0] converts colour itself, pix is never written
  // ---- format, PNG, alpha handling, final conversion
  uint32_t fmt;             // kFmtJpeg / kFmtPng / kFmtGif / kFmtWebp / kFmtVp8 / kFmtBmp
  uint32_t prog;            // progressive JPEG: scans decoded by k_prog_scan (0: sequential)
  uint32_t crec;            // bit c: component c's plane holds chroma records (dg_plane.h; option "chroma_rec")
  uint32_t copy_mode;       // k_copy: 0 same channels, 1 L->RGB, 2 RGBA->RGB blend over gray,
                            // 3 LA->RGB of a resized LA image (GrayImage over the LA bytes, B3),
                            // 4 LA->RGB of an unresized LumaA8 (alpha dropped),
                            // 5 16-bit samples, same channels, 6 16-bit L / LA / RGB / RGBA -> RGB8
                            // ((v + 128) / 257 per sample, luma replicated, alpha dropped)
  uint32_t sample_bytes;    // bytes per sample of the decoded image and, unless copy_mode 6, of the output: 1 or 2
  union {
    PngDesc png;            // fmt == kFmtPng
    GifDesc gif;            // fmt == kFmtGif
    Vp8lDesc vp8l;          // fmt == kFmtWebp
    Vp8Desc vp8;            // fmt == kFmtVp8
    BmpDesc bmp;            // fmt == kFmtBmp
  };
  AlphaOp aop[kAlphaPoints];
  EncDesc enc;
  ScanMap ms;               // option "jpeg_multiscan": the parent of scan descriptors, or one of them
};

static_assert(sizeof(ImageDesc) % 64 == 0, "descriptors start on 64-byte lines");

// The map of a scan of ns (1 or 2) components comp[] of parent `par` (its geometry set), and the blocks the
// scan codes: a component's own grid, or the frame's MCU grid times the scan's blocks per MCU.
DG_HD ScanMap ms_scan_map(const ImageDesc &par, uint32_t ns, const int *comp, uint32_t &total_blocks) {
  ScanMap m = {};
  m.role = kMsScan;
  m.mcux = par.mcux;
  m.bpm = par.bpm;
  const uint32_t c0 = (uint32_t)comp[0];
  m.cf0 = (uint8_t)par.cfirst[c0];
  if (ns == 1) {  // the component's own grid, row by row (T.81 A.2.2)
    const uint32_t gw = (par.cdsw[c0] + 7) / 8, gh = (par.cdsh[c0] + 7) / 8;
    m.div = gw;
    m.lh = (uint8_t)(par.ch[c0] >> 1);  // log2 of 1, 2, 4
    m.lv = (uint8_t)(par.cv[c0] >> 1);
    total_blocks = gw * gh;
  } else {  // the frame's MCU grid, the MCU cut down to the scan's two components (A.2.3)
    const uint32_t c1 = (uint32_t)comp[1];
    m.inter = 1;
    m.na = (uint8_t)(par.ch[c0] * par.cv[c0]);
    m.div = m.na + par.ch[c1] * par.cv[c1];
    m.cf1 = (uint8_t)par.cfirst[c1];
    total_blocks = par.mcux * par.mcuy * m.div;
  }
  m.recip = ms_recip(m.div);
  return m;
}

// ---- progressive JPEG (ImageDesc::prog > 0).  The coefficient blocks are
// zeroed (k_prog_zero), then every scan is decoded by one wave of k_prog_scan
// straight from the stuffed bytes.  Scans that touch disjoint (component,
// coefficient band) sets are independent; the host gives each scan a level
// (1 + the highest level of an earlier overlapping scan) and the list of
// those earlier scans (deps).  All scans of a batch run in one launch,
// taken in level order; a scan waits, chunk by chunk, only until its deps
// have written the MCU rows it is about to read (a pipeline over the
// image's rows instead of a barrier per level).
struct ProgScan {
  uint64_t data;        // device address of the scan's first entropy-coded byte
  uint32_t len;         // entropy-coded bytes (up to the next non-RST marker)
  uint32_t image;       // descriptor index
  uint32_t ns;          // components in the scan
  uint32_t comp[4];     // their component indices
  uint16_t dc[4];       // DC-first scans: Huffman pool index per scan component
  uint16_t ac;          // AC scans: Huffman pool index
  uint16_t pflags;      // kProgChained: the scan runs after its deps in the same work item (no waits)
  uint32_t ss, se, ah, al;
  uint32_t restart;     // restart interval (MCUs; blocks when ns == 1), 0 = none
  uint32_t level;
  uint32_t first;       // batch index of the image's first scan
  uint32_t next;        // next scan of the same work item (chain), kProgNoScan = none
  uint64_t deps;        // earlier scans of the image this one reads (bit e = scan first + e)
};
// Pipelined scans (one launch per batch): progress word of scan j =
// flags[1 + j], in MCU rows whose blocks the scan has written (kProgDone
// when finished); flags[0] hands out scans to workgroups in list order.
constexpr uint32_t kProgDone = 0xFFFFFFFFu;
constexpr uint32_t kProgNoScan = 0xFFFFFFFFu;
constexpr uint16_t kProgChained = 1;
constexpr uint32_t kProgMaxScans = 256;    // per image (the parser's limit)
constexpr uint32_t kProgMaxDepScans = 64;  // deps is a 64-bit mask: images with more scans run chained only
constexpr uint32_t kProgZeroBytes = 65536;  // coefficient bytes zeroed per k_prog_zero workgroup

// One workgroup's work: an image and the first item it handles.
struct WgItem {
  uint32_t image;
  uint32_t item0;
};

// Batch-wide flags written by kernels (zeroed before each batch).
struct BatchFlags {
  uint32_t chain_changed;   // k_huff_fix changed a workgroup's last exit state
  uint32_t fix_count;       // workgroups k_huff_fix had to re-run
  uint32_t write_mismatch;  // k_huff_write exit != next subsequence's input
  uint32_t sync_iters_max;  // longest intra-workgroup sync loop
  uint32_t idct_late;       // fused IDCT: blocks k_huff_write left to k_idct_list (entries in idct_list)
  uint32_t png_next;        // k_png_inflate mode 1: next list entry a workgroup claims
  uint64_t wgtime;          // debug: device array of {start, end} s_memrealtime per workgroup, 0 = off
  uint32_t wgtime_write;    // first record of k_huff_write's workgroups
  uint32_t debug;           // test switches (kDbg*), kept across resync rounds
  uint64_t idct_list;       // fused IDCT: uint32 {image, block} pairs, idct_cap of them
  uint32_t idct_cap;
  uint32_t prio;            // option "entropy_prio": wave issue priority of k_huff_sync / k_huff_write (0-3)
};
// The counters a resync round clears (everything before `wgtime`).
constexpr size_t kFlagCounters = 24;
// BatchFlags::debug: force the failure paths a valid stream never takes, so
// tests can check that they surface as a per-image status.
constexpr uint32_t kDbgForceWriteMismatch = 1u;  // k_huff_write: subsequence 0 of every image disagrees
constexpr uint32_t kDbgForceChainChange = 2u;    // k_huff_fix: the chain never settles

}  // namespace dg
