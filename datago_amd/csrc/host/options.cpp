// options.cpp — the option table: one row per dg_ctx_set_option key.
//
// A row names its field in Options, the values it takes and the text a
// rejected value gets in dg_last_error.  What a key does beyond storing a
// value (a lock, streams made again, a cache started over) is its "after" tag,
// carried out by Context::set_option.  The older flags take any value
// (v != 0); the newer ones (STRICT) take 0 and 1 only: callers rely on both.
#include "options.h"

#include <string.h>

namespace dg {

static_assert(sizeof(size_t) == sizeof(uint64_t), "size_t fields are kOptU64");
static_assert(kMaxInflight == 6, "the texts of \"slots\" and \"coalesce_inflight\" spell it out");

namespace {

template <class T> constexpr OptType opt_type();
template <> constexpr OptType opt_type<bool>() { return kOptBool; }
template <> constexpr OptType opt_type<int>() { return kOptInt; }
template <> constexpr OptType opt_type<uint32_t>() { return kOptU32; }
template <> constexpr OptType opt_type<int64_t>() { return kOptI64; }
template <> constexpr OptType opt_type<uint64_t>() { return kOptU64; }
template <> constexpr OptType opt_type<double>() { return kOptDouble; }

constexpr int64_t kNoMax = INT64_MAX;

#define DG_STR2(x) #x
#define DG_STR(x) DG_STR2(x)
// {name, field, kind, lo, hi, except, shift, why, after}
#define F(f) offsetof(Options, f), opt_type<decltype(Options::f)>()
#define FLAG(key, f) {key, F(f), kOptFlag, 0, 0, 0, 0, nullptr, kAfterNone}
#define STRICT(key, f) {key, F(f), kOptRange, 0, 1, 0, 0, "valid unless v < 0 || v > 1", kAfterNone}
#define RANGE(key, f, lo, hi, why) {key, F(f), kOptRange, lo, hi, 0, 0, why, kAfterNone}
#define POW2(key, f, lo, hi, why) {key, F(f), kOptPow2, lo, hi, 0, 0, why, kAfterNone}
#define POW2_OR_0(key, f, lo, hi, why) {key, F(f), kOptPow2Or0, lo, hi, 0, 0, why, kAfterNone}
#define RAW(key, f) {key, F(f), kOptRaw, 0, 0, 0, 0, nullptr, kAfterNone}

}  // namespace

const OptRow kOptionTable[] = {
    POW2_OR_0("sub_bits", sub_bits, 64, 65536, "valid unless v != 0 && (v < 64 || v > 65536 || (v & (v - 1)))"),
    POW2("sub_auto", sub_auto, 1024, 65536, "valid unless v < 1024 || v > 65536 || (v & (v - 1))"),
    RANGE("lead_bits", lead_bits, -1, 1 << 20, "valid unless v < -1 || v > (1 << 20)"),
    {"coalesce_max", F(coalesce_max), kOptRange, 1, 4096, 0, 0, "valid unless v < 1 || v > 4096", kAfterCoalesce},
    // dg_decode_one: coalesced baseline batches in flight (0 = "slots")
    {"coalesce_inflight", F(coalesce_inflight), kOptRange, 0, kMaxInflight, 0, 0, "valid unless v < 0 || v > 6",
     kAfterCoalesce},
    {"coalesce_us", F(coalesce_us), kOptRange, 0, 1000000, 0, 0, "valid unless v < 0 || v > 1000000", kAfterCoalesce},
    FLAG("wg_timing", wg_timing),
    FLAG("timing", timing),
    FLAG("side_stream", side_stream),
    // Lanczos table cache arena (0: off); takes effect at the next reset
    {"coef_cache_mb", F(ccache_cap), kOptRange, 0, 65536, 0, 20, "valid unless v < 0 || v > 65536", kAfterCoefCache},
    // wave issue priority (s_setprio) of the entropy kernels, 0-3
    RANGE("entropy_prio", entropy_prio, 0, 3, "valid unless v < 0 || v > 3"),
    // device memory budget of the context (0: none)
    {"max_device_mb", F(max_dev_bytes), kOptRange, 0, kNoMax, 0, 20, "valid unless v < 0", kAfterMaxDevice},
    // 1: the first batch under a budget sizes every slot (no growth later); 0: grow and trade
    {"budget_plan", F(budget_plan), kOptFlag, 0, 0, 0, 0, nullptr, kAfterBudgetPlan},
    {"slots", F(nslots), kOptRange, 1, kMaxInflight, 0, 0, "valid unless v < 1 || v > 6", kAfterSlots},
    // Progressive JPEGs on the GPU (dg_prog.hip; default on).  A refinement
    // scan decodes serially in one wave, so a large file takes ~0.1-1 s: the
    // progressive members of a submission run apart from the rest (prog_split)
    // in aggregate batches on slots of their own.  0: DG_ERR_UNSUPPORTED (the
    // caller's CPU decoder takes them).
    FLAG("progressive", progressive),
    // 16-bit PNGs on the GPU (default off: DG_ERR_UNSUPPORTED, the caller's CPU
    // decoder takes them).  1: they decode to native-endian u16 samples
    // (bit_depth 16), or to RGB8 under image_to_rgb8; a 16-bit image that would
    // need the resize or an encoder stays DG_ERR_UNSUPPORTED unless "resize16" /
    // "penc16" take it.
    STRICT("png16", png16),
    // GIF87a / GIF89a files on the GPU (default off: DG_ERR_CORRUPT like any
    // format the library does not know).  1: plan_image takes a GIF, its first
    // frame is LZW-decoded by k_gif_lzw and composited on the logical screen as
    // Rgba8 by k_gif_expand (dg_gif.hip), what image 0.25's GifDecoder returns
    // for load_from_memory; from there it is an RGBA8 PNG's pixels.  Stream
    // irregularities come back DG_ERR_UNSUPPORTED with a dg_last_error text.
    // dg_probe names a GIF either way and keeps describing the default options.
    STRICT("gif", gif),
    // Still lossless WebP files (a VP8L image chunk, simple or behind VP8X) on the
    // GPU (default off: DG_ERR_CORRUPT like any format the library does not
    // know).  1: plan_image takes the file, k_vp8l_decode reads the bitstream,
    // k_vp8l_inverse undoes the transforms and k_vp8l_store writes Rgba8 when
    // the file says it has alpha (the VP8L header's bit, or the VP8X flag of an
    // extended file) and Rgb8 otherwise (dg_vp8l.hip): what image 0.25's
    // WebPDecoder returns for load_from_memory.  From there it is an 8-bit RGB /
    // RGBA PNG's pixels.  Animated and extended lossy files come back
    // DG_ERR_UNSUPPORTED, a simple lossy file stays an unknown format.
    // dg_probe names a lossless or extended WebP either way and keeps
    // describing the default options.
    STRICT("webp", webp),
    // Colour JPEGs with a component at the full horizontal and half the
    // vertical rate (4:4:0, what a lossless 90-degree rotation makes of 4:2:2;
    // default off: DG_ERR_UNSUPPORTED, the caller's CPU decoder takes them).
    // 1: parse_jpeg_header accepts them and upsample8 / upsample8_zune blend the
    // two nearest plane rows 3:1 (kernels.hip).  dg_probe keeps describing the
    // default options.
    STRICT("jpeg_h1v2", jpeg_h1v2),
    // Four-component JPEGs with an Adobe APP14 segment of transform 0 (CMYK)
    // or 2 (YCCK) (default off: DG_ERR_UNSUPPORTED "CMYK/2-component JPEG").
    // 1: parse_jpeg_header accepts them, the batch's entropy passes run their
    // four-component instantiations and k_cmyk (kernels.hip) writes the RGB
    // image that image 0.25 returns for them.  dg_probe keeps describing the
    // default options.
    STRICT("jpeg_cmyk", jpeg_cmyk),
    // Three-component sequential JPEGs whose scans carry one or two components
    // each (non-interleaved; default off: DG_ERR_UNSUPPORTED "non-interleaved
    // multi-scan JPEG").  1: parse_jpeg_header walks their scans, every scan
    // becomes an entropy-only descriptor behind the batch's images and the
    // batch's k_huff_write runs its multiscan instantiation, which stores each
    // scan's blocks in the image's MCU-interleaved order (ms_index, dg_types.h).
    // dg_probe keeps describing the default options.
    STRICT("jpeg_multiscan", jpeg_multiscan),
    // 16-bit PNGs that are not their bucket's size (default off:
    // DG_ERR_UNSUPPORTED).  1, together with "png16": they resize with the
    // image crate's resize_to_fill(Lanczos3), which the reference uses for
    // every non-U8 pixel type (dg_resize16.h); 16-bit into an encoder stays
    // DG_ERR_UNSUPPORTED unless "penc16" is on.
    STRICT("resize16", resize16),
    // 16-bit PNGs into the PNG re-encoder (default off: DG_ERR_UNSUPPORTED).  1,
    // together with "png16" (and "resize16" for an image that is not its
    // bucket's size): under pre_encode_images with encode_format png the
    // transformed samples come back as a bit-depth-16 PNG, as the reference's
    // PngEncoder writes an ImageLuma16 / LumaA16 / Rgb16 / Rgba16
    // (k_penc_filter16, dg_penc16.h).  The JPEG encoder takes 8-bit samples
    // only.  8-bit images and image_to_rgb8 contexts are untouched.
    STRICT("penc16", penc16),
    // PNG re-encode (pre_encode_images, encode_format png): 1 = an image whose
    // DEFLATE block is strictly shorter under a Huffman code built from its own
    // histogram takes a dynamic block (dg_penc_tree.h); every other image, and
    // every image with 0 (the default), takes the fixed block byte for byte as
    // before.  Nothing changes for JPEG re-encoding.
    STRICT("penc_dynamic", penc_dynamic),
    // JPEG re-encode (pre_encode_images, encode_format jpeg): 1 = every image is
    // coded with Huffman tables built from its own symbol counts by libjpeg's
    // jpeg_gen_optimal_table rule (dg_jenc_tree.h) and carries them in its DHT
    // segments; everything else in the file is unchanged.  An image in which
    // the rule meets a code size above 32, and every image with 0 (the
    // default), takes the Annex K tables byte for byte as before.  Nothing
    // changes for PNG re-encoding.
    STRICT("jenc_optimize", jenc_optimize),
    // dg_decode_one: progressive batches in flight on the progressive slots; 0: mixed in
    RANGE("prog_lanes", prog_lanes, 0, kProgSlots, "valid unless v < 0 || v > " DG_STR(DG_PROG_SLOTS)),
    // progressive slots' streams: 0 plain, 1 high / 2 low priority, 3 CU-masked
    {"prog_queue", F(prog_queue), kOptRange, 0, 3, 0, 0, "valid unless v < 0 || v > 3", kAfterProgQueue},
    // baseline slots' streams: 0 plain, 1 high / 2 low priority, 3 CU-masked (own queues)
    {"slot_queue", F(slot_queue), kOptRange, 0, 3, 0, 0, "valid unless v < 0 || v > 3", kAfterSlotQueue},
    // the baseline slots' side streams: -1 as slot_queue, else a slot_queue mode
    {"side_queue", F(side_queue), kOptRange, -1, 3, 0, 0, "valid unless v < -1 || v > 3", kAfterSlotQueue},
    // prog_queue 3: CUs the progressive streams may use (0 = all); set before prog_queue
    RANGE("prog_cus", prog_cus, 0, 4096, "valid unless v < 0 || v > 4096"),
    // dg_submit: progressive members into the progressive aggregate (0: decoded in the batch)
    FLAG("prog_split", prog_split),
    // progressive aggregate: launched once it holds this many images
    RANGE("prog_batch", prog_batch, 1, 65536, "valid unless v < 1 || v > 65536"),
    // ... or once it is this old at a submit / poll / wait_ready
    RANGE("prog_flush_us", prog_flush_us, 0, 100000000, "valid unless v < 0 || v > 100000000"),
    FLAG("sync2", sync2),          // k_huff_sync2: two lead-in + range chains per lane (0: one, k_huff_sync)
    FLAG("sync_pair", sync_pair),  // k_huff_sync: a second AC symbol per single step from the same peek (A/B)
    // k_huff_sync: up to v more multi entries per state-only step from the same peek (0..3)
    RANGE("sync_chain", sync_chain, 0, 3, "valid unless v < 0 || v > 3"),
    // k_huff_write: up to v more AC symbols per step from the same peek (0..3)
    RANGE("write_pair", write_pair, 0, 3, "valid unless v < 0 || v > 3"),
    FLAG("multi_lead", multi_lead),  // multi-symbol AC steps in k_huff_sync's lead-in (A/B)
    FLAG("prog_side", prog_side),    // progressive scans on the side stream, beside the baseline entropy decode
    // chain dependency groups costing <= this % of the batch's longest scan (0: off)
    RANGE("prog_chain", prog_chain, 0, 100000, "valid unless v < 0 || v > 100000"),
    FLAG("prog_pipe", prog_pipe),        // 0: one k_prog_scan launch per level (A/B)
    FLAG("prog_serial", prog_serial),    // every progressive scan on the serial reader (A/B; restart scans always are)
    FLAG("entropy_once", entropy_once),  // decode-once: k_huff_sync stages coefficients, k_huff_scatter writes them
    FLAG("entropy_lpt", entropy_lpt),
    RANGE("hb_bands", hb_bands, 1, 64, "valid unless v < 1 || v > 64"),  // band H kernel: 8-row bands per workgroup
    FLAG("idct_fused", idct_fused),  // IDCT inside k_huff_write's block flush (default 0: measured slower)
    FLAG("idct_thread", idct_thread),
    FLAG("sparse_coef", sparse_coef),
    FLAG("h_prefetch", h_prefetch),
    FLAG("h_planar", h_planar),
    FLAG("destuff_one", destuff_one),
    FLAG("chroma_rec", chroma_rec),
    // zero the host_us_* / host_cpu_us_* stats
    {"reset_host_us", 0, kOptNone, kOptSignal, 0, 0, 0, 0, nullptr, kAfterResetHostUs},
    FLAG("hv_fused", hv_fused),  // fused first H + V pass of colour JPEGs where it fits (default 0: slower)
    // host threads for the output copies of a host-out batch (default 8)
    RANGE("copy_threads", copy_threads, 1, 64, "valid unless v < 1 || v > 64"),
    FLAG("ckpt", ckpt),  // entropy checkpoints for early merging of re-decodes (default 1)
    // 0: libjpeg-turbo (pinned), 1: zune-jpeg 0.5.12 restated (unpinned)
    RANGE("decode_semantics", decode_sem, 0, 1, "valid unless v != 0 && v != 1"),
    // batches under this many coded bytes take sub_small / lead_small (0 = off)
    RANGE("small_coded", small_coded, 0, kNoMax, "valid unless v < 0"),
    POW2("sub_small", sub_small, 64, 65536, "valid unless v < 64 || v > 65536 || (v & (v - 1))"),
    RANGE("lead_small", lead_small, 0, 1 << 16, "valid unless v < 0 || v > (1 << 16)"),
    // V pass output rows per column tile (k_resize_vt); 0: one thread per 16 output bytes
    POW2_OR_0("v_tile", v_tile, 2, 8, "valid: 0, 2, 4, 8"),
    RANGE("v_units", v_units, 1, 8, "valid unless v < 1 || v > 8"),  // k_resize_v: 256-unit strides per workgroup item
    // auto lead-in of images with >= 4-block MCUs (4:2:0), bits
    RANGE("lead_big", lead_big, 0, 1 << 16, "valid unless v < 0 || v > (1 << 16)"),
    FLAG("write_split", write_split),  // 1: k_huff_write decodes each range as two halves (see k_huff_write)
    // the GPU reads from page-locked staging: 1 the descriptors, 2 also host inputs
    RANGE("meta_pull", meta_pull, 0, 2, "valid unless v < 0 || v > 2"),
    // host threads parsing a submission's headers (1 = the caller only)
    RANGE("plan_threads", plan_threads, 1, 64, "valid unless v < 1 || v > 64"),
    // k_inf_find: Kraft survivors queued per full header check round
    POW2("inf_stage3", inf_stage3, 8, 64, "valid unless v != 8 && v != 16 && v != 32 && v != 64"),
    // chunk-parallel inflate: entries per chunk, in tenths of the image's expansion of a span
    RANGE("inf_cap", inf_cap, 10, 100, "valid unless v < 10 || v > 100"),
    FLAG("png_alias", png_alias),  // PNG chunk entries share device memory with the later stages' buffers
    // chunk-parallel inflate: entries per chunk on top of inf_cap's
    RANGE("inf_pad", inf_pad, 0, 1 << 20, "valid unless v < 0 || v > 2^20"),
    // compressed bytes per chunk of the chunk-parallel inflate
    POW2("inf_chunk", inf_chunk, 4096, 65536, "valid unless v < 4096 || v > 65536 || (v & (v - 1))"),
    // 0: every PNG inflates serially (test switch)
    {"png_chunked", F(chunked_off), kOptFlagInv, 0, 0, 0, 0, nullptr, kAfterNone},
    FLAG("lead_density", lead_density),
    // bits-per-block threshold for shorter subsequences (0 = off)
    RANGE("sub_density", sub_density, 0, 4096, "valid unless v < 0 || v > 4096"),
    // PNG unfilter: persistent workers per CU at most (0: as many as the LDS holds)
    RANGE("uf_per_cu", uf_per_cu, 0, 16, "valid unless v < 0 || v > 16"),
    // PNG unfilter: filter units per lane per step (1: half the LDS per worker)
    RANGE("uf_units", uf_units, 1, 2, "valid unless v < 1 || v > 2"),
    // k_inf_decode lookup bits (literal/length, distance): 0 9/7, 1 8/6, 2 7/6, 3 7/5, 4 6/5,
    // 5 6/4; 6, 7 = 2, 1 with the wave-batched register stream buffer; 8 / 9 / 11 =
    // 7/6, 6/5, 8/6 with the canonical walk's symbol tables in LDS; 12 / 13 = 8 / 9
    // with the register buffer; 14 = 0 with it, 15 = 11 with it; 16 = 3 with it;
    // 17 7/4, 18 8/5, 19 8/4; 20 / 21 / 22 = 17 / 4 / 5 with the register buffer;
    // 23 / 24 / 25 / 26 / 27 = 16 with a 4 / 12 / 16 / 24 / 32-word buffer;
    // 28 = 20 with a 16-word buffer
    {"inf_decode", F(inf_decode), kOptRangeBut, 0, 28, 10, 0, "valid unless v < 0 || v > 28 || v == 10", kAfterNone},
    FLAG("h_mfma", h_mfma),      // 0: band H passes with the VALU convolution (k_resize_hb, A/B)
    FLAG("band_dec", band_dec),  // 0: IDCT to planes + band H kernel (the split path, A/B)
    RAW("dec_dbg", dec_dbg),     // timing experiments: skip k_band_dec phases (wrong pixels)
    RANGE("dec_strips", dec_strips, 1, 4096, "valid unless v < 1 || v > 4096"),
    RAW("debug_flags", debug_flags),
};
const int kNumOptions = (int)(sizeof(kOptionTable) / sizeof(kOptionTable[0]));

// Rows added since tests/test_options_cpu.py wrote down kOptionTable's keys and
// defaults one by one: that test reads kOptionTable alone and holds it to
// exactly that list, so a later option stands here, with a test of its own
// (tests/test_vp8_cpu.py for "webp_lossy", tests/test_alph_cpu.py for
// "webp_alpha", tests/test_bmp_cpu.py for "bmp").  find_option looks through both,
// so to dg_ctx_set_option the two tables are one.
const OptRow kOptionTableAdded[] = {
    // Still lossy WebP files (a `VP8 ` image chunk, simple or behind VP8X, no
    // ALPH chunk) on the GPU (default off: nothing changes, see "webp").  1,
    // with or without "webp": plan_image takes the file, k_vp8_parse reads the
    // key frame's header, modes and tokens, k_vp8_recon predicts and adds the
    // residual, k_vp8_filter runs the loop filter and k_vp8_rgb writes Rgb8
    // with libwebp's fancy upsampling (dg_vp8.hip): what image 0.25's
    // WebPDecoder returns.  From there it is an 8-bit RGB PNG's pixels.  A
    // file with an ALPH chunk comes back DG_ERR_UNSUPPORTED "WebP: lossy WebP
    // with alpha", an animated one "WebP: animated WebP"; a broken frame
    // header or stream is DG_ERR_CORRUPT with a text.  A VP8L file is not this
    // option's.  dg_probe keeps describing the default options.
    STRICT("webp_lossy", webp_lossy),
    // With "webp_lossy" (alone it changes nothing, and it does not need
    // "webp"): a still lossy WebP whose VP8X alpha flag is set and which has
    // exactly one ALPH chunk before its `VP8 ` chunk decodes to Rgba8 with
    // non-premultiplied alpha, libwebp's MODE_RGBA bytes (default off: such a
    // file stays DG_ERR_UNSUPPORTED "WebP: lossy WebP with alpha").  The RGB
    // bytes are those of the `VP8 ` chunk alone.  The ALPH payload is a header
    // byte and then the filtered plane, raw or as the green channel of a
    // header-less VP8L stream, which k_vp8l_decode / k_vp8l_inverse decode
    // through a companion descriptor whether or not "webp" is set;
    // k_alph_plane (dg_alph.hip) undoes the horizontal, vertical or gradient
    // filter and k_vp8_rgb stores the fourth channel.  From there the image is
    // an RGBA8 PNG's pixels.  DG_ERR_CORRUPT with a text: a bad header byte, a
    // chunk of fewer than 2 bytes, a raw plane shorter than the image, a VP8L
    // alpha stream that does not decode.  DG_ERR_UNSUPPORTED with a text: a
    // second ALPH chunk, an ALPH chunk in a file whose VP8X alpha flag is
    // clear.  A file without an ALPH chunk before its image chunk decodes to
    // Rgb8 as with "webp_lossy" alone, whatever its flag.
    STRICT("webp_alpha", webp_alpha),
    // Windows bitmaps on the GPU (default off: DG_ERR_CORRUPT like any format
    // the library does not know).  1: plan_image takes a BMP; an RLE8 / RLE4
    // stream is decoded by k_bmp_rle, and k_bmp_expand writes Rgb8, or Rgba8
    // for a bit-field file with an alpha mask, top row first (dg_bmp.hip): what
    // image 0.25's BmpDecoder returns for load_from_memory, for the files it
    // and Pillow decode alike.  From there it is an 8-bit RGB / RGBA PNG's
    // pixels.  16-bit files, the other forms the two decoders disagree on and
    // stream irregularities come back DG_ERR_UNSUPPORTED with a dg_last_error
    // text.  dg_probe names a BMP either way and keeps describing the default
    // options.
    STRICT("bmp", bmp),
};
const int kNumOptionsAdded = (int)(sizeof(kOptionTableAdded) / sizeof(kOptionTableAdded[0]));

const OptRow *find_option(const char *key) {
  for (const OptRow &r : kOptionTable)
    if (!strcmp(r.name, key)) return &r;
  for (const OptRow &r : kOptionTableAdded)
    if (!strcmp(r.name, key)) return &r;
  return nullptr;
}

bool option_takes(const OptRow &r, int64_t v) {
  switch (r.kind) {
    case kOptRange: return v >= r.lo && v <= r.hi;
    case kOptRangeBut: return v >= r.lo && v <= r.hi && v != r.except;
    case kOptPow2: return v >= r.lo && v <= r.hi && !(v & (v - 1));
    case kOptPow2Or0: return v == 0 || (v >= r.lo && v <= r.hi && !(v & (v - 1)));
    default: return true;
  }
}

void store_option(const OptRow &r, Options &o, int64_t v) {
  void *p = (char *)&o + r.off;
  switch (r.type) {
    case kOptNone: break;
    case kOptBool: *(bool *)p = r.kind == kOptFlagInv ? v == 0 : v != 0; break;
    case kOptInt: *(int *)p = (int)v; break;
    case kOptU32: *(uint32_t *)p = (uint32_t)v; break;
    case kOptI64: *(int64_t *)p = v; break;
    case kOptU64: *(uint64_t *)p = (uint64_t)v << r.shift; break;
    case kOptDouble: *(double *)p = (double)v; break;
  }
}

OptResult apply_option(Options &o, const char *key, int64_t v, std::string *why) {
  const OptRow *r = find_option(key);
  if (!r) {
    *why = "unknown option";
    return kOptUnknown;
  }
  if (!option_takes(*r, v)) {
    *why = r->why;
    return kOptRejected;
  }
  store_option(*r, o, v);
  return kOptStored;
}

std::string option_error_text(const char *key, int64_t v, const std::string &why) {
  return std::string("dg_ctx_set_option(\"") + key + "\", " + std::to_string(v) + "): " + why;
}

}  // namespace dg
