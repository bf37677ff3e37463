// options.h — the context's options (dg_ctx_set_option): their state, and the
// one table that says which key sets which field and which values it takes.
// Host-only: no HIP header, so the table is checked without a GPU
// (tests/native/options_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../dg_types.h"

namespace dg {

// Three (option "slots", 1 to kMaxInflight) slots let the host plan and
// upload batch k+1 while the GPU still runs batches k and k-1.  kProgSlots
// more run progressive batches only (dg_submit's progressive aggregates,
// dg_decode_one's progressive lanes), so a ~0.1-1 s refinement chain never
// holds a baseline slot.
constexpr int kMaxInflight = 6;
#ifndef DG_PROG_SLOTS
#define DG_PROG_SLOTS 2
#endif
constexpr int kProgSlots = DG_PROG_SLOTS;  // (-DDG_PROG_SLOTS=n: experiment builds)

// What the option keys set: one field per key (Context::opt_).  Adding a plain
// option is a field here and a row in options.cpp.
struct Options {
  // entropy decode: subsequence sizes and the kernels' variants
  uint32_t sub_bits = 0;  // 0 = auto per batch (see submit)
  uint32_t sub_auto = 8192;  // the auto size of large batches
  int64_t lead_bits = -1;  // -1 = auto per image (see submit)
  uint32_t lead_big = 4096;        // option "lead_big" (6144 -> 4096 with 8192-bit ranges: +1.3%, profiles/r04/lead_big)
  uint64_t small_coded = 0;        // option "small_coded" (0: off)
  uint32_t sub_small = 512, lead_small = 1024;  // options "sub_small", "lead_small"
  double sub_density = 0;              // option "sub_density": bits per block below which subsequences shrink
  bool lead_density = false;           // option "lead_density": their lead-in shrinks by the same factor
  bool multi_lead = true;   // option "multi_lead": multi-symbol AC steps in k_huff_sync's state-only decodes
  int write_pair = 3;       // option "write_pair": up to this many more AC symbols per k_huff_write step from one peek
  bool sync2 = false;       // option "sync2": k_huff_sync with two chains per lane (k_huff_sync2)
  int sync_chain = 2;       // option "sync_chain": up to this many more multi entries per k_huff_sync step from one peek
  bool sync_pair = false;   // option "sync_pair": the same in k_huff_sync (measured slower beside multi_lead: off)
  bool write_split = true;         // option "write_split"
  bool ckpt = true;                    // option "ckpt"
  int entropy_prio = 0;  // option "entropy_prio"
  bool entropy_lpt = true;             // option "entropy_lpt": slow entropy workgroups first
  bool entropy_once = false;           // option "entropy_once": decode-once staging + k_huff_scatter
  bool destuff_one = false;            // option "destuff_one": single-pass destuff with decoupled look-back
                                       // (configs[1] 0.66 vs 0.43 ms three-pass: off)
  int decode_sem = 0;                  // option "decode_semantics"

  // IDCT, colour, resize
  bool idct_fused = false;             // option "idct_fused" (measured 7x slower k_huff_write: off)
  bool idct_thread = true;             // option "idct_thread": one lane per block (k_idct_t) instead of 8 (k_idct)
  bool sparse_coef = true;             // option "sparse_coef": k_huff_write stores, k_idct_t loads, only the
                                       // 16-byte parts through each block's last nonzero (ImageDesc::ccnt)
  bool chroma_rec = true;              // option "chroma_rec": half-rate chroma planes as 8-byte records (dg_plane.h)
  bool band_dec = false;               // option "band_dec": IDCT + colour + first H pass in k_band_dec
  uint32_t dec_dbg = 0;                // option "dec_dbg": k_band_dec phase switches (timing experiments only)
  uint32_t dec_strips = kDecStripsDefault;  // option "dec_strips"
  uint32_t hb_bands = kHBandsDefault;  // option "hb_bands"
  bool hv_fused = false;               // option "hv_fused": first H + V pass fused (k_resize_hv) when it fits
  bool h_prefetch = true;              // option "h_prefetch": specialised fused fills load the next band before the convolution
  bool h_planar = true;                // option "h_planar": fused 8/16-tap band passes over planar u16-pair segments (k_resize_hbp)
  bool h_mfma = false;                 // option "h_mfma": band H passes on the matrix cores (k_resize_hm; measured slower: off)
  uint32_t v_tile = 4;             // option "v_tile": V pass on R-row column tiles (k_resize_vt<R>; 0 = k_resize_v)
  uint32_t v_units = 2;            // option "v_units" (profiles/r04/v_units: 1 / 2 / 4 -> V traffic 1.95 / ? / 3.91 GB per batch)
  size_t ccache_cap = (size_t)256 << 20;  // option "coef_cache_mb": the Lanczos table cache's arena

  // PNG
  bool chunked_off = false;  // option "png_chunked" = 0
  uint32_t inf_chunk = kInfChunk;  // option "inf_chunk"
  uint32_t inf_cap = 30;           // option "inf_cap": chunk entries, tenths of the expansion of a span
  bool png_alias = true;           // option "png_alias": chunk entries alias the unfilter/resize buffers
  uint32_t inf_pad = 65536;        // option "inf_pad": chunk entries on top of inf_cap's
  uint32_t inf_stage3 = 32;        // option "inf_stage3"
  uint32_t inf_decode = 25;            // option "inf_decode": k_inf_decode shape (25 = 7/5 lookup bits, 20 KiB LDS
                                       // per wave, 16 stream words per lane in registers)
  int uf_per_cu = 0;     // option "uf_per_cu"
  uint32_t uf_units = 1;               // option "uf_units": PNG unfilter units per lane per step (1 or 2; round 5: 1)

  // formats and encoders that are off by default
  bool progressive = true;             // option "progressive"
  bool png16 = false;                  // option "png16": 16-bit PNGs decode on the GPU
  bool gif = false;                    // option "gif": a GIF's first frame decodes on the GPU (dg_gif.hip)
  bool bmp = false;                    // option "bmp": a Windows bitmap decodes on the GPU (dg_bmp.hip)
  bool webp = false;                   // option "webp": a lossless WebP decodes on the GPU (dg_vp8l.hip)
  bool webp_lossy = false;             // option "webp_lossy": a lossy WebP without alpha decodes on the GPU (dg_vp8.hip)
  bool webp_alpha = false;             // option "webp_alpha": with "webp_lossy", a lossy WebP with an ALPH chunk decodes as Rgba8 (dg_alph.hip)
  bool jpeg_h1v2 = false;              // option "jpeg_h1v2": 4:4:0-style JPEGs decode on the GPU
  bool jpeg_cmyk = false;              // option "jpeg_cmyk": Adobe CMYK / YCCK JPEGs decode on the GPU (to RGB)
  bool jpeg_multiscan = false;         // option "jpeg_multiscan": non-interleaved baseline JPEGs decode on the GPU
  bool resize16 = false;               // option "resize16": ... and resize to their bucket (dg_resize16.hip)
  bool penc16 = false;                 // option "penc16": ... and go into the PNG re-encoder as 16-bit samples (dg_penc16.h)
  bool penc_dynamic = false;           // option "penc_dynamic": PNG re-encode with per-image Huffman codes where shorter
  bool jenc_optimize = false;          // option "jenc_optimize": JPEG re-encode with per-image Huffman tables

  // progressive JPEGs
  int prog_lanes = 1;  // option "prog_lanes": progressive batches in flight beside the baseline ones
  bool prog_split = true;
  int prog_batch = 2048;
  int prog_flush_us = 20000;
  int prog_cus = 0;        // option "prog_cus" (prog_queue 3: CU mask width, 0 = all)
  int prog_queue = 2;      // option "prog_queue" (make_prog_streams): low priority, a queue of its own
  bool prog_side = false;  // option "prog_side": progressive scans on the side stream (measured slower: off)
  bool prog_serial = false;            // option "prog_serial": serial reader for every scan (A/B)
  bool prog_pipe = true;               // option "prog_pipe": all scans in one pipelined launch (0: one launch per level)
  int prog_chain = 100;                // option "prog_chain": chain dependency groups costing <= this % of the longest scan

  // slots, streams, host threads, device budget
  int nslots = 4;  // option "slots": batches in flight (each slot: own streams + scratch; 4 measured +2% over 3 with own queues)
  int slot_queue = 1;      // option "slot_queue" (make_streams for the baseline slots): high priority
  int side_queue = 3;      // option "side_queue": the baseline slots' side streams (-1: as slot_queue; 3: own queues)
  bool side_stream = true;
  size_t max_dev_bytes = 0;        // option "max_device_mb" (0: no budget)
  // Planned budget (option "budget_plan", default 1): the
  // first baseline batch under a budget decides the slot count and each
  // slot's buffer sizes from the budget, and every planned slot is sized
  // then; later batches that do not fit their slot are split, never grown.
  bool budget_plan = true;
  int plan_threads = 4;            // option "plan_threads"
  int meta_pull = 1;               // option "meta_pull"
  int copy_threads = 8;                // option "copy_threads": host threads for a host-out batch's output copies
  int coalesce_max = 64, coalesce_us = 500;
  // option "coalesce_inflight": coalesced batches in flight (0 = nslots); 3 fills the batches better
  // (7.6 vs 5.4 images) and measured 5-20% faster than 4 from 32 callers (profiles/r04/one_r4*)
  int coalesce_inflight = 3;

  // timing and debugging
  bool timing = false;
  bool wg_timing = false;
  int debug_flags = 0;
};

// A row's field: where it is in Options and what it holds.
enum OptType : uint8_t { kOptNone, kOptBool, kOptInt, kOptU32, kOptI64, kOptU64, kOptDouble };

// Which values a row takes.
enum OptKind : uint8_t {
  kOptFlag,      // any value: stores v != 0
  kOptFlagInv,   // any value: stores v == 0
  kOptRange,     // lo <= v <= hi (a strict flag is the range 0..1 over a bool)
  kOptRangeBut,  // ... and v != except
  kOptPow2,      // a power of two in lo..hi
  kOptPow2Or0,   // ... or 0
  kOptRaw,       // any value, cast to the field's type
  kOptSignal,    // no field: the value is ignored, the "after" step is the option
};

// What Context::set_option does around the store (pipeline.cpp).
enum OptAfter : uint8_t {
  kAfterNone,
  kAfterCoalesce,     // stored under the coalescing lock
  kAfterCoefCache,    // refused while a batch in flight uses the cache; the cache starts over
  kAfterMaxDevice,    // the budget starts over; the slots' streams move to the shared queues
  kAfterBudgetPlan,   // the planned budget starts over
  kAfterSlots,        // the slot in turn stays below the count
  kAfterProgQueue,    // the progressive slots finish, their streams are made again
  kAfterSlotQueue,    // the baseline slots finish, their streams are made again
  kAfterResetHostUs,  // the host_us_* / host_cpu_us_* stats go to zero
};

struct OptRow {
  const char *name;
  size_t off;  // the field: offset in Options, type
  OptType type;
  OptKind kind;
  int64_t lo, hi, except;
  uint8_t shift;    // the field holds v << shift (an option in MiB over a byte count)
  const char *why;  // dg_last_error's text behind "dg_ctx_set_option("key", v): " for a rejected value
  OptAfter after;
};

extern const OptRow kOptionTable[];
extern const int kNumOptions;
extern const OptRow kOptionTableAdded[];  // later rows (options.cpp says why they stand apart); find_option reads both
extern const int kNumOptionsAdded;

enum OptResult { kOptStored, kOptRejected, kOptUnknown };

const OptRow *find_option(const char *key);              // null: no such key
bool option_takes(const OptRow &r, int64_t v);           // v passes the row's check
void store_option(const OptRow &r, Options &o, int64_t v);  // ... and goes into the row's field
// The three in a row: a rejected or unknown key leaves o alone and says why
// (the rejecting condition, or "unknown option").
OptResult apply_option(Options &o, const char *key, int64_t v, std::string *why);
// dg_last_error's text for a failed dg_ctx_set_option: the option, the value
// and the accepted range (the range as the condition that rejects it).
std::string option_error_text(const char *key, int64_t v, const std::string &why);

}  // namespace dg
