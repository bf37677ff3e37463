// submit.cpp — the batch planner: Context::submit and its phases.
//
// One submit plans every image's header, pools its tables, lays every buffer
// of the batch out in the slot's arenas, fits them to the device, turns the
// offsets into addresses, builds the workgroup lists, stages descriptors and
// lists in one meta buffer and launches.  Each phase is a function of its
// own; SubmitArgs (the caller's arrays), BatchLayout (cursors and offsets),
// the Batch and the Slot are all that crosses from one phase to the next.
#include <string.h>
#include <time.h>

#include <algorithm>
#include <chrono>
#include <cmath>

#include "../dg_alph.h"
#include "../dg_entropy.h"
#include "../dg_bmp.h"
#include "../dg_gif.h"
#include "../dg_vp8.h"
#include "../dg_vp8l.h"
#include "../dg_jenc_tree.h"
#include "../dg_pixel.h"
#include "../kernels.h"
#include "pipeline_util.h"

namespace dg {

static double thread_cpu_us() {
  timespec ts;
  clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
  return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3;
}

// 64-row unfilter bands of pass p of a PNG (the image itself when not
// interlaced); k_png_unfilter numbers its progress flags the same way.
static uint32_t png_pass_bands(const ImageDesc &d, uint32_t p) {
  if (!d.png.interlace) return p == 0 ? (d.height + 63) / 64 : 0u;
  uint32_t pw, ph;
  png_adam7_pass(d.width, d.height, p, pw, ph);
  return pw && ph ? (ph + 63) / 64 : 0u;
}
static uint32_t png_bands(const ImageDesc &d) {
  uint32_t n = 0;
  for (uint32_t p = 0; p < 7; p++) n += png_pass_bands(d, p);
  return n;
}

// H pass kernel choice.  The band kernel stages the source pixels of
// kHBandCols consecutive outputs in LDS: at most 255 * scale + 2 * support
// (+ window rounding, 8-pixel alignment and ksize slack) pixels, which must
// fit kHSegPx.  Wider segments (extreme downscales) use the direct kernel;
// the first pass of a colour JPEG in the band kernel upsamples and converts
// colour in its fill.
static double h_pass_span(const ResizePass &ps) {
  const double scale = (ps.in1 - ps.in0) / (double)ps.out_size;
  const double fs = scale > 1.0 ? scale : 1.0;
  return std::ceil((kHBandCols - 1) * scale + 6.0 * fs) + 2.0 + 8.0 + (double)ps.ksize + 8.0;
}
static uint32_t h_pass_mode(const ResizePass &ps, bool colour_source) {
  if (h_pass_span(ps) > (double)kHSegPx) return kHDirect;
  return colour_source ? kHFused : 0u;
}
// k_resize_hv takes the first H and V passes of a colour JPEG together when
// its smaller segment and ring fit them and the H taps are in the <= 16 class
static bool hv_fusable(const ResizePass &h, const ResizePass &v) {
  return h.kind == 1 && (h.mode & kHFused) && !(h.mode & kHDirect) && v.kind == 2 && h.C == 3 && h.row0 == 0 &&
         v.row0 == 0 &&
         h.ksize + 1 <= 16 && v.ksize <= kHVTapsMax && h_pass_span(h) <= (double)kHVSegPx;
}

// k_band_dec takes pass[0] of a JPEG when its sampling is one the fused fill
// knows (gray; 4:4:4, 4:2:2, 4:2:0 with luma at the maximum factors) and its
// segments fit: the 128-column tile's source segment (plus the 16-pixel
// alignment) in the class's LDS, every 16-column MFMA subtile's window in the
// class's K steps (320-pixel class: one 64-wide step, downscales up to ~2x;
// 640-pixel class: two).  Returns the mode bits (0: not eligible).
static uint32_t band_dec_mode(const ImageDesc &d, const ResizePass &ps) {
  if (ps.kind != 1 || (ps.mode & (kHDirect | kHVFused)) || d.idct_fused) return 0;
  if (d.ncomp == 3) {
    if (!(ps.mode & kHFused)) return 0;
    if (d.ch[0] != d.hmax || d.cv[0] != d.vmax || d.ch[1] != d.ch[2] || d.cv[1] != d.cv[2]) return 0;
    if (d.hmax % d.ch[1] || d.vmax % d.cv[1]) return 0;
    const uint32_t hr = d.hmax / d.ch[1], vr = d.vmax / d.cv[1];
    if (hr > 2 || vr > 2 || (hr == 1 && vr == 2)) return 0;
  } else if (d.ncomp != 1) {
    return 0;
  }
  const double scale = (ps.in1 - ps.in0) / (double)ps.out_size;
  const double window = 15.0 + std::ceil(15.0 * scale) + (double)ps.ksize + 2.0;  // a subtile's K range
  const double span = h_pass_span(ps) + 16.0;
  if (span <= (double)kDecSeg0 && window <= 64.0) return kHDecode;  // one K step
  if (span <= (double)kDecSeg1 && window <= 128.0) return kHDecode | kHDecWide;
  return 0;
}

// k_resize_hm takes a band H pass when every 16-column subtile's window fits
// one or two 64-wide K steps and the 16-aligned segment fits kHSegPx: returns
// the K steps (0: the VALU band kernel runs it).
static uint32_t h_mfma_steps(const ResizePass &ps) {
  if (ps.kind != 1 || (ps.mode & (kHDirect | kHVFused | kHDecode)) || ps.C < 1 || ps.C > 4) return 0;
  if (h_pass_span(ps) + 8.0 > (double)kHSegPx) return 0;
  const double scale = (ps.in1 - ps.in0) / (double)ps.out_size;
  const double window = 15.0 + std::ceil(15.0 * scale) + (double)ps.ksize + 2.0;
  return window <= 64.0 ? 1u : (window <= 128.0 ? 2u : 0u);
}

// Row stride of the decoded image a JPEG's or PNG's first pass (or k_copy) reads:
// the RGB image or the PNG's pixels, or the luma plane of a gray JPEG.
static uint32_t decoded_stride(const ImageDesc &d) {
  return (d.fmt != kFmtJpeg || d.ncomp >= 3) ? d.pix_stride : d.cbw[0] * 8;
}

struct Layout {
  size_t off = 0;
  size_t take(size_t bytes, size_t align = 256) {
    off = align_up(off, align);
    size_t o = off;
    off += bytes;
    return o;
  }
};

// The caller's arrays of one submit.
struct SubmitArgs {
  int n;
  const uint8_t *const *h_srcs;
  const uint8_t *const *d_srcs;
  const size_t *lens;
  const int32_t *forced;
  uint8_t *const *outs;
  const uint64_t *caps;
  bool host_io;
};

// One image's buffer offsets: sizes first, pointers are patched after allocation.
struct Offs {
  size_t coef, ccnt, plane[4], pix, pass_dst[kStages], pass_coef[kStages], pass_bounds[kStages], pass_srcoff[kStages];
  int pass_cache[kStages];    // Lanczos table cache entry of the pass (-1: tables in the scratch arena)
  bool pass_hit[kStages];     // ... already computed (no k_coeffs item)
  size_t final_off, tmp, out, ds, mk, chunk, stage;
  size_t zs, raw, unf, pal;
  size_t tout, ecoef, ebits, ewords, hdr, eaux;  // JPEG / PNG re-encode
  size_t etab;  // PNG, option "penc_dynamic": bytes of histogram / code table at the head of ewords;
                // JPEG, option "jenc_optimize": bytes of histogram / EncTables / DHT segments there
  // alpha programs: buffer = dst of pass `stage` (-1: the decoded image), byte offset
  int aop_stage[kAlphaPoints];
  size_t aop_off[kAlphaPoints];
  // offsets taken from the late region (LT): bit 0 unf, 1 pix, 2 out, 3 + s pass_dst[s]
  uint32_t late = 0;
  int img = -1;
};

// The layout state of one batch: all that the planning phases hand on.
struct BatchLayout {
  Layout L;        // scratch arena
  Layout CO;       // coefficient arena (zero-filled per batch)
  Layout IN;       // input arena (host path)
  // The chunk-parallel inflate's entries (CH, 2 bytes per output byte, most
  // of a PNG batch's memory) are dead once k_inf_resolve has turned them into
  // raw bytes, before anything writes the buffers of the unfilter / expand /
  // resize stages (LT).  Both regions are laid out from 0 and placed at the
  // same offset of the scratch arena (option "png_alias", default on).
  Layout LT, CH;
  bool alias = false;
  Layout &late() { return alias ? LT : L; }    // the unfilter / expand / resize buffers
  Layout &chunks() { return alias ? CH : L; }  // the chunk-parallel inflate's entries
  std::vector<Offs> offs;       // one per planned image, in image order
  std::vector<size_t> in_off;   // per image: its coded bytes in the input arena (host path)
  uint32_t sub_bits = 0;        // the batch's subsequence size
  bool small = false;           // a latency-bound batch (option "small_coded")
  uint32_t sub_base = 0;        // SubStates so far
  uint64_t ckpt_total = 0;      // checkpoint records of the batch (per-image sub_bits)
  size_t subs_off = 0, ckpt_off = 0, idct_list_off = 0;  // SubStates, checkpoints, fused-IDCT list (scratch arena)
};

// Work items that are concatenated class by class once every image has pushed its own.
struct ClassLists {
  std::vector<WgItem> hb[2][2][4];  // band H items per (stage, fused fill, weight-count class)
  std::vector<WgItem> hvl[2];       // k_resize_hv items per H weight class
  std::vector<WgItem> decl[2];      // k_band_dec items per segment class
  std::vector<WgItem> hm[2][2][2];  // k_resize_hm items per (stage, fused fill, K steps)
};

dg_status Context::submit(int n, const uint8_t *const *h_srcs, const uint8_t *const *d_srcs, const size_t *lens,
                          const int32_t *forced, uint8_t *const *outs, const uint64_t *caps,
                          dg_payload_meta *metas, bool host_io, uint64_t *ticket, dg_payload_meta *const *mptrs,
                          int force_slot, bool defer_meta) {
  const auto wait_t0 = std::chrono::steady_clock::now();
  std::unique_lock<std::mutex> lk(mu_);
  if (n < 0 || (n > 0 && (!h_srcs || !lens || !outs || !caps || (!metas && !mptrs)))) {
    set_error("null argument");
    return DG_ERR_INVALID;
  }
  const SubmitArgs a{n, h_srcs, d_srcs, lens, forced, outs, caps, host_io};
  HIPCHK(hipSetDevice(device_));
  Slot &sl = slots_[force_slot >= 0 ? force_slot : pick_slot()];
  if (dg_status st = slot_streams(sl)) return st;
  if (dg_status st = wait_slot(sl, lk)) return st;
  // context lock + the slot's previous batch (stat "host_us_slotwait")
  host_us_[7] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - wait_t0).count();
  std::unique_ptr<Batch> bp(new Batch());
  Batch &b = *bp;
  b.ticket = next_ticket_++;
  b.fin = std::make_shared<BatchEvent>();
  HIPCHK(hipEventCreateWithFlags(&b.fin->e, hipEventDisableTiming));
  b.n = n;
  b.host_io = host_io;
  b.mptr.resize(n);
  for (int i = 0; i < n; i++) b.mptr[i] = mptrs ? mptrs[i] : &metas[i];
  if (defer_meta) {
    // A progressive aggregate's members: the callers' metas keep reading
    // DG_ERR_NOT_READY until finish() publishes the batch's own copies
    // (dg_wait_ready's contract; the GPU is still decoding while planning
    // fills in status and dimensions).
    b.pub = b.mptr;
    b.local_meta.assign(n, dg_payload_meta{});
    for (int i = 0; i < n; i++) b.mptr[i] = &b.local_meta[i];
  }
  b.plans.resize(n);
  b.desc_of.assign(n, -1);
  // host time per submit phase: wall ("host_us_<phase>") and this thread's CPU
  // time ("host_cpu_us_<phase>"); wall well above CPU = blocking (allocation,
  // copies, driver locks), not planning work
  auto phase_t0 = std::chrono::steady_clock::now();
  double cpu_t0 = thread_cpu_us();
  auto phase = [&](int k) {
    const auto now = std::chrono::steady_clock::now();
    const double c = thread_cpu_us();
    host_us_[k] += std::chrono::duration<double, std::micro>(now - phase_t0).count();
    host_cpu_us_[k] += c - cpu_t0;
    phase_t0 = now;
    cpu_t0 = c;
  };
  plan_images(a, b);
  phase(0);
  if (dg_status st = pool_tables(b)) return st;
  phase(1);
  // Lanczos table cache: entries this submit creates are dropped again if it
  // returns before its batch is installed (budget split, allocation failure)
  ccache_maybe_reset(sl);
  struct CacheRoll {
    Context *c;
    size_t n0, off0;
    bool armed = true;
    ~CacheRoll() {
      if (armed) c->ccache_rollback(n0, off0);
    }
  } croll{this, ccache_.size(), ccache_off_};
  BatchLayout bl;
  choose_sub_bits(b, bl);
  layout_images(a, b, bl);
  layout_batch_regions(b, bl);
  if (dg_status st = fit_device(sl, b, bl)) return st;
  patch_addresses(a, sl, b, bl);
  phase(2);
  build_lists(b);
  phase(3);
  if (dg_status st = stage_and_upload(a, sl, b, bl)) return st;
  phase(4);
  if (dg_status st = enqueue_upload(a, sl, b, bl)) return st;
  sl.batch = std::move(bp);
  croll.armed = false;
  phase(5);
  if (dg_status st = launch_all(sl, false)) {
    fail_batch(sl, st);
    return st;
  }
  phase(6);
  stat_batches_++;
  *ticket = sl.batch->ticket;
  if ((!opt_.max_dev_bytes || budget_planned_) && stat_batches_ <= 2 * kMaxInflight) prewarm_slots(sl);
  return DG_OK;
}

// This slot's previous batch must complete first.  Its GPU work is waited
// for without the context lock: a progressive slot's batch can run ~1 s,
// and every other dg_submit / dg_wait / dg_poll of the context would stall
// behind it.  Re-checked after relocking: another thread may
// have finished that batch, or queued one of its own on the slot.
dg_status Context::wait_slot(Slot &sl, std::unique_lock<std::mutex> &lk) {
  while (sl.batch && !sl.batch->done) {
    if (hipEventQuery(sl.batch->fin->e) == hipErrorNotReady) {
      std::shared_ptr<BatchEvent> fin = sl.batch->fin;
      lk.unlock();
      const hipError_t e = hipEventSynchronize(fin->e);
      lk.lock();
      if (e != hipSuccess) {
        set_error(std::string("HIP error: ") + hipGetErrorString(e) + " waiting for a slot's batch");
        return DG_ERR_DEVICE;
      }
      continue;
    }
    dg_status st = finish(sl);
    if (st) return st;
  }
  return DG_OK;
}

// ---- 1. plan every image (host, header only; on the planning workers)
void Context::plan_images(const SubmitArgs &a, Batch &b) {
  auto plan_one = [&](int i) {
    ImagePlan &p = b.plans[i];
    plan_image(a.h_srcs[i], a.lens[i], a.forced ? a.forced[i] : -1, p);
    dg_payload_meta &m = *b.mptr[i];
    memset(&m, 0, sizeof(m));
    m.status = p.status;
    m.bucket = p.bucket;
    if (p.fmt == kFmtJpeg && p.hdr.status == JH_OK) {
      m.original_width = p.hdr.width;
      m.original_height = p.hdr.height;
    } else if (p.fmt == kFmtPng && p.png.status == PH_OK) {
      m.original_width = p.png.width;
      m.original_height = p.png.height;
    } else if (p.fmt == kFmtGif && p.gif.status == GH_OK) {  // the logical screen
      m.original_width = p.gif.width;
      m.original_height = p.gif.height;
    } else if (p.fmt == kFmtBmp && p.bmp.status == BH_OK) {  // the file's width and |height|
      m.original_width = p.bmp.width;
      m.original_height = p.bmp.height;
    } else if (p.fmt == kFmtWebp && p.webp.status == WH_OK) {
      m.original_width = p.webp.width;
      m.original_height = p.webp.height;
    } else if (p.fmt == kFmtVp8 && p.vp8.status == WH_OK) {
      m.original_width = p.vp8.width;
      m.original_height = p.vp8.height;
    }
    m.width = p.out_w;
    m.height = p.out_h;
    m.channels = p.channels;
    m.bit_depth = p.bit_depth;
    m.is_encoded = p.encode ? 1 : 0;
    m.nbytes = p.out_bytes;
    if (p.status == DG_OK && a.caps[i] < p.out_bytes) {
      p.status = DG_ERR_SMALL_BUFFER;
      m.status = DG_ERR_SMALL_BUFFER;
    }
    if (p.status == DG_OK && !a.outs[i]) {
      p.status = DG_ERR_INVALID;
      m.status = DG_ERR_INVALID;
    }
  };
  if (opt_.plan_threads > 1 && a.n >= 2 * kPlanGrain) {
    if (!plan_pool_ || plan_pool_->threads() != opt_.plan_threads) plan_pool_.reset(new HostPool(opt_.plan_threads));
    plan_pool_->run(a.n, kPlanGrain, plan_one);
  } else {
    for (int i = 0; i < a.n; i++) plan_one(i);
  }
}

// ---- 2. table pools
dg_status Context::pool_tables(Batch &b) {
  const int n = b.n;
  size_t hneed = 0, qneed = 0;  // upper bound of the tables this batch adds
  for (int i = 0; i < n; i++) {
    const ImagePlan &p = b.plans[i];
    // (planning may run on pool threads; dg_last_error is the caller's)
    if (p.status == DG_ERR_UNSUPPORTED && p.fmt == kFmtPng && p.png.depth == 16) set_error(p.png.why);
    if (p.status && p.fmt == kFmtGif && p.gif.why[0]) set_error(p.gif.why);
    if (p.status && p.fmt == kFmtBmp && p.bmp.why[0]) set_error(p.bmp.why);
    if (p.status && p.fmt == kFmtWebp && p.webp.why[0]) set_error(p.webp.why);
    if (p.status && p.fmt == kFmtVp8 && p.vp8.why[0]) set_error(p.vp8.why);
    if (p.status || p.fmt != kFmtJpeg) continue;
    hneed += (p.hdr.progressive || p.hdr.multiscan) ? p.hdr.tables.size() : 2u * (size_t)p.hdr.ncomp;
    qneed += (size_t)p.hdr.ncomp;
  }
  if (hpool_.size() > kPoolKeep || qpool_.size() > kPoolKeep ||
      (hpool_.size() && hpool_.size() + hneed > kPoolMax) || (qpool_.size() && qpool_.size() + qneed > kPoolMax)) {
    dg_status st = flush_pools();
    if (st) return st;
  }
  for (int i = 0; i < n; i++) {
    ImagePlan &p = b.plans[i];
    if (p.status || p.fmt != kFmtJpeg) continue;
    int worst = 0;  // -1: a table that does not build (corrupt), -2: pools full for this batch
    auto use = [&](int idx) { worst = std::min(worst, idx); };
    if (p.hdr.progressive || p.hdr.multiscan) {  // the tables each scan uses
      for (const HuffSpec &t : p.hdr.tables) use(pool_huff(t));
      for (int c = 0; c < p.hdr.ncomp; c++) use(pool_quant(p.hdr.q[p.hdr.comp[c].tq]));
    } else {
      for (int c = 0; c < p.hdr.ncomp; c++) {
        use(pool_huff(p.hdr.dc[p.hdr.comp[c].td]));
        use(pool_huff(p.hdr.ac[p.hdr.comp[c].ta]));
        use(pool_quant(p.hdr.q[p.hdr.comp[c].tq]));
      }
    }
    if (worst == -2) {
      p.status = DG_ERR_UNSUPPORTED;
      b.mptr[i]->status = DG_ERR_UNSUPPORTED;
    } else if (worst < 0) {
      p.status = DG_ERR_CORRUPT;
      b.mptr[i]->status = DG_ERR_CORRUPT;
    }
  }
  dg_status st = upload_pools();
  if (st) return st;
  b.pool_gen = pool_gen_;
  b.hp = (const HuffTable *)d_hpool_[pool_gen_].p;
  b.qp = (const QuantTable *)d_qpool_[pool_gen_].p;
  return DG_OK;
}

// ---- 3. layout
// Subsequence size: the entropy kernels are latency-bound, so they want as
// many lanes as the chip can keep resident, but every subsequence costs a
// sync re-decode.  Measured on MI355X (profiles/r01/sweep_v4): 2048 bits
// below 64 MiB of coded data (configs[2]'s 1,024 WebDataset members, ~25
// MiB: 39.9 vs 38.5 Gpx/s with 4096, profiles/r04/wds_sub2); from 64 MiB
// option "sub_auto"
// (round 4: 8192, profiles/r04/ab -- the chip stays full with half the
// lanes once the write pass no longer decodes, and the 6 kbit lead-in of a
// 4:2:0 range costs 75% instead of 150% of its bits).
// Small batches (dg_decode_one's few images, option "small_coded" bytes of
// coded data) are latency-bound: a lane's chain of lead-in + range bits is
// the batch's k_huff_sync time (0.87 ms of a ~3 ms coalesced batch in the
// decode_one trace, profiles/r04/one_trace), so they take short ranges and
// lead-ins ("sub_small", "lead_small") at the cost of more total decode.
void Context::choose_sub_bits(const Batch &b, BatchLayout &bl) {
  bl.sub_bits = opt_.sub_bits;
  bl.small = false;
  if (!bl.sub_bits) {
    uint64_t coded = 0;
    for (int i = 0; i < b.n; i++)
      if (!b.plans[i].status && b.plans[i].fmt == kFmtJpeg && !b.plans[i].hdr.progressive)
        coded += b.plans[i].hdr.scan_end - b.plans[i].hdr.scan_off;
    bl.small = coded < opt_.small_coded;
    bl.sub_bits = coded >= (64ull << 20) ? opt_.sub_auto : bl.small ? opt_.sub_small : 2048u;
  }
  last_sub_bits_ = bl.sub_bits;
}

// first pass: sizes only (pointers are patched after allocation)
void Context::layout_images(const SubmitArgs &a, Batch &b, BatchLayout &bl) {
  bl.alias = opt_.png_alias;
  bl.in_off.assign(a.n, 0);
  b.out_dev_off.assign(a.n, 0);
  b.out_direct.assign(a.n, 0);
  b.descs.reserve(a.n);
  // a four-component JPEG (option "jpeg_cmyk") puts the whole batch on the entropy kernels' NC = 4
  // instantiations; the paths that keep three DC sums (sync2, entropy_once, idct_fused) stand down for it
  for (int i = 0; i < a.n; i++)
    if (!b.plans[i].status && b.plans[i].fmt == kFmtJpeg && b.plans[i].hdr.ncomp == 4) b.nc4 = true;
  // a non-interleaved baseline JPEG (option "jpeg_multiscan") puts the batch on k_huff_write's multiscan
  // instantiation; entropy_once and idct_fused stand down for it
  for (int i = 0; i < a.n; i++)
    if (!b.plans[i].status && b.plans[i].fmt == kFmtJpeg && b.plans[i].hdr.multiscan) b.ms = true;
  for (int i = 0; i < a.n; i++) {
    const ImagePlan &p = b.plans[i];
    if (p.status) continue;
    ImageDesc d;
    memset(&d, 0, sizeof(d));
    d.sample_bytes = 1;
    Offs o;
    memset(&o, 0, sizeof(o));
    o.late = 0;
    o.img = i;
    for (int s_ = 0; s_ < kStages; s_++) o.pass_cache[s_] = -1;
    if (p.fmt == kFmtPng)
      layout_png(a, i, b, bl, d, o);
    else if (p.fmt == kFmtGif)
      layout_gif(a, i, b, bl, d, o);
    else if (p.fmt == kFmtBmp)
      layout_bmp(a, i, b, bl, d, o);
    else if (p.fmt == kFmtWebp)
      layout_webp(a, i, b, bl, d, o);
    else if (p.fmt == kFmtVp8)
      layout_webp_lossy(a, i, b, bl, d, o);
    else
      layout_jpeg(a, i, b, bl, d, o);
    const int last_stage = plan_resize(p, b, bl, d, o);
    layout_output_and_encode(a, i, last_stage, b, bl, d, o);
    b.desc_of[i] = (int)b.descs.size();
    b.descs.push_back(d);
    bl.offs.push_back(o);
  }
  // the scan descriptors of multiscan images, behind every image's descriptor (image index order and
  // descriptor index order still agree for real images)
  for (int i = 0; b.ms && i < a.n; i++) {
    const ImagePlan &p = b.plans[i];
    if (p.status || p.fmt != kFmtJpeg || !p.hdr.multiscan) continue;
    for (int j = 0; j < (int)p.hdr.scans.size(); j++) layout_scan(i, j, b, bl);
  }
  // likewise the companion descriptors of VP8L-coded alpha streams (option "webp_alpha")
  for (int i = 0; b.any_alph && i < a.n; i++) {
    const ImagePlan &p = b.plans[i];
    if (!p.status && p.fmt == kFmtVp8 && b.descs[b.desc_of[i]].dec_c == 4 && alph_compression(p.vp8.alph_hdr) == kAlphVp8l)
      layout_alph_stream(i, b, bl);
  }
}

// The companion descriptor of image i's VP8L-coded alpha stream: a lossless image of the frame's size whose
// bitstream is the ALPH payload after its header byte, with a work arena and a table area of its own and no
// pixels; k_alph_plane reads the green channel of its final plane.
void Context::layout_alph_stream(int i, Batch &b, BatchLayout &bl) {
  const Vp8Header &g = b.plans[i].vp8;
  ImageDesc d;
  memset(&d, 0, sizeof(d));
  Offs o;
  memset(&o, 0, sizeof(o));
  for (int s_ = 0; s_ < kStages; s_++) o.pass_cache[s_] = -1;
  d.fmt = kFmtWebp;
  d.sample_bytes = 1;
  d.width = g.width;
  d.height = g.height;
  Vp8lDesc &vd = d.vp8l;
  vd.nbytes = g.alph_len - 1;
  vd.groups_cap = vp8l_groups_cap(g.width, g.height);
  vd.alph = 1;
  o.raw = bl.L.take((size_t)vp8l_work_words(g.width, g.height) * 4, 256);
  o.zs = bl.L.take((size_t)vd.groups_cap * kVp8lGroupWords * 4, 256);
  b.descs[b.desc_of[i]].vp8.alph_desc = (uint32_t)b.descs.size();
  b.alph_streams.push_back({(int)b.descs.size(), b.desc_of[i], i});
  b.descs.push_back(d);
  bl.offs.push_back(o);
  b.any_webp = true;
}

// The entropy-only descriptor of scan j of multiscan image i (ScanMap, dg_types.h): a stream of its own with
// its own subsequences, tables and restart interval, decoded in the scan's own block order.
void Context::layout_scan(int i, int j, Batch &b, BatchLayout &bl) {
  const JpegHeader &h = b.plans[i].hdr;
  const JpegScan &sc = h.scans[j];
  const ImageDesc &par = b.descs[b.desc_of[i]];
  ImageDesc d;
  memset(&d, 0, sizeof(d));
  Offs o;
  memset(&o, 0, sizeof(o));
  for (int s_ = 0; s_ < kStages; s_++) o.pass_cache[s_] = -1;
  d.fmt = kFmtJpeg;
  d.sample_bytes = 1;
  d.ncomp = (uint8_t)sc.ns;
  d.sem = par.sem;
  d.ckpt = opt_.ckpt ? 1u : 0u;
  d.ms = ms_scan_map(par, (uint32_t)sc.ns, sc.comp, d.total_blocks);
  uint32_t bpm = 0;
  for (int q = 0; q < sc.ns; q++) {  // the scan's components, numbered in scan order
    const int c = sc.comp[q];
    d.ch[q] = par.ch[c];
    d.cv[q] = par.cv[c];
    d.cfirst[q] = bpm;
    const uint32_t nb = sc.ns == 1 ? 1u : par.ch[c] * par.cv[c];
    for (uint32_t k = 0; k < nb; k++) d.blk_comp[bpm + k] = (uint8_t)q;
    bpm += nb;
  }
  d.bpm = bpm;
  for (uint32_t k = 0; k < bpm; k++) d.comp_bits |= (uint32_t)d.blk_comp[k] << (2 * k);
  if (sc.ns > 1) {
    d.mcux = par.mcux;
    d.mcuy = par.mcuy;
  }
  d.restart = (uint32_t)sc.restart;  // in the scan's own MCUs: blocks for a one-component scan
  d.blocks_per_seg = d.restart * bpm;
  int nslots = 0;
  auto slot_of = [&](int pidx) {
    for (int s = 0; s < nslots; s++)
      if (d.hslot[s] == pidx) return s;
    d.hslot[nslots] = (uint16_t)pidx;
    return nslots++;
  };
  uint32_t acs = 0;
  for (int q = 0; q < sc.ns; q++) {
    d.slotmap |= (uint32_t)slot_of(pool_huff(h.tables[sc.dc_tab[q]])) << ((2 * q) * 4);
    const int as = slot_of(pool_huff(h.tables[sc.ac_tabs[q]]));
    d.slotmap |= (uint32_t)as << ((2 * q + 1) * 4);
    acs |= 1u << as;
  }
  d.nslots = (uint8_t)nslots;
  b.max_slots = std::max<uint32_t>(b.max_slots, (uint32_t)nslots);
  b.max_ac = std::max<uint32_t>(b.max_ac, std::min<uint32_t>((uint32_t)__builtin_popcount(acs), kMultiLuts));
  layout_entropy_stream(sc.end - sc.off, b, bl, d, o);
  b.ms_scans.push_back({(int)b.descs.size(), b.desc_of[i], i, j});
  b.descs.push_back(d);
  bl.offs.push_back(o);
}

void Context::layout_png(const SubmitArgs &a, int i, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const PngHeader &g = b.plans[i].png;
  const uint32_t W = g.width, H = g.height, C = (uint32_t)g.out_c;
  d.fmt = kFmtPng;
  d.width = W;
  d.height = H;
  d.dec_c = (uint8_t)C;
  PngDesc &pd = d.png;
  pd.zlen = (uint32_t)g.zlen;
  pd.rowbytes = g.rowbytes;
  pd.ustride = (uint32_t)align_up(g.rowbytes, 16);
  pd.bpp = (uint32_t)g.bpp;
  pd.ctype = (uint32_t)g.ctype;
  pd.depth = (uint32_t)g.depth;
  pd.has_trns = (uint32_t)g.has_trns;
  for (int k = 0; k < 3; k++) pd.trns[k] = g.trns[k];
  pd.interlace = (uint32_t)g.interlace;
  pd.rawlen = (uint32_t)g.rawlen;
  pd.expand = g.ctype == 3 || g.depth < 8 || g.has_trns || g.interlace;  // k_png_expand also de-interlaces
  const bool deep = g.depth == 16;  // always through k_png_expand16 (byte order)
  if (deep) pd.expand = 1;
  if (deep) d.sample_bytes = 2;
  o.zs = bl.L.take((size_t)g.zlen + 64, 256);
  // chunk-parallel inflate for streams of at least two chunks (small ones,
  // e.g. masks, inflate serially in one wave)
  {
    const uint64_t want = g.rawlen;
    const uint32_t span = opt_.inf_chunk;
    const uint32_t nch = (uint32_t)((g.zlen + span - 1) / span);
    if (nch >= 2 && !opt_.chunked_off) {
      pd.chunk0 = (uint32_t)b.ichunks.size();
      pd.nchunks = nch;
      // entries per chunk: inf_cap / 10 times the image's average expansion of a span (+64 Ki), at
      // most the whole image; a chunk that needs more sends the image to the serial kernel.  The
      // entries (2 bytes per output byte) are most of a PNG batch's device memory: 3x made them
      // 6x the raw image
      const double ratio = (double)want / (double)g.zlen;
      const uint64_t cap = std::min<uint64_t>(want, (uint64_t)(0.1 * opt_.inf_cap * ratio * span) + opt_.inf_pad);
      for (uint32_t k = 0; k < nch; k++) {
        InfChunk c;
        memset(&c, 0, sizeof(c));
        c.image = (uint32_t)b.descs.size();
        c.idx = k;
        c.span = span;
        c.cap = (uint32_t)cap;
        c.start = k == 0 ? 16u : kInfNone;  // chunk 0: first block after the 2-byte zlib header
        c.out = bl.chunks().take(cap * 2, 256);  // offsets: made absolute below
        c.tab = bl.chunks().take(kInfTabBytes, 256);
        b.ichunks.push_back(c);
      }
    }
  }
  o.raw = bl.L.take((size_t)g.rawlen + 16, 256);
  o.unf = bl.late().take(g.interlace ? (size_t)g.unflen + 16 : (size_t)H * pd.ustride, 256);
  o.late |= bl.alias ? 1u : 0u;
  if (deep) {  // k_png_expand16 writes whole pixel pairs: C dwords each
    d.pix_stride = (uint32_t)align_up((size_t)((W + 1) / 2) * 4 * C, 16);
    o.pix = bl.late().take((size_t)d.pix_stride * H);
    o.late |= bl.alias ? 2u : 0u;
  } else if (pd.expand) {
    d.pix_stride = (uint32_t)align_up((size_t)W * C, 16);
    o.pix = bl.late().take((size_t)d.pix_stride * H);
    o.late |= bl.alias ? 2u : 0u;
  } else {
    d.pix_stride = pd.ustride;
  }
  if (g.ctype == 3) {
    o.pal = b.blob.size();
    b.blob.insert(b.blob.end(), &g.pal[0][0], &g.pal[0][0] + 1024);
  }
  if (a.host_io) bl.in_off[i] = bl.IN.take(a.lens[i] + 16, 16);
  b.any_png = true;
}

// A GIF (option "gif"): the code stream (gathered only when the sub-block chain is not 255, .., 255, last),
// the frame's index plane and the Rgba8 screen, which then is what an RGBA8 PNG's pixels are.
void Context::layout_gif(const SubmitArgs &a, int i, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const GifHeader &g = b.plans[i].gif;
  d.fmt = kFmtGif;
  d.width = g.width;
  d.height = g.height;
  d.dec_c = 4;
  GifDesc &gd = d.gif;
  gd.nbytes = (uint32_t)g.nbytes;
  gd.blocked = g.closed ? 1u : 0u;
  gd.mcs = (uint32_t)g.min_code_size;
  gd.npal = (uint32_t)g.npal;
  gd.left = g.left;
  gd.top = g.top;
  gd.fw = g.fw;
  gd.fh = g.fh;
  gd.interlace = (uint32_t)g.interlace;
  if (!g.closed) o.zs = bl.L.take((size_t)g.nbytes + 64, 256);
  o.raw = bl.L.take((size_t)g.fw * g.fh + 64, 256);
  d.pix_stride = (uint32_t)align_up((size_t)g.width * 4, 16);
  o.pix = bl.late().take((size_t)d.pix_stride * g.height);
  o.late |= bl.alias ? 2u : 0u;
  while (b.blob.size() % 4) b.blob.push_back(0);  // k_gif_expand loads whole entries
  o.pal = b.blob.size();
  b.blob.insert(b.blob.end(), &g.pal[0][0], &g.pal[0][0] + 1024);
  if (a.host_io) bl.in_off[i] = bl.IN.take(a.lens[i] + 16, 16);
  b.any_gif = true;
}

// A BMP (option "bmp"): the pixel array or the RLE stream is read in place; an RLE file's index plane and
// the Rgb8 / Rgba8 pixels, which then are what an 8-bit PNG's pixels are.
void Context::layout_bmp(const SubmitArgs &a, int i, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const BmpHeader &g = b.plans[i].bmp;
  d.fmt = kFmtBmp;
  d.width = g.width;
  d.height = g.height;
  d.dec_c = (uint32_t)g.out_c;
  BmpDesc &bd = d.bmp;
  bd.bits = (uint32_t)g.bits;
  bd.rle = g.compression == BMP_RLE8 ? 1u : g.compression == BMP_RLE4 ? 2u : 0u;
  bd.stride = g.stride;
  bd.top_down = (uint32_t)g.top_down;
  bd.npal = (uint32_t)g.npal;
  bd.pos = (uint32_t)g.pos[0] | ((uint32_t)g.pos[1] << 8) | ((uint32_t)g.pos[2] << 16) | ((g.pos[3] < 0 ? 4u : (uint32_t)g.pos[3]) << 24);
  bd.data_len = (uint32_t)g.data_len;
  if (bd.rle) o.raw = bl.L.take((size_t)g.width * g.height + 64, 256);
  d.pix_stride = (uint32_t)align_up((size_t)g.width * d.dec_c, 16);
  o.pix = bl.late().take((size_t)d.pix_stride * g.height);
  o.late |= bl.alias ? 2u : 0u;
  if (g.bits <= 8) {
    while (b.blob.size() % 4) b.blob.push_back(0);  // k_bmp_expand loads whole entries
    o.pal = b.blob.size();
    b.blob.insert(b.blob.end(), &g.pal[0][0], &g.pal[0][0] + 1024);
  }
  if (a.host_io) bl.in_off[i] = bl.IN.take(a.lens[i] + 16, 16);
  b.any_bmp = true;
}

// A lossless WebP (option "webp"), sized from the header alone: the coded bytes are read in place; the work
// arena (two ARGB planes, three sub-image planes of at most ceil(w/4) x ceil(h/4), the colour table), the
// prefix-code table area and the Rgb8 / Rgba8 pixels, which then are what an 8-bit PNG's pixels are.
void Context::layout_webp(const SubmitArgs &a, int i, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const WebpHeader &g = b.plans[i].webp;
  d.fmt = kFmtWebp;
  d.width = g.width;
  d.height = g.height;
  d.dec_c = g.alpha ? 4 : 3;
  Vp8lDesc &vd = d.vp8l;
  vd.nbytes = (uint32_t)g.nbytes;
  vd.groups_cap = vp8l_groups_cap(g.width, g.height);
  o.raw = bl.L.take((size_t)vp8l_work_words(g.width, g.height) * 4, 256);
  o.zs = bl.L.take((size_t)vd.groups_cap * kVp8lGroupWords * 4, 256);
  d.pix_stride = (uint32_t)align_up((size_t)g.width * d.dec_c, 16);
  o.pix = bl.late().take((size_t)d.pix_stride * g.height);
  o.late |= bl.alias ? 2u : 0u;
  if (a.host_io) bl.in_off[i] = bl.IN.take(a.lens[i] + 16, 16);
  b.any_webp = true;
}

// A lossy WebP (option "webp_lossy"), sized from width and height alone: the VP8 chunk is read in place; the
// work arena (layout_vp8: per-MB records, coefficients, Y / U / V planes padded to whole MBs, probabilities)
// and the Rgb8 pixels, which then are what an 8-bit RGB PNG's pixels are.
void Context::layout_webp_lossy(const SubmitArgs &a, int i, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const Vp8Header &g = b.plans[i].vp8;
  d.fmt = kFmtVp8;
  d.width = g.width;
  d.height = g.height;
  d.dec_c = (opt_.webp_alpha && g.has_alph) ? 4 : 3;
  d.vp8.nbytes = g.chunk_len;
  d.vp8.part0 = g.part0;
  o.raw = bl.L.take((size_t)layout_vp8(g.width, g.height).bytes, 256);
  if (d.dec_c == 4) {  // option "webp_alpha": the unfiltered plane, a whole number of dwords (k_alph_plane reads it back by dwords)
    d.vp8.alph_filter = alph_filter(g.alph_hdr);
    o.zs = bl.L.take(align_up((size_t)g.width * g.height, 4), 256);
    b.any_alph = true;
  }
  d.pix_stride = (uint32_t)align_up((size_t)g.width * d.dec_c, 16);
  o.pix = bl.late().take((size_t)d.pix_stride * g.height);
  o.late |= bl.alias ? 2u : 0u;
  if (a.host_io) bl.in_off[i] = bl.IN.take(a.lens[i] + 16, 16);
  b.any_vp8 = true;
}

void Context::layout_jpeg(const SubmitArgs &a, int i, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const JpegHeader &h = b.plans[i].hdr;
  const uint32_t W = h.width, H = h.height;
  d.width = W;
  d.height = H;
  d.ncomp = (uint8_t)h.ncomp;
  d.colorspace = (uint8_t)h.colorspace;
  d.sem = (uint16_t)opt_.decode_sem;
  d.ckpt = opt_.ckpt ? 1u : 0u;
  d.dec_c = h.ncomp == 1 ? 1 : 3;
  d.hmax = (uint32_t)h.hmax;
  d.vmax = (uint32_t)h.vmax;
  d.mcux = (W + 8 * d.hmax - 1) / (8 * d.hmax);
  d.mcuy = (H + 8 * d.vmax - 1) / (8 * d.vmax);
  uint32_t bpm = 0;
  for (int c = 0; c < h.ncomp; c++) {
    const JpegComponent &k = h.comp[c];
    d.ch[c] = (uint32_t)k.h;
    d.cv[c] = (uint32_t)k.v;
    d.cdsw[c] = (uint32_t)(((uint64_t)W * k.h + d.hmax - 1) / d.hmax);
    d.cdsh[c] = (uint32_t)(((uint64_t)H * k.v + d.vmax - 1) / d.vmax);
    if (h.ncomp == 1) {
      d.cbw[c] = (d.cdsw[c] + 7) / 8;
      d.cbh[c] = (d.cdsh[c] + 7) / 8;
      d.cfirst[c] = 0;
      d.blk_comp[0] = 0;
      bpm = 1;
    } else {
      d.cbw[c] = d.mcux * k.h;
      d.cbh[c] = d.mcuy * k.v;
      d.cfirst[c] = bpm;
      for (int j = 0; j < k.h * k.v; j++) d.blk_comp[bpm + j] = (uint8_t)c;
      bpm += (uint32_t)(k.h * k.v);
    }
  }
  d.bpm = bpm;
  d.comp_bits = 0;
  for (uint32_t k = 0; k < bpm; k++) d.comp_bits |= (uint32_t)d.blk_comp[k] << (2 * k);
  d.total_blocks = h.ncomp == 1 ? d.cbw[0] * d.cbh[0] : d.mcux * d.mcuy * bpm;
  d.restart = (uint32_t)h.restart;
  d.blocks_per_seg = d.restart * bpm;
  // Huffman slots: unique pool indices per image
  int nslots = 0;
  auto slot_of = [&](int pidx) {
    for (int s = 0; s < nslots; s++)
      if (d.hslot[s] == pidx) return s;
    d.hslot[nslots] = (uint16_t)pidx;
    return nslots++;
  };
  d.slotmap = 0;
  for (int c = 0; c < h.ncomp; c++) {
    if (!h.progressive && !h.multiscan) {  // (a multiscan image's scan descriptors hold its tables)
      d.slotmap |= (uint32_t)slot_of(pool_huff(h.dc[h.comp[c].td])) << ((2 * c) * 4);
      d.slotmap |= (uint32_t)slot_of(pool_huff(h.ac[h.comp[c].ta])) << ((2 * c + 1) * 4);
    }
    d.qpool[c] = (uint16_t)pool_quant(h.q[h.comp[c].tq]);
  }
  d.nslots = (uint8_t)nslots;
  b.max_slots = std::max<uint32_t>(b.max_slots, (uint32_t)nslots);
  // distinct AC slots (k_huff_sync builds a multi-symbol lookup for each, up to 3)
  if (!h.progressive && !h.multiscan) {
    uint32_t acs = 0;
    for (int c = 0; c < h.ncomp; c++) acs |= 1u << ((d.slotmap >> ((2 * c + 1) * 4)) & 15u);
    b.max_ac = std::max<uint32_t>(b.max_ac, std::min<uint32_t>((uint32_t)__builtin_popcount(acs), kMultiLuts));
  }
  if (h.progressive) {  // scans decoded by k_prog_scan (records built once the source address is known)
    d.prog = (uint32_t)h.scans.size();
    if (a.host_io) bl.in_off[i] = bl.IN.take(a.lens[i] + 16, 16);
  } else if (h.multiscan) {  // the parent of its scans' descriptors (layout_scan): no entropy stream of its own
    d.ms.role = kMsParent;
    if (a.host_io) bl.in_off[i] = bl.IN.take(a.lens[i] + 16, 16);
  } else {
    layout_entropy(a, i, b, bl, d, o);
  }
  // buffers
  o.coef = bl.CO.take((size_t)d.total_blocks * 128);
  // sparse blocks: k_huff_write's cooperative flush + k_idct_t only (not the
  // fused / decode-once writers, k_idct or k_band_dec; progressive scans
  // write whole blocks)
  o.ccnt = (opt_.sparse_coef && opt_.idct_thread && !d.prog && !d.idct_fused && !(opt_.entropy_once && !b.nc4 && !b.ms))
               ? bl.CO.take((size_t)d.total_blocks, 64) + 1
               : 0;
  for (int c = 0; c < 4; c++) o.plane[c] = (size_t)-1;  // allocated after the pass plan (not for k_band_dec)
  // (the RGB image of a colour JPEG is only materialised if no pass fuses it)
  if (h.ncomp >= 3) d.pix_stride = (uint32_t)align_up((size_t)W * 3, 16);
}

// The entropy data of a baseline (sequential) JPEG: subsequences, checkpoints, destuff buffers.
void Context::layout_entropy(const SubmitArgs &a, int i, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const JpegHeader &h = b.plans[i].hdr;
  layout_entropy_stream(h.scan_end - h.scan_off, b, bl, d, o);
  if (a.host_io) bl.in_off[i] = bl.IN.take(a.lens[i] + 16, 16);
}

// ... of one entropy stream of scan_len bytes: an image's single scan, or a scan descriptor's (layout_scan)
void Context::layout_entropy_stream(size_t scan_len, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const uint32_t sub_bits = bl.sub_bits;
  // (a batch with a four-component or a multiscan image: the default write pass)
  const bool once = opt_.entropy_once && !b.nc4 && !b.ms;
  d.scan_len = (uint32_t)scan_len;
  // Per-image subsequence size (option "sub_density" T > 0): a lane's
  // decode time follows its symbols and blocks, not its bits, so images
  // with few coded bits per block (flat, low quality: short EOB-heavy
  // codes, ~2x the symbols per bit) take shorter ranges -- half below T
  // bits per block, a quarter below T / 2 -- and their workgroups stop
  // forming the entropy kernels' tail.
  d.sub_bits = sub_bits;
  if (opt_.sub_density > 0 && opt_.sub_bits == 0) {
    const double bpb = (double)d.scan_len * 8.0 / (double)std::max<uint32_t>(1, d.total_blocks);
    if (bpb < opt_.sub_density * 0.5 && sub_bits >= 2048)
      d.sub_bits = sub_bits / 4;
    else if (bpb < opt_.sub_density && sub_bits >= 1024)
      d.sub_bits = sub_bits / 2;
  }
  // completed blocks go straight to plane pixels inside k_huff_write (not
  // with decode-once staging, whose k_huff_scatter writes coefficients)
  d.idct_fused = (opt_.idct_fused && !once && !b.nc4 && !b.ms) ? 1u : 0u;
  // k_huff_write splits each range at the sync pass's half-way checkpoint
  // (option "write_split"): needs that checkpoint, no restart markers and
  // the plain write path
  if (opt_.write_split && d.ckpt && !d.idct_fused && !once && d.restart == 0 && d.sub_bits >= 1024 &&
      d.sub_bits / 2 / kCkptBits - 1 < num_ckpt(d.sub_bits))
    d.ckpt |= 2u;
  if (d.idct_fused) b.any_fused = true;
  // lead-in before each subsequence (lead_in in dg_entropy.h): covers the
  // self-synchronisation distance, which is longest for 6-block MCUs
  // (4:2:0; p99.9 ~7 kbit on the bench corpus, tools/sync_stats.cpp).
  // Option "lead_big" (4096): shorter than that tail, but a wrong entry
  // guess only costs a re-decode up to the first checkpoint where it merges
  // (6144 -> 4096: +1.3% on configs[1]; 2048 / 1024 slower on configs[2])
  d.lead_bits = opt_.lead_bits >= 0 ? (uint32_t)opt_.lead_bits : bl.small ? opt_.lead_small : (d.bpm >= 4 ? opt_.lead_big : 2048u);
  // shorter ranges of symbol-dense images get a proportionally shorter lead-in (option
  // "lead_density"): their codes are short, so the decoder self-synchronises in fewer bits
  if (opt_.lead_density && opt_.lead_bits < 0 && d.sub_bits < sub_bits)
    d.lead_bits = std::max<uint32_t>(1024u, d.lead_bits / (sub_bits / d.sub_bits));
  d.nsub = std::max<uint32_t>(1, (uint32_t)(((uint64_t)d.scan_len * 8 + d.sub_bits - 1) / d.sub_bits));
  d.sub_base = bl.sub_base;
  bl.sub_base += d.nsub;
  d.ckpt_base = (uint32_t)bl.ckpt_total;
  bl.ckpt_total += (uint64_t)d.nsub * num_ckpt(d.sub_bits);
  d.nchunk = std::max<uint32_t>(1, (d.scan_len + kDestuffChunk - 1) / kDestuffChunk);
  const uint32_t mcus = d.total_blocks / d.bpm;
  d.mk_cap = (d.restart ? mcus / d.restart + 2 : 0) + 64;
  d.ds_lsw = 0;
  while ((32u << d.ds_lsw) < d.sub_bits) d.ds_lsw++;
  o.ds = bl.L.take((size_t)ds_words_alloc(d.nsub, d.ds_lsw) * 4, 256);
  if (once && d.sub_bits <= 8192) {  // decode-once staging (dg_entropy.h StageCtx)
    d.stage_cap = (d.sub_bits / 2 + d.sub_bits / 8 + 64 + 3) / 4;
    o.stage = bl.L.take((size_t)((d.nsub + 63) / 64) * d.stage_cap * 64 * 16, 256);
    b.stage_on = true;
  }
  o.mk = bl.L.take((size_t)d.mk_cap * 4, 16);
  o.chunk = bl.L.take((size_t)d.nchunk * 16, 16);
}

// The pass plan (image_processing.rs:264-325), the alpha programs around it and the JPEG
// planes it leaves needed.  Returns the last pass's stage (-1: no pass).
//
// Passes (fast_image_resize semantics, B1): call 1 resizes W x H to the
// scaled nw x nh, call 2 crops the bucket out of it with a possibly
// fractional (x.5) offset.  An integral crop offset on an axis is only a
// window of call 1's outputs on that axis, so call 1's pass computes just
// that window (out0 / width) and call 2 needs no pass there; a fractional
// offset keeps call 2's sub-pixel pass.  Without a call-1 pass on an axis
// the window is a plain offset into the current image.
int Context::plan_resize(const ImagePlan &p, Batch &b, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const uint32_t W = d.width, H = d.height, C = d.dec_c;
  const bool colour = p.fmt == kFmtJpeg && d.ncomp == 3;  // the source is the YCbCr planes of a colour JPEG
  size_t cur_stride = decoded_stride(d);
  d.out_w = p.out_w;
  d.out_h = p.out_h;
  d.out_c = p.out_c;
  d.out_stride = p.out_w * p.out_c * (p.bit_depth == 16 ? 2 : 1);
  if (p.r16) return plan_resize16(p, bl, d, o);  // 16-bit PNG (option "resize16"): the image crate's f32 passes
  uint32_t cw = W, chh = H;     // extent of the current image's valid window
  uint32_t xoff = 0, yoff = 0;  // window origin (pixels, rows) inside the current buffer
  int last_stage = -1;
  auto add_pass = [&](int stage, uint32_t kind, double in0, double in1, uint32_t in_size, uint32_t out_size,
                      uint32_t out0, uint32_t width, uint32_t rows, uint32_t row0) -> ResizePass & {
    ResizePass &ps = d.pass[stage];
    ps.kind = kind;
    ps.in0 = in0;
    ps.in1 = in1;
    ps.in_size = in_size;
    ps.out_size = out_size;
    ps.out0 = out0;
    ps.ksize = fir_ksize(in0, in1, out_size);
    ps.src_stride = (uint32_t)cur_stride;
    ps.width = width;
    ps.rows = rows;
    ps.row0 = row0;
    ps.bands = opt_.hb_bands;
    ps.C = C;
    ps.dst_stride = (uint32_t)align_up((size_t)width * C, 16);
    o.pass_srcoff[stage] = (size_t)xoff * C;  // column window of the source (V passes)
    o.pass_dst[stage] = bl.late().take((size_t)ps.dst_stride * ps.rows);
    o.late |= bl.alias ? 8u << stage : 0u;
    o.pass_cache[stage] = ccache_lookup(ps, b, o.pass_hit[stage]);
    if (o.pass_cache[stage] < 0) {
      o.pass_coef[stage] = bl.L.take((size_t)out_size * ps.ksize * 2);
      o.pass_bounds[stage] = bl.L.take((size_t)out_size * 8);
    }
    cur_stride = ps.dst_stride;
    last_stage = stage;
    return ps;
  };
  if (has_cfg_ && !(W == p.out_w && H == p.out_h)) {
    uint32_t nw, nh;
    scaled_size(W, H, p.out_w, p.out_h, nw, nh);
    double l, t, bw, bh;
    fit_crop_box(nw, nh, p.out_w, p.out_h, l, t, bw, bh);
    // A window is exact for a scale-1 crop at an integral offset.  The crop box
    // comes out of f64 arithmetic (640x480 -> top 6.000000000000028, height
    // 431.99999999999994): deviations this small leave the i16 Lanczos
    // weights exactly one-hot (they are < 2^-15 off), so the sub-pixel pass
    // would copy pixel rint(offset) + i and the window is still bit-exact.
    auto near_int = [](double v, double tgt) { return std::fabs(v - tgt) <= 1e-6; };
    const bool fold_x = near_int(l, std::rint(l)) && near_int(bw, (double)p.out_w);
    const bool fold_y = near_int(t, std::rint(t)) && near_int(bh, (double)p.out_h);
    const uint32_t lx = fold_x ? (uint32_t)std::rint(l) : 0u, ty = fold_y ? (uint32_t)std::rint(t) : 0u;
    if (nw != W) {  // call 1, horizontal
      ResizePass &ps = add_pass(0, 1, 0.0, (double)W, W, nw, fold_x ? lx : 0u, fold_x ? p.out_w : nw, chh, 0);
      ps.mode = h_pass_mode(ps, colour);
      cw = ps.width;
    } else if (fold_x) {
      xoff = lx;
      cw = p.out_w;
    }
    if (nh != H) {  // call 1, vertical (reads the column window, absorbs xoff)
      ResizePass &ps = add_pass(1, 2, 0.0, (double)H, H, nh, fold_y ? ty : 0u, cw, fold_y ? p.out_h : nh, 0);
      chh = ps.rows;
      xoff = 0;
    } else if (fold_y) {
      yoff = ty;
      chh = p.out_h;
    }
    if (!fold_x) {  // call 2, horizontal sub-pixel crop (reads the row window, absorbs yoff)
      ResizePass &ps = add_pass(2, 1, l, l + bw, cw, p.out_w, 0, p.out_w, chh, yoff);
      ps.mode = h_pass_mode(ps, false);
      cw = p.out_w;
      yoff = 0;
    }
    if (!fold_y) {  // call 2, vertical sub-pixel crop (reads the column window, absorbs xoff)
      add_pass(3, 2, t, t + bh, chh, p.out_h, 0, cw, p.out_h, 0);
      chh = p.out_h;
      xoff = 0;
    }
    // U8x2 / U8x4: fast_image_resize multiplies colour by alpha before each
    // convolution call and divides after (mul_div_alpha); a call
    // whose crop box has the destination's size at integral offsets is a
    // copy and touches no alpha.  Programs run in place at three points.
    if (C == 2 || C == 4) {
      const bool call1 = !(nw == W && nh == H);
      const bool call2 = !(bw == (double)p.out_w && bh == (double)p.out_h && l == std::floor(l) &&
                           t == std::floor(t));
      const bool call2_passes = d.pass[2].kind || d.pass[3].kind;
      const int s1 = d.pass[1].kind ? 1 : 0;  // last call-1 pass (when call1)
      auto set = [&](int k, int stage, uint32_t w, uint32_t rows, uint32_t prog) {
        if (!prog) return;
        o.aop_stage[k] = stage;
        d.aop[k].width = w;
        d.aop[k].rows = rows;
        d.aop[k].prog = prog;
        b.any_alpha = true;
      };
      set(0, -1, W, H, call1 ? 1u : 0u);
      uint32_t prog1 = 0, sh = 0;
      auto push = [&](uint32_t op) {
        prog1 |= op << sh;
        sh += 2;
      };
      if (call1) push(2);
      if (call2) push(1);
      if (call2 && !call2_passes) push(2);
      if (call1)
        set(1, s1, d.pass[s1].width, d.pass[s1].rows, prog1);
      else
        set(1, -1, W, H, prog1);
      if (call2 && call2_passes) set(2, d.pass[3].kind ? 3 : 2, p.out_w, p.out_h, 2u);
    }
  }
  // colour images whose first pass is not a fused H pass need the RGB image
  d.color_fused = colour && d.pass[0].kind == 1 && (d.pass[0].mode & kHFused);
  if (opt_.hv_fused && hv_fusable(d.pass[0], d.pass[1])) d.pass[0].mode |= kHVFused;
  if (p.fmt == kFmtJpeg) {
    // k_band_dec decodes pass[0]'s source from the coefficients: no planes
    const uint32_t dm = opt_.band_dec ? band_dec_mode(d, d.pass[0]) : 0u;
    d.pass[0].mode |= dm;
    if (dm) stat_band_dec_++;
    if (!dm)
      for (uint32_t c = 0; c < d.ncomp; c++) {
        // half-rate chroma as 8-byte records (dg_plane.h, option "chroma_rec"): twice the bytes
        const bool rec = opt_.chroma_rec && d.ncomp == 3 && d.hmax == 2 * d.ch[c];
        if (rec) d.crec |= 1u << c;
        o.plane[c] = bl.L.take((size_t)d.cbw[c] * 8 * d.cbh[c] * 8 * (rec ? 2 : 1));
      }
  }
  // (a CMYK / YCCK image is never fused: k_cmyk always writes its RGB image)
  if ((colour && !d.color_fused) || (p.fmt == kFmtJpeg && d.ncomp == 4)) o.pix = bl.L.take((size_t)d.pix_stride * H);
  o.final_off = (size_t)yoff * cur_stride + (size_t)xoff * C;  // an uncomputed integral crop (k_copy's source)
  return last_stage;
}

// The passes of a 16-bit PNG that is not its bucket's size (dg_resize16.h):
// pass[0] = the vertical pass into the f32 intermediate, pass[1] = the
// horizontal pass; the integer centre crop folds into both (out0, and the
// sample window [r16_s0, + r16_ns) of the intermediate's rows).  The tap
// tables sit in the early region (k_r16_taps runs beside the inflate), the
// intermediate in the late one.  No alpha programs: the crate's resize does
// not premultiply.  Returns the last pass's stage (-1: a pure crop).
int Context::plan_resize16(const ImagePlan &p, BatchLayout &bl, ImageDesc &d, Offs &o) {
  const uint32_t W = d.width, H = d.height, C = d.dec_c;
  const R16Geom &g = p.r16g;
  if (!p.r16_passes) {  // the intermediate is the source: k_copy reads the centre window
    o.final_off = (size_t)g.y0 * d.pix_stride + (size_t)g.x0 * C * 2;
    return -1;
  }
  auto tables = [&](int stage, uint32_t entries, uint32_t ksize) {
    o.pass_coef[stage] = bl.L.take((size_t)entries * ksize * 4);
    o.pass_bounds[stage] = bl.L.take((size_t)entries * 8);
  };
  ResizePass &v = d.pass[0];
  v.kind = kR16V;
  v.in_size = H;
  v.out_size = g.h2;
  v.out0 = g.y0;
  v.ksize = p.r16_kv;
  v.src_stride = d.pix_stride;
  v.dst_stride = p.r16_ns * 4;  // whole 16-byte units (r16_ns is a multiple of 4)
  v.width = p.r16_ns;           // samples per intermediate row
  v.rows = p.out_h;
  v.row0 = p.r16_s0;
  v.C = C;
  o.pass_srcoff[0] = (size_t)p.r16_s0 * 2;
  o.pass_dst[0] = bl.late().take((size_t)v.dst_stride * v.rows);
  o.late |= bl.alias ? 8u : 0u;
  tables(0, v.rows, v.ksize);
  ResizePass &h = d.pass[1];
  h.kind = kR16H;
  h.in_size = W;
  h.out_size = g.w2;
  h.out0 = g.x0;
  h.ksize = p.r16_kh;
  h.src_stride = v.dst_stride;
  h.dst_stride = (uint32_t)align_up((size_t)p.out_w * C * 2, 16);
  h.width = p.out_w;
  h.rows = p.out_h;
  h.row0 = p.r16_s0;  // the intermediate's first sample (of a decoded row)
  h.C = C;
  if (p.bit_depth == 16) {
    o.pass_dst[1] = (size_t)-1;  // straight into the output (layout_output_and_encode)
  } else {                       // image_to_rgb8: k_copy mode 6 reads the resized samples
    o.pass_dst[1] = bl.late().take((size_t)h.dst_stride * h.rows);
    o.late |= bl.alias ? 16u : 0u;
  }
  tables(1, h.width, h.ksize);
  return 1;
}

void Context::layout_output_and_encode(const SubmitArgs &a, int i, int last_stage, Batch &b, BatchLayout &bl,
                                       ImageDesc &d, Offs &o) {
  const ImagePlan &p = b.plans[i];
  const uint32_t W = d.width, H = d.height, C = d.dec_c;
  // final write: the last pass writes straight into the output when the
  // channel count is unchanged; otherwise (or with no pass) k_copy runs.
  // (16-bit samples under image_to_rgb8 always go through k_copy's 16-to-8 conversion)
  if (last_stage >= 0 && d.out_c == C && !(d.sample_bytes == 2 && p.bit_depth != 16)) {
    d.pass[last_stage].dst_stride = d.out_stride;
    o.pass_dst[last_stage] = (size_t)-1;  // -> out
    d.copy_needed = 0;
  } else {
    d.copy_needed = 1;
    d.final_src_c = C;
    d.final_src_stride = last_stage >= 0 ? d.pass[last_stage].dst_stride : decoded_stride(d);
    if (d.sample_bytes == 2)  // 16-bit PNG (a bucket's size, a pure crop or the resized samples): u16 copy, or to_rgb8
      d.copy_mode = p.bit_depth == 16 ? 5 : 6;
    else if (d.out_c == C)
      d.copy_mode = 0;
    else if (C == 1)
      d.copy_mode = 1;  // L8 -> RGB8
    else if (C == 4)
      d.copy_mode = 2;  // RGBA8 -> RGB8 over gray
    else  // LA8 -> RGB8: resized images went through image_to_dyn_image's GrayImage (B3)
      d.copy_mode = (has_cfg_ && !(W == p.out_w && H == p.out_h)) ? 3 : 4;
  }
  if (a.host_io) {
    o.out = bl.late().take(p.out_bytes, 16);
    o.late |= bl.alias ? 4u : 0u;
    b.out_dev_off[i] = o.out;
  }
  if (p.encode && p.enc_png) {  // PNG re-encode (dg_penc.hip): the transform lands in tout
    EncDesc &e = d.enc;
    e.active = 1;
    e.png = 1;
    e.w = p.out_w;
    e.h = p.out_h;
    // 16-bit samples (option "penc16"): C is bytes per pixel, the filter rows go to k_penc_filter16, and the
    // transform's three endings (k_copy mode 5, the pure-crop window, the horizontal resize pass) write tout
    // with the tight stride out_w * out_c * 2
    const uint32_t sb = p.bit_depth == 16 ? 2 : 1;
    e.C = (p.enc_la_gray ? 1 : p.out_c) * sb;
    e.src_stride = p.enc_la_gray ? p.out_w : d.out_stride;
    const uint64_t nf = (uint64_t)e.h * ((uint64_t)e.w * e.C + 1);
    e.nblocks = (uint32_t)((nf + 1023) / 1024);
    const std::vector<uint8_t> hdr = png_enc_header(e.w, e.h, e.C / sb, sb);
    e.hdr_len = (uint32_t)hdr.size();
    o.hdr = b.blob.size();
    b.blob.insert(b.blob.end(), hdr.begin(), hdr.end());
    o.tout = bl.L.take(p.img_bytes + 16, 256);
    o.ecoef = bl.L.take((size_t)nf + 16, 256);
    o.ebits = bl.L.take((size_t)e.nblocks * 4, 256);
    o.eaux = bl.L.take((size_t)e.nblocks * 8, 256);
    o.ewords = (size_t)((3 + 9 * nf + 7 + 64) / 8 + 64) / 4 * 4;  // size for now; placed with the batch's regions
    e.hdr_bits = 3;  // the fixed block, unless k_penc_tree chooses the dynamic one (never longer: same buffer)
    e.eob_len = 7;
    e.dyn = 0;
    // option "penc_dynamic": the image's histogram / code table (dg_penc_tree.h) in front of its bit buffer,
    // inside the region the batch zeroes
    o.etab = opt_.penc_dynamic ? kPencTabBytes : 0;
    o.ewords += o.etab;
    b.penc_dyn = b.penc_dyn || opt_.penc_dynamic;
    b.any_enc = true;
  } else if (p.encode) {  // the transform lands in tout; the JPEG goes to the caller's buffer
    EncDesc &e = d.enc;
    e.active = 1;
    e.w = p.out_w;
    e.h = p.out_h;
    e.C = p.out_c;
    e.ncomp = p.out_c <= 2 ? 1 : 3;
    e.mode = p.enc_la_gray ? 1 : 0;
    e.src_stride = d.out_stride;
    e.nbx = (p.out_w + 7) / 8;
    e.nby = (p.out_h + 7) / 8;
    e.nblocks = e.nbx * e.nby * e.ncomp;
    int qual = cfg_.jpeg_quality;
    uint8_t q[2][64];
    jpeg_enc_qtables(qual, q);
    memcpy(e.q, q, sizeof(q));
    uint32_t dht_off = 0, sos_off = 0;
    const std::vector<uint8_t> hdr = jpeg_enc_header(p.out_w, p.out_h, (int)e.ncomp, qual, &dht_off, &sos_off);
    e.hdr_len = e.hdr_std = (uint32_t)hdr.size();
    e.hdr_pre = (uint16_t)dht_off;
    e.hdr_sos = (uint16_t)sos_off;
    e.dyn = 0;
    o.hdr = b.blob.size();
    b.blob.insert(b.blob.end(), hdr.begin(), hdr.end());
    o.tout = bl.L.take(p.img_bytes + 16, 256);
    o.ecoef = bl.L.take((size_t)e.nblocks * 128, 256);
    o.ebits = bl.L.take((size_t)e.nblocks * 4, 256);
    o.ewords = (size_t)(e.nblocks * 210ull + 64) / 4 * 4 + 16;  // size for now; placed with the batch's regions
    // option "jenc_optimize": the image's histogram, EncTables and DHT segments (dg_jenc_tree.h) in front of its
    // bit buffer, inside the region the batch zeroes
    o.etab = opt_.jenc_optimize ? kJencOptBytes : 0;
    o.ewords += o.etab;
    b.jenc_opt = b.jenc_opt || opt_.jenc_optimize;
    b.any_enc = true;
  }
}

// The regions of the scratch arena that belong to the batch, not to one image.
void Context::layout_batch_regions(Batch &b, BatchLayout &bl) {
  Layout &L = bl.L;
  if (bl.alias) {  // the late buffers and the chunk entries share one region after the early ones
    const size_t r0 = align_up(L.off, 256);
    L.off = r0 + std::max(bl.LT.off, bl.CH.off);
    for (Offs &o : bl.offs) {
      if (o.late & 1u) o.unf += r0;
      if (o.late & 2u) o.pix += r0;
      if (o.late & 4u) {
        o.out += r0;
        b.out_dev_off[o.img] = o.out;
      }
      for (int s = 0; s < kStages; s++)
        if ((o.late & (8u << s)) && o.pass_dst[s] != (size_t)-1) o.pass_dst[s] += r0;
    }
    for (InfChunk &c : b.ichunks) {
      c.out += r0;
      c.tab += r0;
    }
  }
  b.total_subs = bl.sub_base;
  if (b.any_enc) {  // encoder bit buffers: one contiguous region, zeroed with one memset per batch
    size_t tot = 0;
    for (Offs &o : bl.offs)
      if (o.ewords) {
        const size_t sz = o.ewords;
        o.ewords = tot;
        tot += (sz + 255) / 256 * 256;
      }
    b.words_off = L.take(tot, 256);
    b.words_bytes = tot;
    // (by the descriptor, not by o.tout: a batch's first image may hold tout at offset 0 of the arena, as a
    // BMP without an index plane does)
    for (size_t k = 0; k < bl.offs.size() && k < b.descs.size(); k++)
      if (b.descs[k].enc.active) bl.offs[k].ewords += b.words_off;
    EncTables et;
    jpeg_enc_tables(et);
    while (b.blob.size() % 16) b.blob.push_back(0);
    b.enctab_off = b.blob.size();
    b.blob.insert(b.blob.end(), (const uint8_t *)&et, (const uint8_t *)&et + sizeof(et));
  }
  // PNG unfilter: one progress flag per 64-row band of every plane
  b.uf_n = 0;
  b.uf_maxbpp = 1;
  for (ImageDesc &dd : b.descs)
    if (dd.fmt == kFmtPng) {
      dd.png.uf_flag0 = b.uf_n;
      b.uf_n += png_bands(dd);
      b.uf_maxbpp = std::max(b.uf_maxbpp, dd.png.bpp);
    }
  b.uf_flags_off = b.uf_n ? L.take((size_t)(b.uf_n + 1) * 4) : 0;
  b.pf_n = 0;
  for (const ImageDesc &dd : b.descs)
    if (dd.fmt == kFmtJpeg) b.pf_n += dd.prog;
  b.pf_off = b.pf_n ? L.take((size_t)(b.pf_n + 2) * 4) : 0;  // AC ticket, progress words, DC ticket
  // k_destuff_one: a ticket word + one state word per destuff chunk (zeroed per batch)
  b.ds_n = 0;
  for (const ImageDesc &dd : b.descs)
    if (dd.fmt == kFmtJpeg && !dd.prog) b.ds_n += dd.nchunk;
  b.ds_state_off = (opt_.destuff_one && b.ds_n) ? L.take((size_t)(b.ds_n + 1) * 8) : 0;
  bl.subs_off = L.take(b.total_subs * sizeof(SubState));
  bl.ckpt_off = L.take(std::max<uint64_t>(1, bl.ckpt_total) * (b.nc4 ? sizeof(CkptN<4>) : sizeof(Ckpt)));
  // fused IDCT leftovers: at most one carried-in block per subsequence, plus
  // the blocks of flushes with < 8 active lanes -- the tail of a wave, or
  // every block of an image with fewer subsequences than that.  Sized for
  // the worst case (all blocks of the fused images; 8 B each is small next
  // to their 128 B of coefficients); k_idct_list clamps to it and finish()
  // checks it.
  uint64_t fused_blocks = 0;
  for (const ImageDesc &dd : b.descs)
    if (dd.idct_fused) fused_blocks += dd.total_blocks;
  b.idct_cap = b.any_fused ? (uint32_t)std::min<uint64_t>(2 * b.total_subs + fused_blocks + 4096, 0xFFFFFFF0u) : 0u;
  bl.idct_list_off = L.take((size_t)b.idct_cap * 8 + 16);
}

// Device memory: under the budget (option "max_device_mb") a batch that
// does not fit even with the other slots drained goes back to the caller
// to be split (submit_split); without one, a failed allocation first
// finishes the other slots' batches and frees their buffers, then splits.
dg_status Context::fit_device(Slot &sl, const Batch &b, const BatchLayout &bl) {
  const size_t rs = bl.L.off + 256, rc = bl.CO.off + 256, ri = b.host_io ? bl.IN.off + 64 : 0;
  const bool planned = opt_.max_dev_bytes && opt_.budget_plan && &sl - slots_ < kMaxInflight;
  dg_status st = DG_OK;
  if (planned) {
    st = budget_planned_fit(sl, rs, rc, ri);
    if (st) return st;
  } else {
    if (sl.views) free_slot_buffers(sl);  // (the budget plan was switched off)
    if (!budget_fit(sl, rs, rc, ri)) return kNeedSplit;
  }
  for (int attempt = 0; !planned; attempt++) {
    st = ensure(sl.scratch, rs, sl.st);
    if (!st) st = ensure(sl.coef, rc, sl.st);
    if (!st && b.host_io) st = ensure(sl.input, ri, sl.st);
    if (st != DG_ERR_OOM) break;
    if (attempt > 0) return kNeedSplit;
    for (Slot &o : slots_) {
      if (&o == &sl) continue;
      if (o.batch && !o.batch->done && finish(o)) continue;
      free_slot_buffers(o);
    }
    // the Lanczos table arena counts too (256 MiB by default): with every
    // other batch finished only this one could read it
    bool cache_busy = b.uses_ccache;
    for (const Slot &o : slots_)
      if (&o != &sl && o.batch && !o.batch->done && o.batch->uses_ccache) cache_busy = true;
    if (!cache_busy && d_ccache_.p) ccache_clear(true);
  }
  if (st) return st;
  sl.coef_bytes = bl.CO.off;
  return DG_OK;
}

static void patch_png(const PngHeader &g, const uint8_t *src, char *S, const Offs &o, ImageDesc &d, Batch &b) {
  PngDesc &pd = d.png;
  pd.zs = (uint64_t)(uintptr_t)(S + o.zs);
  pd.raw = (uint64_t)(uintptr_t)(S + o.raw);
  pd.unf = (uint64_t)(uintptr_t)(S + o.unf);
  d.pix = pd.expand ? (uint64_t)(uintptr_t)(S + o.pix) : pd.unf;
  pd.pal = g.ctype == 3 ? o.pal + 1 : 0;  // blob offset + 1, made absolute with the meta buffer
  uint64_t zo = 0;
  for (size_t c = 0; c < g.idat_off.size(); c++) {
    GatherJob j;
    j.src = (uint64_t)(uintptr_t)(src + g.idat_off[c]);
    j.dst = pd.zs + zo;
    j.len = g.idat_len[c];
    j.count = 0;
    zo += g.idat_len[c];
    b.gjobs.push_back(j);
  }
}

static void patch_gif(const GifHeader &g, const uint8_t *src, char *S, const Offs &o, ImageDesc &d, Batch &b) {
  GifDesc &gd = d.gif;
  gd.idx = (uint64_t)(uintptr_t)(S + o.raw);
  d.pix = (uint64_t)(uintptr_t)(S + o.pix);
  gd.pal = o.pal + 1;  // blob offset + 1, made absolute with the meta buffer
  if (g.closed) {      // k_gif_lzw reads through the chain
    gd.src = (uint64_t)(uintptr_t)(src + g.data_off);
    gd.src_end = gd.src + (g.nbytes ? gif_src_index((uint32_t)g.nbytes - 1u, 1u) + 1u : 0u);
    return;
  }
  gd.src = (uint64_t)(uintptr_t)(S + o.zs);
  gd.src_end = gd.src + g.nbytes;
  uint64_t zo = 0;
  for (const GifRun &r : g.runs) {
    GatherJob j;
    j.src = (uint64_t)(uintptr_t)(src + r.off);
    j.dst = gd.src + zo;
    j.len = r.len;
    j.count = r.count;
    zo += (uint64_t)r.len * r.count;
    b.gjobs.push_back(j);
  }
}

static void patch_bmp(const BmpHeader &g, const uint8_t *src, char *S, const Offs &o, ImageDesc &d) {
  BmpDesc &bd = d.bmp;
  d.pix = (uint64_t)(uintptr_t)(S + o.pix);
  bd.src = (uint64_t)(uintptr_t)(src + g.data_off);
  bd.src_end = bd.src + g.data_len;
  if (bd.rle) bd.idx = (uint64_t)(uintptr_t)(S + o.raw);
  bd.pal = g.bits <= 8 ? o.pal + 1 : 0;  // blob offset + 1, made absolute with the meta buffer
}

static void patch_webp(const WebpHeader &g, const uint8_t *src, char *S, const Offs &o, ImageDesc &d) {
  Vp8lDesc &vd = d.vp8l;
  vd.work = (uint64_t)(uintptr_t)(S + o.raw);
  vd.tabs = (uint64_t)(uintptr_t)(S + o.zs);
  d.pix = (uint64_t)(uintptr_t)(S + o.pix);
  vd.src = (uint64_t)(uintptr_t)(src + g.data_off);
  vd.src_end = vd.src + g.nbytes;
}

static void patch_webp_lossy(const Vp8Header &g, const uint8_t *src, char *S, const Offs &o, ImageDesc &d) {
  d.vp8.work = (uint64_t)(uintptr_t)(S + o.raw);
  d.pix = (uint64_t)(uintptr_t)(S + o.pix);
  d.vp8.src = (uint64_t)(uintptr_t)(src + g.chunk_off);
  if (d.dec_c == 4) {
    d.vp8.alph_plane = (uint64_t)(uintptr_t)(S + o.zs);
    if (alph_compression(g.alph_hdr) == kAlphRaw) d.vp8.alph_src = (uint64_t)(uintptr_t)(src + g.alph_off + 1);
  }
}

// ---- 4. patch device addresses
void Context::patch_addresses(const SubmitArgs &a, Slot &sl, Batch &b, const BatchLayout &bl) {
  char *S = (char *)sl.scratch.p;
  for (InfChunk &c : b.ichunks) {
    c.out = (uint64_t)(uintptr_t)(S + c.out);
    c.tab = (uint64_t)(uintptr_t)(S + c.tab);
  }
  int k = 0;
  for (int i = 0; i < a.n; i++) {
    if (b.desc_of[i] < 0) continue;
    ImageDesc &d = b.descs[b.desc_of[i]];
    const Offs &o = bl.offs[k++];
    const uint8_t *src = a.host_io ? (const uint8_t *)sl.input.p + bl.in_off[i] : a.d_srcs[i];
    const uint64_t user_out = a.host_io ? (uint64_t)(uintptr_t)(S + o.out) : (uint64_t)(uintptr_t)a.outs[i];
    const uint64_t out = d.enc.active ? (uint64_t)(uintptr_t)(S + o.tout) : user_out;
    d.out = out;
    if (d.enc.active) {
      EncDesc &e = d.enc;
      e.src = out;
      e.out = user_out;
      e.coef = (uint64_t)(uintptr_t)(S + o.ecoef);
      e.bits = (uint64_t)(uintptr_t)(S + o.ebits);
      e.words = (uint64_t)(uintptr_t)(S + o.ewords + o.etab);
      if (e.png) e.tab = o.etab ? (uint64_t)(uintptr_t)(S + o.ewords) : 0;
      else e.jopt = o.etab ? (uint64_t)(uintptr_t)(S + o.ewords) : 0;
      e.aux = o.eaux ? (uint64_t)(uintptr_t)(S + o.eaux) : 0;
      e.hdr = o.hdr + 1;  // blob offset + 1: made absolute with the meta buffer
    }
    if (d.fmt == kFmtPng)
      patch_png(b.plans[i].png, src, S, o, d, b);
    else if (d.fmt == kFmtGif)
      patch_gif(b.plans[i].gif, src, S, o, d, b);
    else if (d.fmt == kFmtBmp)
      patch_bmp(b.plans[i].bmp, src, S, o, d);
    else if (d.fmt == kFmtWebp)
      patch_webp(b.plans[i].webp, src, S, o, d);
    else if (d.fmt == kFmtVp8)
      patch_webp_lossy(b.plans[i].vp8, src, S, o, d);
    else
      patch_jpeg(b.plans[i].hdr, src, sl, o, b.desc_of[i], b);
    patch_passes(S, o, b.desc_of[i], b);
  }
  for (const Batch::MsScan &ms : b.ms_scans) {  // scan descriptors: a stream inside the parent's source, its buffers
    ImageDesc &d = b.descs[ms.desc];
    const Offs &o = bl.offs[ms.desc];
    const ImageDesc &par = b.descs[ms.parent];
    const uint8_t *src = a.host_io ? (const uint8_t *)sl.input.p + bl.in_off[ms.image] : a.d_srcs[ms.image];
    d.scan = (uint64_t)(uintptr_t)(src + b.plans[ms.image].hdr.scans[ms.scan].off);
    d.coef = par.coef;
    d.ccnt = par.ccnt;
    d.ds = (uint64_t)(uintptr_t)(S + o.ds);
    d.mk = (uint64_t)(uintptr_t)(S + o.mk);
    d.chunk = (uint64_t)(uintptr_t)(S + o.chunk);
  }
  for (const Batch::AlphStream &as : b.alph_streams) {  // alpha streams: inside the parent's source, their own arenas
    Vp8lDesc &vd = b.descs[as.desc].vp8l;
    const Offs &o = bl.offs[as.desc];
    const uint8_t *src = a.host_io ? (const uint8_t *)sl.input.p + bl.in_off[as.image] : a.d_srcs[as.image];
    vd.work = (uint64_t)(uintptr_t)(S + o.raw);
    vd.tabs = (uint64_t)(uintptr_t)(S + o.zs);
    vd.src = (uint64_t)(uintptr_t)(src + b.plans[as.image].vp8.alph_off + 1);
    vd.src_end = vd.src + vd.nbytes;
  }
}

void Context::patch_jpeg(const JpegHeader &h, const uint8_t *src, const Slot &sl, const Offs &o, int di, Batch &b) {
  ImageDesc &d = b.descs[di];
  char *S = (char *)sl.scratch.p;
  d.scan = (uint64_t)(uintptr_t)(src + h.scan_off);
  d.coef = (uint64_t)(uintptr_t)((char *)sl.coef.p + o.coef);
  d.ccnt = (o.ccnt && !(d.pass[0].mode & kHDecode)) ? (uint64_t)(uintptr_t)((char *)sl.coef.p + o.ccnt - 1) : 0;
  if (d.prog) {
    prog_scan_records(h, src, di, b);
  } else if (d.ms.role != kMsParent) {
    d.ds = (uint64_t)(uintptr_t)(S + o.ds);
    d.stage = d.stage_cap ? (uint64_t)(uintptr_t)(S + o.stage) : 0;
    d.mk = (uint64_t)(uintptr_t)(S + o.mk);
    d.chunk = (uint64_t)(uintptr_t)(S + o.chunk);
  }
  for (int c = 0; c < h.ncomp; c++) d.plane[c] = o.plane[c] == (size_t)-1 ? 0 : (uint64_t)(uintptr_t)(S + o.plane[c]);
  d.pix = h.ncomp >= 3 && !d.color_fused ? (uint64_t)(uintptr_t)(S + o.pix) : 0;
}

// One record per scan of a progressive JPEG (descriptor di); level = 1 + the
// highest level of an earlier scan sharing a component and an overlapping
// coefficient band.
void Context::prog_scan_records(const JpegHeader &h, const uint8_t *src, int di, Batch &b) {
  const size_t first = b.pscans.size();
  for (size_t j = 0; j < h.scans.size(); j++) {
    const JpegScan &sc = h.scans[j];
    ProgScan r;
    memset(&r, 0, sizeof(r));
    r.data = (uint64_t)(uintptr_t)(src + sc.off);
    r.len = (uint32_t)(sc.end - sc.off);
    r.image = (uint32_t)di;
    r.ns = (uint32_t)sc.ns;
    for (int q = 0; q < sc.ns; q++) {
      r.comp[q] = (uint32_t)sc.comp[q];
      r.dc[q] = sc.dc_tab[q] >= 0 ? (uint16_t)pool_huff(h.tables[sc.dc_tab[q]]) : 0;
    }
    r.ac = sc.ac_tab >= 0 ? (uint16_t)pool_huff(h.tables[sc.ac_tab]) : 0;
    r.ss = (uint32_t)sc.ss;
    r.se = (uint32_t)sc.se;
    r.ah = (uint32_t)sc.ah;
    r.al = (uint32_t)sc.al;
    r.restart = (uint32_t)sc.restart;
    r.first = (uint32_t)first;
    r.next = kProgNoScan;
    r.pflags = 0;
    uint32_t lvl = 0;
    for (size_t e = 0; e < j; e++) {
      const JpegScan &pr = h.scans[e];
      if (pr.se < sc.ss || sc.se < pr.ss) continue;
      bool share = false;
      for (int x = 0; x < pr.ns; x++)
        for (int y = 0; y < sc.ns; y++) share |= pr.comp[x] == sc.comp[y];
      if (share) {
        lvl = std::max(lvl, b.pscans[first + e].level + 1);
        if (h.scans.size() <= kProgMaxDepScans) r.deps |= 1ull << e;  // larger files: chained only
      }
    }
    r.level = lvl;
    b.pscans.push_back(r);
  }
}

// The resize passes, k_copy's source and the alpha programs' buffers of descriptor di (its
// pix / plane and out are set).
void Context::patch_passes(char *S, const Offs &o, int di, Batch &b) {
  ImageDesc &d = b.descs[di];
  uint64_t cur = (d.fmt != kFmtJpeg || d.ncomp >= 3) ? d.pix : d.plane[0];
  const uint64_t decoded = cur;
  for (int s = 0; s < kStages; s++) {
    ResizePass &ps = d.pass[s];
    if (!ps.kind) continue;
    ps.src = cur + o.pass_srcoff[s];
    ps.dst = o.pass_dst[s] == (size_t)-1 ? d.out : (uint64_t)(uintptr_t)(S + o.pass_dst[s]);
    if (o.pass_cache[s] >= 0) {  // cached tables: bounds, then the weights
      const CEntry &e = ccache_[o.pass_cache[s]];
      char *cb = (char *)d_ccache_.p + e.off;
      ps.bounds = (uint64_t)(uintptr_t)cb;
      ps.coef = (uint64_t)(uintptr_t)(cb + (size_t)ps.out_size * 8);
      if (o.pass_hit[s]) {
        ps.precision = e.precision;
        b.coef_hit.resize(b.descs.size(), 0);
        b.coef_hit[di] |= (uint8_t)(1u << s);
      } else
        b.ccache_prod.push_back({di, s, o.pass_cache[s]});
    } else {
      ps.coef = (uint64_t)(uintptr_t)(S + o.pass_coef[s]);
      ps.bounds = (uint64_t)(uintptr_t)(S + o.pass_bounds[s]);
    }
    cur = ps.dst;
  }
  d.final_src = cur + (d.copy_needed ? o.final_off : 0);
  for (uint32_t k = 0; k < kAlphaPoints; k++) {
    if (!d.aop[k].prog) continue;
    const int sg = o.aop_stage[k];
    if (sg < 0) {
      d.aop[k].buf = decoded;
      d.aop[k].stride = decoded_stride(d);
      d.aop[k].on_decoded = 1;
    } else {
      d.aop[k].buf = d.pass[sg].dst;
      d.aop[k].stride = d.pass[sg].dst_stride;
    }
  }
}

// ---- 5. workgroup lists
void Context::build_lists(Batch &b) {
  for (int l = 0; l < L_COUNT; l++) {  // sized from the previous batch: no regrowth copies
    b.lists[l].clear();
    b.lists[l].reserve(list_hint_[l] + list_hint_[l] / 4);
  }
  ClassLists cl;
  for (int di = 0; di < (int)b.descs.size(); di++) image_items(di, b, cl);
  for (int l = 0; l < L_COUNT; l++) list_hint_[l] = b.lists[l].size();
  if (opt_.entropy_lpt) {
    // Entropy workgroups decode a fixed number of bits, but their time follows
    // the symbol count: images with few coded bits per block (low quality,
    // flat content: short EOB-heavy codes) run up to 2x the mean.  Dispatch
    // those first (workgroups start in list order) so they do not form the
    // kernel's tail.
    auto cost_sort = [&](std::vector<WgItem> &l) {
      std::stable_sort(l.begin(), l.end(), [&](const WgItem &x, const WgItem &y) {
        const ImageDesc &a = b.descs[x.image], &c = b.descs[y.image];
        return (uint64_t)a.scan_len * c.total_blocks < (uint64_t)c.scan_len * a.total_blocks;
      });
    };
    cost_sort(b.lists[L_SYNC]);
    cost_sort(b.lists[L_HUFF]);
  }
  for (uint32_t j = 0; j < (uint32_t)b.gjobs.size(); j++) {
    const GatherJob &gj = b.gjobs[j];  // count != 0: a run of a GIF's sub-blocks
    const uint64_t bytes = gj.count ? (uint64_t)gj.len * gj.count : gj.len;
    for (uint32_t pc = 0; (uint64_t)pc * kGatherPiece < bytes; pc++) b.lists[gj.count ? L_GIF_GATHER : L_GATHER].push_back({j, pc});
  }
  if (b.uf_n) {  // unfilter bands in ticket order: the j-th band of every plane, j = 0, 1, ...
    std::vector<std::vector<uint32_t>> per;  // per PNG image: pass << 24 | band, pass-major
    std::vector<uint32_t> who;
    for (uint32_t di = 0; di < (uint32_t)b.descs.size(); di++) {
      const ImageDesc &d = b.descs[di];
      if (d.fmt != kFmtPng) continue;
      std::vector<uint32_t> v;
      for (uint32_t p = 0; p < (d.png.interlace ? 7u : 1u); p++) {
        const uint32_t nb = png_pass_bands(d, p);
        for (uint32_t k = 0; k < nb; k++) v.push_back(p << 24 | k);
      }
      per.push_back(std::move(v));
      who.push_back(di);
    }
    for (size_t j = 0, more = 1; more; j++) {
      more = 0;
      for (size_t i = 0; i < per.size(); i++)
        if (j < per[i].size()) {
          b.lists[L_UNF].push_back({who[i], per[i][j]});
          more = 1;
        }
    }
  }
  b.prog_level_n.clear();
  for (uint32_t j = 0; j < (uint32_t)b.pscans.size(); j++) {  // L_PROG: scans grouped by level
    const uint32_t lv = b.pscans[j].level;
    if (lv >= b.prog_level_n.size()) b.prog_level_n.resize(lv + 1, 0);
    b.prog_level_n[lv]++;
  }
  b.prog_dc_n = 0;
  if (opt_.prog_pipe) {
    plan_prog_items(b);
  } else {  // one launch per level: scans grouped by level
    std::vector<uint32_t> at(b.prog_level_n.size(), 0);
    for (size_t lv = 1; lv < at.size(); lv++) at[lv] = at[lv - 1] + b.prog_level_n[lv - 1];
    b.lists[L_PROG].resize(b.pscans.size());
    for (uint32_t j = 0; j < (uint32_t)b.pscans.size(); j++)
      b.lists[L_PROG][at[b.pscans[j].level]++] = WgItem{b.pscans[j].image, j};
  }
  for (int c = 0; c < 2; c++) {
    b.decclass[c] = (uint32_t)cl.decl[c].size();
    b.lists[L_DEC].insert(b.lists[L_DEC].end(), cl.decl[c].begin(), cl.decl[c].end());
  }
  for (int c = 0; c < 2; c++) {
    b.hvclass[c] = (uint32_t)cl.hvl[c].size();
    b.lists[L_RHV].insert(b.lists[L_RHV].end(), cl.hvl[c].begin(), cl.hvl[c].end());
  }
  for (int h = 0; h < 2; h++)
    for (int f = 1; f >= 0; f--)  // launch order (launch_resize_hm): fused KS 1, KS 2, byte-fill KS 1, KS 2
      for (int k = 0; k < 2; k++) {
        b.hmclass[h][f][k] = (uint32_t)cl.hm[h][f][k].size();
        auto &l = b.lists[h ? L_RM2 : L_RM0];
        l.insert(l.end(), cl.hm[h][f][k].begin(), cl.hm[h][f][k].end());
      }
  for (int h = 0; h < 2; h++)
    for (int f = 1; f >= 0; f--)  // launch order: fused classes, then byte-fill classes
      for (int c = 0; c < 4; c++) {
        b.hclass[h][f][c] = (uint32_t)cl.hb[h][f][c].size();
        auto &l = b.lists[h ? L_RH2 : L_RH0];
        l.insert(l.end(), cl.hb[h][f][c].begin(), cl.hb[h][f][c].end());
      }
}

// The work items of descriptor di, in its kernels' order.
void Context::image_items(int di, Batch &b, ClassLists &cl) {
  const ImageDesc &d = b.descs[di];
  const uint32_t I = (uint32_t)di;
  auto entropy_items = [&]() {
    // split ranges (write_split): 128 ranges per k_huff_write workgroup, two lanes each
    const uint32_t wstep = (d.ckpt & 2u) ? kSubPerWg / 2 : kSubPerWg;
    for (uint32_t w = 0; w < d.nsub; w += wstep) b.lists[L_HUFF].push_back({I, w});
    for (uint32_t w = 0; w < d.nsub; w += kSubPerWg - 1) b.lists[L_SYNC].push_back({I, w});
    b.descs[di].ds_state0 = (uint32_t)b.lists[L_DESTUFF].size();  // k_destuff_one's state words, list order
    for (uint32_t c = 0; c < d.nchunk; c++) b.lists[L_DESTUFF].push_back({I, c});
    for (uint32_t c = 0; c < d.nchunk; c += kDsWgChunks) b.lists[L_DESTUFF_WG].push_back({I, c});
    b.lists[L_SCAN].push_back({I, 0});
  };
  if (d.ms.role == kMsScan) {  // a multiscan image's scan: the entropy passes only
    entropy_items();
    return;
  }
  for (uint32_t k = 0; k < kAlphaPoints; k++)
    if (d.aop[k].prog) {
      const uint32_t cnt = d.aop[k].width * d.aop[k].rows;
      for (uint32_t it = 0; it < cnt; it += 256) b.lists[L_ALPHA0 + k].push_back({I, it});
    }
  if (d.fmt == kFmtWebp && !d.dec_c) {  // an alpha stream's companion descriptor: the VP8L decode only
    b.lists[L_VP8L].push_back({I, 0});
    return;
  }
  if (d.fmt == kFmtVp8) {
    b.lists[L_VP8].push_back({I, 0});
    if (d.dec_c == 4)
      for (uint32_t it = 0; it < alph_items(d.vp8.alph_filter, d.width, d.height); it++) b.lists[L_ALPH].push_back({I, it});
    for (uint32_t it = 0; it < d.width * d.height; it += 256) b.lists[L_VP8_RGB].push_back({I, it});
  } else if (d.fmt == kFmtWebp) {
    b.lists[L_VP8L].push_back({I, 0});
    for (uint32_t it = 0; it < d.width * d.height; it += 256) b.lists[L_VP8L_STORE].push_back({I, it});
  } else if (d.fmt == kFmtBmp) {
    if (d.bmp.rle) b.lists[L_BMP_RLE].push_back({I, 0});
    for (uint32_t it = 0; it < bmp_row_groups(d.width) * d.height; it += 64) b.lists[L_BMP_EXPAND].push_back({I, it});
  } else if (d.fmt == kFmtGif) {
    b.lists[L_GIF_LZW].push_back({I, 0});
    for (uint32_t it = 0; it < d.width * d.height; it += 256) b.lists[L_GIF_EXPAND].push_back({I, it});
  } else if (d.fmt == kFmtPng) {
    b.lists[L_PNG].push_back({I, 0});
    if (d.png.nchunks) {
      b.lists[L_INF_RES].push_back({I, 0});
      for (uint32_t k = 1; k < d.png.nchunks; k++) b.lists[L_INF_FIND].push_back({d.png.chunk0 + k, 0});
    }
    if (d.sample_bytes == 2)
      for (uint32_t it = 0; it < (d.width + 1) / 2 * d.height; it += 256) b.lists[L_EXPAND16].push_back({I, it});
    else if (d.png.expand)
      for (uint32_t it = 0; it < d.width * d.height; it += 256) b.lists[L_EXPAND].push_back({I, it});
  } else {
    if (d.prog) {
      const uint64_t bytes = (uint64_t)d.total_blocks * 128;
      for (uint32_t c = 0; (uint64_t)c * kProgZeroBytes < bytes; c++) b.lists[L_PROG_ZERO].push_back({I, c});
    } else if (d.ms.role == kMsParent) {  // its scan descriptors decode; k_ms_zero clears what no scan codes
      b.lists[L_MS_ZERO].push_back({I, 0});
    } else {
      entropy_items();
    }
    uint32_t items = 0;
    for (uint32_t c = 0; c < d.ncomp; c++) items += d.cbh[c] * ((d.cbw[c] + 63) / 64);  // kIdctBlocks
    if (!d.idct_fused && !(d.pass[0].mode & kHDecode))  // fused: k_huff_write (+ k_idct_list) / k_band_dec
      for (uint32_t it = 0; it < items; it += opt_.idct_thread ? kIdctItemStride : 1u) b.lists[L_IDCT].push_back({I, it});
    if (d.ncomp >= 3 && !d.color_fused) {  // the RGB image: k_color, or k_cmyk for four components
      uint32_t q = (d.width + 7) / 8 * d.height;
      for (uint32_t it = 0; it < q; it += 256) b.lists[d.ncomp == 4 ? L_CMYK : L_COLOR].push_back({I, it});
    }
  }
  const bool hv = (d.pass[0].mode & kHVFused) != 0;
  if (hv) {  // one workgroup per (V segment of kHVRows rows, column tile)
    const uint32_t tiles = (d.pass[0].width + kHBandCols - 1) / kHBandCols;
    const uint32_t cnt = tiles * ((d.pass[1].rows + kHVRows - 1) / kHVRows);
    const int cls = d.pass[0].ksize + 1 <= 8 ? 0 : 1;
    for (uint32_t it = 0; it < cnt; it++) cl.hvl[cls].push_back({I, it});
  }
  if (d.pass[0].mode & kHDecode) {  // one workgroup per (group of dec_strips 16-row strips, 128-column tile)
    const ResizePass &ps = d.pass[0];
    const uint32_t tiles = (ps.width + kDecCols - 1) / kDecCols;
    const uint32_t strips = (ps.row0 + ps.rows + 15) / 16 - ps.row0 / 16;
    const uint32_t cnt = tiles * ((strips + opt_.dec_strips - 1) / opt_.dec_strips);
    for (uint32_t it = 0; it < cnt; it++) cl.decl[(ps.mode & kHDecWide) ? 1 : 0].push_back({I, it});
  }
  for (int s = 0; s < kStages; s++) {
    const ResizePass &ps = d.pass[s];
    if (!ps.kind) continue;
    if (ps.kind == kR16V || ps.kind == kR16H) {  // 16-bit resize (dg_resize16.hip)
      const bool vp = ps.kind == kR16V;
      const uint32_t entries = vp ? ps.rows : ps.width;
      for (uint32_t j = 0; j < entries; j += 256) b.lists[L_R16T].push_back({I, (uint32_t)s << 31 | j});
      // one workgroup per 256 sample quads (V) / 256 output pixels (H) of a row
      const uint32_t cnt = ps.rows * (((vp ? ps.width / 4 : ps.width) + 255) / 256);
      for (uint32_t it = 0; it < cnt; it++) b.lists[vp ? L_R16V : L_R16H].push_back({I, it});
      continue;
    }
    if (!(di < (int)b.coef_hit.size() && (b.coef_hit[di] >> s) & 1u)) b.lists[L_COEF].push_back({I, (uint32_t)s});
    if (hv && s < 2) continue;  // k_resize_hv runs both
    if (s == 0 && (ps.mode & kHDecode)) continue;  // k_band_dec runs it
    if (ps.kind == 1 && (ps.mode & kHDirect)) {  // one workgroup per (row, 512-column tile)
      uint32_t cnt = ps.rows * ((ps.width + 511) / 512);
      for (uint32_t it = 0; it < cnt; it++) b.lists[s == 0 ? L_RHX0 : L_RHX2].push_back({I, it});
    } else if (ps.kind == 1) {  // one workgroup per (band of rows, column tile)
      const uint32_t rows_per_wg = kHBandRows * ps.bands;
      uint32_t cnt = ((ps.rows + rows_per_wg - 1) / rows_per_wg) * ((ps.width + kHBandCols - 1) / kHBandCols);
      // k_resize_hb<K> reads taps in even-aligned pairs: a window starting
      // at an odd segment position spans ksize + 1 positions
      const uint32_t kk = ps.ksize + 1;
      int cls = kk <= 8 ? 0 : kk <= 16 ? 1 : kk <= 32 ? 2 : 3;
      // the 8- and 16-tap kernels stage narrower segments (hseg_px in kernels.hip)
      while (cls < 2 && h_pass_span(ps) > (cls == 0 ? 192.0 : 384.0)) cls++;
      const int fused = (ps.mode & kHFused) ? 1 : 0;
      const uint32_t ks = opt_.h_mfma ? h_mfma_steps(ps) : 0u;
      if (ks)
        for (uint32_t it = 0; it < cnt; it++) cl.hm[s / 2][fused][ks - 1].push_back({I, it});
      else
        for (uint32_t it = 0; it < cnt; it++) cl.hb[s / 2][fused][cls].push_back({I, it});
      if (fused && d.sem) b.h_zune = 1;  // the planar fused kernels of the zune fill classes
    } else if (opt_.v_tile && (ps.src_stride & 15) == 0) {  // k_resize_vt: 4 waves of (R rows x 1 KiB) tiles
      const uint32_t units = (ps.width * ps.C + 15) / 16;
      const uint32_t tiles = (units + 63) / 64 * ((ps.rows + opt_.v_tile - 1) / opt_.v_tile);
      for (uint32_t it = 0; it < tiles; it += 4) b.lists[s == 1 ? L_RVT1 : L_RVT3].push_back({I, it});
      b.v_tile = opt_.v_tile;
    } else {
      uint32_t cnt = (ps.width * ps.C + 15) / 16 * ps.rows;
      for (uint32_t it = 0; it < cnt; it += 256 * opt_.v_units) b.lists[L_RH0 + s].push_back({I, it});
    }
  }
  if (d.copy_needed) {
    uint32_t cnt = d.out_w * d.out_h;
    for (uint32_t it = 0; it < cnt; it += 256) b.lists[L_COPY].push_back({I, it});
  }
  if (d.enc.active && d.enc.png) {
    const EncDesc &e = d.enc;
    // the transformed image holds 16-bit samples (option "penc16"): its rows go to k_penc_filter16
    const ListId rows = d.out_stride == 2 * d.out_w * d.out_c ? L_PENC_ROW16 : L_PENC_ROW;
    for (uint32_t it = 0; it < e.h; it += 4) b.lists[rows].push_back({I, it});
    for (uint32_t it = 0; it < e.nblocks; it += 256) b.lists[L_PENC_PIECE].push_back({I, it});
    b.lists[L_ENC_IMG].push_back({I, 0});  // k_enc_scan: piece offsets
    b.lists[L_PENC_IMG].push_back({I, 0});
  } else if (d.enc.active) {
    const EncDesc &e = d.enc;
    for (uint32_t it = 0; it < e.nbx * e.nby; it += 256) b.lists[L_ENC_MCU].push_back({I, it});
    for (uint32_t it = 0; it < e.nblocks; it += 256) b.lists[L_ENC_BLK].push_back({I, it});
    b.lists[L_ENC_IMG].push_back({I, 0});
  }
}

// ---- 6. meta buffer: [flags][descs][lists...], staged in pinned memory with the host inputs
dg_status Context::stage_and_upload(const SubmitArgs &a, Slot &sl, Batch &b, const BatchLayout &bl) {
  Layout M;
  b.flags_off = M.take(sizeof(BatchFlags));
  b.desc_off = M.take(b.descs.size() * sizeof(ImageDesc));
  for (int l = 0; l < L_COUNT; l++) b.list_off[l] = M.take(b.lists[l].size() * sizeof(WgItem));
  b.gjob_off = M.take(b.gjobs.size() * sizeof(GatherJob));
  b.ichunk_off = M.take(b.ichunks.size() * sizeof(InfChunk));
  b.pscan_off = M.take(b.pscans.size() * sizeof(ProgScan));
  b.blob_off = M.take(b.blob.size());
  b.meta_bytes = align_up(M.off, 256);  // the host inputs follow, 16-byte aligned for k_meta_pull
  dg_status st = ensure(sl.meta, b.meta_bytes + 256, sl.st);
  if (st) return st;
  for (ImageDesc &d : b.descs) {
    if (d.fmt == kFmtPng && d.png.pal) d.png.pal = (uint64_t)(uintptr_t)((char *)sl.meta.p + b.blob_off + d.png.pal - 1);
    if (d.fmt == kFmtBmp && d.bmp.pal) d.bmp.pal = (uint64_t)(uintptr_t)((char *)sl.meta.p + b.blob_off + d.bmp.pal - 1);
    if (d.fmt == kFmtGif) d.gif.pal = (uint64_t)(uintptr_t)((char *)sl.meta.p + b.blob_off + d.gif.pal - 1);
    if (d.enc.active) {
      d.enc.hdr = (uint64_t)(uintptr_t)((char *)sl.meta.p + b.blob_off + d.enc.hdr - 1);
      if (!d.enc.png) d.enc.tab = d.enc.tab_std = (uint64_t)(uintptr_t)((char *)sl.meta.p + b.blob_off + b.enctab_off);
    }
  }
  size_t stage_bytes = b.meta_bytes + (a.host_io ? bl.IN.off : 0);
  st = ensure_pinned(sl.stage, stage_bytes + 256, sl.st);
  if (st) return st;
  char *P = (char *)sl.stage.p;
  memset(P + b.flags_off, 0, sizeof(BatchFlags));
  b.ptime_off = 0;
  if (opt_.wg_timing) {
    const size_t nrec = b.lists[L_SYNC].size() + b.lists[L_HUFF].size();
    b.ptime_off = b.pscans.empty() ? 0 : nrec * 16 + 64;  // per-scan {start, end} after the entropy records
    st = ensure(sl.wgt, nrec * 16 + 64 + b.pscans.size() * 16, sl.st);
    if (st) return st;
    BatchFlags *bf = (BatchFlags *)(P + b.flags_off);
    bf->wgtime = (uint64_t)(uintptr_t)sl.wgt.p;
    bf->wgtime_write = (uint32_t)b.lists[L_SYNC].size();
  }
  ((BatchFlags *)(P + b.flags_off))->debug = (uint32_t)(opt_.debug_flags >> 16) & 3u;
  ((BatchFlags *)(P + b.flags_off))->prio = (uint32_t)opt_.entropy_prio;
  ((BatchFlags *)(P + b.flags_off))->idct_list = (uint64_t)(uintptr_t)((char *)sl.scratch.p + bl.idct_list_off);
  ((BatchFlags *)(P + b.flags_off))->idct_cap = b.idct_cap;
  memcpy(P + b.desc_off, b.descs.data(), b.descs.size() * sizeof(ImageDesc));
  for (int l = 0; l < L_COUNT; l++)
    if (!b.lists[l].empty()) memcpy(P + b.list_off[l], b.lists[l].data(), b.lists[l].size() * sizeof(WgItem));
  if (!b.gjobs.empty()) memcpy(P + b.gjob_off, b.gjobs.data(), b.gjobs.size() * sizeof(GatherJob));
  if (!b.ichunks.empty()) memcpy(P + b.ichunk_off, b.ichunks.data(), b.ichunks.size() * sizeof(InfChunk));
  if (!b.pscans.empty()) memcpy(P + b.pscan_off, b.pscans.data(), b.pscans.size() * sizeof(ProgScan));
  if (!b.blob.empty()) memcpy(P + b.blob_off, b.blob.data(), b.blob.size());
  if (a.host_io) {
    std::vector<CopyJob> ins;
    for (int i = 0; i < a.n; i++)
      if (b.desc_of[i] >= 0) ins.push_back({P + b.meta_bytes + bl.in_off[i], a.h_srcs[i], a.lens[i]});
    parallel_copy(ins, opt_.copy_threads);
  }
  last_meta_bytes_ = b.meta_bytes;
  return DG_OK;
}

// The staged meta buffer and inputs go to the device on the slot's stream; what
// finish() needs of the layout and of the caller's arrays is kept with the slot and the batch.
dg_status Context::enqueue_upload(const SubmitArgs &a, Slot &sl, Batch &b, const BatchLayout &bl) {
  char *P = (char *)sl.stage.p;
  if (opt_.timing) HIPCHK(hipEventRecord(sl.ev[0], sl.st));
  if (opt_.meta_pull >= 1) {
    launch_meta_pull(sl.st, P, sl.meta.p, b.meta_bytes);
    HIPCHK(hipGetLastError());
  } else {
    HIPCHK(hipMemcpyAsync(sl.meta.p, P, b.meta_bytes, hipMemcpyHostToDevice, sl.st));
  }
  if (a.host_io && bl.IN.off) {  // the coded inputs (dg_submit / dg_decode_one)
    if (opt_.meta_pull >= 2) {  // off by default: dg_decode_one 18.1 -> 16.6 Gpx/s with it (profiles/r04/one_r4i)
      launch_meta_pull(sl.st, P + b.meta_bytes, sl.input.p, bl.IN.off);
      HIPCHK(hipGetLastError());
    } else {
      HIPCHK(hipMemcpyAsync(sl.input.p, P + b.meta_bytes, bl.IN.off, hipMemcpyHostToDevice, sl.st));
    }
  }
  b.stage_ms.clear();
  sl.subs_off = bl.subs_off;  // SubStates and checkpoints live in the scratch arena
  sl.ckpt_off = bl.ckpt_off;
  if (a.host_io) {
    b.host_outs.assign(a.outs, a.outs + a.n);
    b.host_caps.assign(a.caps, a.caps + a.n);
    // outputs into page-locked caller memory go there by DMA, not via the staging buffer
    for (int i = 0; i < a.n; i++)
      if (b.desc_of[i] >= 0 && !b.plans[i].encode && b.plans[i].out_bytes && a.outs[i] &&
          host_pinned(a.outs[i], b.plans[i].out_bytes))
        b.out_direct[i] = 1;
  }
  return DG_OK;
}

}  // namespace dg
