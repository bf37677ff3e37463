// pipeline.cpp — batch runtime for the decode/bucket-resize stage: context
// lifecycle, options, statistics, device memory, launch and finish.
//
// Host work per image is header-only (parse + bucket + buffer layout); all
// pixel and coefficient arithmetic runs in kernels.hip.  A batch is laid out
// in one device scratch arena, its descriptors and workgroup lists go up in
// one H2D copy, and every kernel of the batch is launched on the context's
// stream back to back.  The reference equivalent is one tokio task per sample
// (worker_files.rs:32-72 -> image_processing.rs:341-431).
//
// The batch planner (Context::submit and its phases: the buffer layout, the
// pass plan with band_dec_mode and the other kernel choices, the workgroup
// lists) is in submit.cpp.
#include "pipeline_util.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <thread>

#include "../dg_entropy.h"
#include "../dg_pixel.h"
#include "../dg_vp8.h"
#include "../kernels.h"

namespace dg {

thread_local std::string g_last_error;
void set_error(const std::string &s) { g_last_error = s; }

// Boundary-repair rounds (finish()) before a batch is declared unsettled.
static constexpr int kMaxResyncRounds = 64;

void parallel_copy(const std::vector<CopyJob> &jobs, int nthreads) {
  constexpr size_t kPiece = 1 << 20;
  std::vector<CopyJob> pieces;
  size_t total = 0;
  for (const CopyJob &j : jobs) {
    for (size_t o = 0; o < j.n; o += kPiece)
      pieces.push_back({(char *)j.dst + o, (const char *)j.src + o, std::min(kPiece, j.n - o)});
    total += j.n;
  }
  const int nt = (int)std::min<size_t>((size_t)std::max(1, nthreads), std::max<size_t>(1, total / (4 * kPiece)));
  if (nt <= 1) {
    for (const CopyJob &p : pieces) memcpy(p.dst, p.src, p.n);
    return;
  }
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t k; (k = next.fetch_add(1)) < pieces.size();) memcpy(pieces[k].dst, pieces[k].src, pieces[k].n);
  };
  std::vector<std::thread> ts;
  for (int t = 1; t < nt; t++) ts.emplace_back(work);
  work();
  for (std::thread &t : ts) t.join();
}

static const char *kStageNames[] = {"upload",     "png_inflate", "png_unfilter", "destuff",   "prog_scans",
                                    "huff_sync",  "huff_fix",    "huff_scan",    "huff_write", "coeffs",
                                    "idct",       "color",       "resize_h1",    "resize_v1", "resize_h2",
                                    "resize_v2",  "copy",        "encode",       "download"};
static const int kNumStages = 19;

Context::Context(int device, const dg_image_config *cfg) : device_(device) {
  if (cfg && cfg->crop_and_resize) {
    has_cfg_ = true;
    cfg_ = *cfg;
  } else if (cfg) {
    cfg_ = *cfg;
  }
  if (cfg) opt_.decode_sem = cfg->decode_semantics == 1 ? 1 : 0;
}

Context::~Context() {
  plan_pool_.reset();  // join the planning workers before any HIP object goes
  hipSetDevice(device_);
  sync_all();
  for (int g = 0; g < kPoolGens; g++)
    for (DevBuf *b : {&d_hpool_[g], &d_qpool_[g]})
      if (b->p) hipFree(b->p);
  free_retired();
  for (Slot &sl : slots_) {
    for (auto e : sl.ev) hipEventDestroy(e);
    if (sl.done) hipEventDestroy(sl.done);
    for (hipEvent_t e : {sl.ev_meta, sl.ev_coef, sl.ev_zero, sl.ev_prog, sl.ev_png0, sl.ev_png1})
      if (e) hipEventDestroy(e);
    if (sl.coef.p && !sl.views) hipFree(sl.coef.p);
    for (hipStream_t q : {sl.st, sl.side})
      if (q) hipStreamDestroy(q);
    if (sl.wgt.p) hipFree(sl.wgt.p);
    for (DevBuf *b : {&sl.scratch, &sl.meta, &sl.input})
      if (b->p && (b == &sl.meta || !sl.views)) hipFree(b->p);
    if (sl.arena.p) hipFree(sl.arena.p);
    for (PinBuf *b : {&sl.stage, &sl.out})
      if (b->p) hipHostFree(b->p);
  }
  if (side_) hipStreamSynchronize(side_);
  if (ev_meta_) hipEventDestroy(ev_meta_);
  if (ev_coef_) hipEventDestroy(ev_coef_);
  if (side_) hipStreamDestroy(side_);
  if (stream_) hipStreamDestroy(stream_);
}

dg_status Context::init() {
  if (has_cfg_) {
    // ImageTransformConfig::get_ar_aware_transform asserts (image_processing.rs:78-93)
    if (cfg_.default_image_size == 0 || cfg_.downsampling_ratio == 0 || !(cfg_.min_aspect_ratio > 0.0) ||
        !(cfg_.max_aspect_ratio >= cfg_.min_aspect_ratio)) {
      set_error("invalid image_config (default_image_size/downsampling_ratio/aspect ratios)");
      return DG_ERR_INVALID;
    }
    buckets_.reset(new BucketTable(cfg_.default_image_size, cfg_.downsampling_ratio, cfg_.min_aspect_ratio,
                                   cfg_.max_aspect_ratio));
    if (buckets_->buckets().empty()) {
      set_error("empty bucket table");
      return DG_ERR_INVALID;
    }
  }
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device_ < 0 || device_ >= ndev) {
    set_error("device ordinal out of range");
    return DG_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(device_));
  {
    int ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_));
    if (ncu > 0) ncu_ = (uint32_t)ncu;
  }
  HIPCHK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&ev_meta_, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&ev_coef_, hipEventDisableTiming));
  for (Slot &sl : slots_) {
    sl.ev.resize(kNumStages + 1);
    for (auto &e : sl.ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));

    HIPCHK(hipEventCreateWithFlags(&sl.ev_meta, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&sl.ev_coef, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&sl.ev_zero, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&sl.ev_prog, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&sl.ev_png0, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&sl.ev_png1, hipEventDisableTiming));
  }
  return make_streams(0, kMaxInflight, opt_.slot_queue, 0, opt_.side_queue);  // the progressive slots' on first use
}

// Streams of the progressive slots (option "prog_queue").  A progressive
// batch holds its stream for ~0.1-1 s; HIP maps streams onto the process's
// few hardware queues (GPU_MAX_HW_QUEUES, 4), and kernels behind it in the
// same queue wait for it -- a baseline slot's stream sharing that queue then
// stalls behind the refinement chains.  0: plain streams; 1 / 2: highest /
// lowest priority; 3: a CU mask over every CU (a masked stream gets a
// hardware queue of its own).
dg_status Context::make_prog_streams() {
  return make_streams(kMaxInflight, kProgSlots, opt_.prog_queue, opt_.prog_cus, -1);
}

// A slot's streams on first use: the baseline slots past "slots" and the
// progressive slots have none until a batch goes to them -- every stream
// with a queue of its own is a hardware queue, and eight processes sharing
// one device run out of them (each rank would hold 16).
dg_status Context::slot_streams(Slot &sl) {
  if (sl.st) return DG_OK;
  const int j = (int)(&sl - slots_);
  return j < kMaxInflight ? make_streams(j, 1, opt_.slot_queue, 0, opt_.side_queue)
                          : make_streams(j, 1, opt_.prog_queue, opt_.prog_cus, -1, kAllSlots);
}

// (Re)create the main and side streams of slots [first, first + count):
// mode 0 plain, 1 / 2 highest / lowest priority, 3 a CU mask over `cus` CUs
// (0 = all).  Modes 1-3 get hardware queues of their own.  HIP hands a new
// stream the least-used queue of its pool, so the main streams are made
// first: the slots in use then start on distinct queues, and a side stream
// (side_mode, -1 = mode) shares a queue with at most one other slot's stream.
// Only slots below `limit` (-1: "slots") get streams now; the others on
// first use (slot_streams).
dg_status Context::make_streams(int first, int count, int mode, int cus, int side_mode, int limit) {
  if (limit < 0) limit = opt_.nslots;
  HIPCHK(hipSetDevice(device_));
  int least = 0, greatest = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  for (int j = first; j < first + count; j++) {
    Slot &sl = slots_[j];
    for (hipStream_t *q : {&sl.st, &sl.side}) {
      if (*q) {
        HIPCHK(hipStreamSynchronize(*q));
        HIPCHK(hipStreamDestroy(*q));
        *q = nullptr;
      }
    }
  }
  for (int pass = 0; pass < 2; pass++) {
    const int m = pass == 1 && side_mode >= 0 ? side_mode : mode;
    for (int j = first; j < first + count && (j < limit || count == 1); j++) {
      hipStream_t *q = pass == 0 ? &slots_[j].st : &slots_[j].side;
      if (m == 1 || m == 2) {
        HIPCHK(hipStreamCreateWithPriority(q, hipStreamNonBlocking, m == 1 ? greatest : least));
      } else if (m == 3) {  // cus of the CUs, spread evenly (every ncu/cus-th)
        std::vector<uint32_t> mask((ncu_ + 31) / 32, 0u);
        const uint32_t want = cus > 0 && (uint32_t)cus < ncu_ ? (uint32_t)cus : ncu_;
        for (uint32_t k = 0; k < want; k++) {
          const uint32_t cu = (uint32_t)(((uint64_t)k * ncu_) / want);
          mask[cu / 32] |= 1u << (cu % 32);
        }
        HIPCHK(hipExtStreamCreateWithCUMask(q, (uint32_t)mask.size(), mask.data()));
      } else {
        HIPCHK(hipStreamCreateWithFlags(q, hipStreamNonBlocking));
      }
    }
  }
  return DG_OK;
}

dg_status Context::host_register(void *ptr, size_t bytes) {
  HIPCHK(hipSetDevice(device_));
  if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) != hipSuccess) {
    set_error("hipHostRegister failed");
    return DG_ERR_DEVICE;
  }
  std::lock_guard<std::mutex> lk(reg_mu_);
  registered_.push_back({(uintptr_t)ptr, bytes});
  return DG_OK;
}

dg_status Context::host_unregister(void *ptr) {
  {
    std::lock_guard<std::mutex> lk(reg_mu_);
    for (size_t i = 0; i < registered_.size(); i++)
      if (registered_[i].first == (uintptr_t)ptr) {
        registered_.erase(registered_.begin() + (long)i);
        break;
      }
  }
  sync_all();  // no copy into the range may still be in flight
  HIPCHK(hipSetDevice(device_));
  return hipHostUnregister(ptr) == hipSuccess ? DG_OK : DG_ERR_INVALID;
}

bool Context::host_pinned(const void *ptr, size_t bytes) {
  const uintptr_t a = (uintptr_t)ptr;
  {
    std::lock_guard<std::mutex> lk(reg_mu_);
    for (const auto &r : registered_)
      if (a >= r.first && a + bytes <= r.first + r.second) return true;
  }
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
    (void)hipGetLastError();  // plain pageable memory: not an error
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

dg_status Context::sync_all() {
  bool ok = true;
  for (hipStream_t q : {stream_, side_})
    if (q) ok &= hipStreamSynchronize(q) == hipSuccess;
  for (Slot &sl : slots_)
    for (hipStream_t q : {sl.st, sl.side})
      if (q) ok &= hipStreamSynchronize(q) == hipSuccess;
  if (!ok) {
    set_error("HIP stream synchronisation failed");
    return DG_ERR_DEVICE;
  }
  return DG_OK;
}

// A rejected option names itself, the value and the accepted range in
// dg_last_error (the range as the condition that rejects it).
static dg_status opt_error(const std::string &k, int64_t v, const std::string &why) {
  set_error(option_error_text(k.c_str(), v, why));
  return DG_ERR_INVALID;
}

// mu_ held: the batches in flight on slots [first, first + count) finish.
dg_status Context::finish_slots(int first, int count) {
  for (int j = first; j < first + count; j++) {
    Slot &sl = slots_[j];
    if (sl.batch && !sl.batch->done) {
      dg_status st = finish(sl);
      if (st) return st;
    }
  }
  return DG_OK;
}

// The keys, their fields and the values they take are the table in
// options.cpp (apply_option is its find, check and store in a row); here is
// what a key does around the store.  A value is checked before anything
// changes, and a key whose slots must finish first stores once they have.
dg_status Context::set_option(const std::string &k, int64_t v) {
  const OptRow *r = find_option(k.c_str());
  if (!r) return opt_error(k, v, "unknown option");
  if (!option_takes(*r, v)) return opt_error(k, v, r->why);
  std::unique_lock<std::mutex> lk;  // held through the store and what follows it
  switch (r->after) {
    case kAfterCoalesce:
      lk = std::unique_lock<std::mutex>(cmu_);
      break;
    case kAfterCoefCache:
      lk = std::unique_lock<std::mutex>(mu_);
      for (const Slot &o : slots_)
        if (o.batch && !o.batch->done && o.batch->uses_ccache) return opt_error(k, v, "not while a batch in flight uses the table cache");  // not while tables are in use
      break;
    case kAfterProgQueue: {
      {
        std::lock_guard<std::mutex> plk(pmu_);
        if (!pagg_.empty()) flush_pagg_locked();
      }
      lk = std::unique_lock<std::mutex>(mu_);
      dg_status st = finish_slots(kMaxInflight, kProgSlots);
      if (st) return st;
      break;
    }
    case kAfterSlotQueue: {
      queue_set_ = true;
      lk = std::unique_lock<std::mutex>(mu_);
      dg_status st = finish_slots(0, kMaxInflight);
      if (st) return st;
      break;
    }
    default:
      break;
  }
  store_option(*r, opt_, v);
  switch (r->after) {
    case kAfterCoefCache:
      ccache_clear(true);
      break;
    case kAfterMaxDevice:
      budget_slots_ = kMaxInflight;
      budget_planned_ = false;
      // Contexts under a budget are the ones that share a device (several
      // ranks, or a loader beside training): their slot streams share the
      // process's hardware queues instead of taking two of their own each --
      // 8 ranks x 4 slots x 2 own queues oversubscribed the device's queues
      // (profiles/r05/ranks: 6-9 Gpx/s at 4 slots, 104 at 2).  An explicit
      // slot_queue / side_queue wins.
      if (v > 0 && !queue_set_ && (opt_.slot_queue != 0 || opt_.side_queue != -1)) {
        lk = std::unique_lock<std::mutex>(mu_);
        dg_status st = finish_slots(0, kMaxInflight);
        if (st) return st;
        opt_.slot_queue = 0;
        opt_.side_queue = -1;
        bool any = false;
        for (int j = 0; j < kMaxInflight; j++) any = any || slots_[j].st;
        if (any) return make_streams(0, kMaxInflight, opt_.slot_queue, 0, opt_.side_queue);
      }
      break;
    case kAfterBudgetPlan:
      budget_planned_ = false;
      break;
    case kAfterSlots:
      next_slot_ %= opt_.nslots;
      break;
    case kAfterProgQueue:
      return make_prog_streams();
    case kAfterSlotQueue:
      return make_streams(0, kMaxInflight, opt_.slot_queue, 0, opt_.side_queue);
    case kAfterResetHostUs:
      for (double &x : host_us_) x = 0;
      for (double &x : host_cpu_us_) x = 0;
      break;
    default:
      break;
  }
  return DG_OK;
}

int64_t Context::get_stat(const std::string &k) {
  if (k == "batches") return stat_batches_;
  if (k == "coalesced_batches") return stat_coalesced_batches_;
  if (k == "coalesced_images") return stat_coalesced_images_;
  if (k == "resync_rounds") return stat_resync_;
  if (k == "fix_workgroups") return stat_fix_;
  if (k == "write_mismatch") return stat_mismatch_;
  if (k == "unsettled_batches") return stat_unsettled_;
  if (k == "prog_items") return stat_prog_items_;
  if (k == "prog_aggregates") return stat_prog_aggs_;
  if (k == "prog_aggregate_images") return stat_prog_agg_images_;
  if (k == "prog_chains") return stat_prog_chains_;
  if (k == "pool_flushes") return stat_pool_flush_;
  if (k == "sync_iters_max") return stat_iters_;
  if (k == "sync_chain") return opt_.sync_chain;
  {  // wg_timing summaries, in nanoseconds: wg_{sync,write}_{span,mean,p90,max}
    static const char *kn[2] = {"sync", "write"}, *sn[4] = {"span", "mean", "p90", "max"};
    for (int a = 0; a < 2; a++)
      for (int q = 0; q < 4; q++)
        if (k == std::string("wg_") + kn[a] + "_" + sn[q]) return (int64_t)(wgstat_[a][q] * 1000.0);
  }
  if (k == "sub_bits") return last_sub_bits_;
  if (k == "sub_auto") return opt_.sub_auto;
  if (k == "coalesce_inflight") return opt_.coalesce_inflight;
  if (k == "meta_bytes") return (int64_t)last_meta_bytes_;
  if (k == "allocs") return stat_allocs_;
  if (k == "alloc_mb") return stat_alloc_mb_;
  if (k == "alloc_us") return (int64_t)stat_alloc_us_;
  if (k == "reclaims") return stat_reclaims_;
  if (k == "peak_device_mb") return stat_peak_dev_ >> 20;
  if (k == "device_mb") {
    std::lock_guard<std::mutex> lk(mu_);
    return (int64_t)(dev_footprint() >> 20);
  }
  if (k == "max_device_mb") return (int64_t)(opt_.max_dev_bytes >> 20);
  if (k == "budget_splits") return stat_budget_splits_;
  if (k == "budget_plan_mb") return (int64_t)(plan_arena_ >> 20);  // planned bytes per slot
  if (k == "budget_slots") return opt_.max_dev_bytes ? std::min<int64_t>(opt_.nslots, stat_budget_slots_min_) : opt_.nslots;
  if (k == "coef_cache_hits") return stat_ccache_hits_;
  if (k == "coef_cache_new") return stat_ccache_new_;
  if (k == "coef_cache_resets") return stat_ccache_resets_;
  if (k == "coef_cache_mb") return (int64_t)(ccache_off_ >> 20);
  if (k == "budget_frees") return stat_budget_frees_;
  if (k == "budget_oom") return stat_budget_oom_;
  if (k == "retire_syncs") return stat_retire_syncs_;
  if (k == "png_serial_fallbacks") return stat_png_serial_;
  if (k == "band_dec_images") return stat_band_dec_;
  if (k == "direct_d2h") return stat_direct_d2h_;
  if (k == "png_chunks") return stat_png_chunks_;
  if (k == "png_small_streams") return stat_png_small_;
  {  // host microseconds spent in dg_submit* since the last reset, per phase: wall and thread CPU
    static const char *pn[8] = {"plan", "pools", "layout", "lists", "upload", "h2d", "launch", "slotwait"};
    for (int q = 0; q < 8; q++) {
      if (k == std::string("host_us_") + pn[q]) return (int64_t)host_us_[q];
      if (q < 7 && k == std::string("host_cpu_us_") + pn[q]) return (int64_t)host_cpu_us_[q];
    }
  }
  if (k == "hpool") return (int64_t)hpool_.size();
  if (k == "qpool") return (int64_t)qpool_.size();
  set_error("dg_ctx_get_stat(\"" + k + "\"): unknown statistic");
  return -1;
}


int Context::timings(const char **names, float *ms, int cap) {
  int n = (int)last_ms_.size();
  for (int i = 0; i < n && i < cap; i++) {
    if (names) names[i] = kStageNames[i];
    if (ms) ms[i] = last_ms_[i];
  }
  return n;
}

// Grow a device buffer.  `user`: the only stream that can still be using it
// (a slot's own buffers); nullptr = shared by every stream (the table pools).
// Growing a buffer never frees the old one on the spot: hipFree / hipHostFree
// synchronise the whole device, which would make a baseline batch's growth
// wait for a ~1 s progressive aggregate on another slot (and serialised the
// aggregates).  The caller guarantees the old buffer is idle (a slot's
// previous batch is finished before its buffers are reused), so it is only
// retired and freed later: at destruction, or once retired buffers pass
// kRetiredMax, after a sync of every stream.
// Device and page-locked host memory have limits of their own: several ranks
// per host each keeping GiBs of grown-out buffers page-locked would pin a lot
// of the host's memory.  Retired buffers are also freed at the first idle
// moment (a wait that leaves no batch in flight, free_retired_if_idle).
// 32 GiB of retired device buffers at most before a device-wide sync frees
// them (growth happens while a workload sets new size maxima, i.e. in its
// first batches; a lower limit made those batches sync every few growths).
// Ranks sharing one device should set a budget (option "max_device_mb"):
// under a budget nothing is retired -- a grown-out buffer is freed at once.
static constexpr size_t kRetiredDevMax = (size_t)32 << 30;
static constexpr size_t kRetiredPinMax = (size_t)512 << 20;

void Context::retire(void *p, size_t bytes, bool pinned) {
  (pinned ? retired_pinned_ : retired_dev_).push_back(p);
  (pinned ? retired_pin_bytes_ : retired_dev_bytes_) += bytes;
  if ((retired_dev_bytes_ > kRetiredDevMax || retired_pin_bytes_ > kRetiredPinMax) && sync_all() == DG_OK) {
    stat_retire_syncs_++;
    free_retired();
  }
}

void Context::free_retired() {
  for (void *p : retired_dev_) hipFree(p);
  for (void *p : retired_pinned_) hipHostFree(p);
  retired_dev_.clear();
  retired_pinned_.clear();
  retired_dev_bytes_ = retired_pin_bytes_ = 0;
}

void Context::note_alloc(std::chrono::steady_clock::time_point t0, size_t bytes) {
  stat_allocs_++;
  stat_alloc_mb_ += (int64_t)(bytes >> 20);
  stat_alloc_us_ += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

size_t Context::grow_cap(size_t bytes, bool headroom) {
  return align_up(std::max(bytes, (size_t)1 << 20) + (headroom ? bytes / 2 : 0), 1 << 20);
}

// An allocation failed: free the retired buffers (after a sync of every
// stream; the failed call is about to fail the submit anyway) so the retry
// sees them.  True = worth retrying.
bool Context::reclaim() {
  (void)hipGetLastError();
  stat_reclaims_++;
  if (sync_all() != DG_OK) return false;
  free_retired();
  return true;
}

// mu_ held.  hipFree synchronises the device, so only when nothing is in flight.
void Context::free_retired_if_idle() {
  if (retired_dev_.empty() && retired_pinned_.empty()) return;
  for (const Slot &s : slots_)
    if (s.batch && !s.batch->done) return;
  free_retired();
}

// exact: no growth headroom and no reclaim on failure (prewarm_slots: a
// failed allocation there just leaves the slot to grow on first use)
dg_status Context::ensure(DevBuf &b, size_t bytes, hipStream_t user, bool exact) {
  (void)user;
  if (b.cap >= bytes) return DG_OK;
  if (b.p) {
    if (opt_.max_dev_bytes) {  // under a budget the old buffer is gone now (budget_fit counted it so)
      hipFree(b.p);
    } else {
      retire(b.p, b.cap, false);
    }
    b.p = nullptr;
    b.cap = 0;
  }
  // 50% headroom: an allocation blocks on the driver (8 ranks sharing one
  // GPU measured 36-209 ms of wall time per step in the layout phase against
  // 0.3 ms of CPU while batches kept setting new size maxima,
  // profiles/r04/ranks), so growth must stay rare.  (Headroom on re-growth
  // only cost configs[1] 1.4 ms of submit time per batch: the extra growths
  // retired enough to trigger device-wide syncs.)  Under memory pressure the
  // retired buffers go first, then the headroom.
  // no headroom once the device is three quarters full (several ranks or
  // contexts sharing one device: 8 ranks x 4 slots x 1.5 ran a 288 GB device
  // out of memory, profiles/r04/ranks_r4f); under a budget, only the room
  // budget_fit left.
  size_t dfree = 0, dtotal = 0;
  const bool roomy = hipMemGetInfo(&dfree, &dtotal) != hipSuccess || dfree > dtotal / 4 + bytes;
  size_t cap = exact ? align_up(bytes, (size_t)1 << 20) : grow_cap(bytes, roomy);
  if (opt_.max_dev_bytes) {
    const size_t lim = align_up(bytes, 1 << 20) + (budget_room_ / 3 & ~(((size_t)1 << 20) - 1));
    cap = std::min(cap, std::max(lim, align_up(bytes, 1 << 20)));
    budget_room_ -= std::min(budget_room_, cap - std::min(cap, bytes));
  }
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipMalloc(&b.p, cap);
  if (e != hipSuccess && !exact && reclaim()) {
    cap = grow_cap(bytes, false);
    e = hipMalloc(&b.p, cap);
  }
  note_alloc(t0, cap);
  if (e != hipSuccess) {
    if (exact) {
      (void)hipGetLastError();
      b.p = nullptr;
      return DG_ERR_OOM;
    }
    set_error("device allocation failed");
    b.p = nullptr;
    return DG_ERR_OOM;
  }
  b.cap = cap;
  stat_peak_dev_ = std::max<int64_t>(stat_peak_dev_, (int64_t)dev_footprint());
  return DG_OK;
}

// Device bytes the context holds: every slot's buffers, the table pools and
// the retired buffers not yet freed (`except`'s buffers left out).
size_t Context::dev_footprint(const Slot *except) const {
  size_t t = retired_dev_bytes_;
  for (const Slot &o : slots_) {
    if (&o == except) continue;
    for (const DevBuf *b : {&o.meta, &o.wgt, &o.arena}) t += b->cap;
    if (!o.views)
      for (const DevBuf *b : {&o.scratch, &o.input, &o.coef}) t += b->cap;
  }
  for (int g = 0; g < kPoolGens; g++) t += d_hpool_[g].cap + d_qpool_[g].cap;
  return t + d_ccache_.cap;
}

// The arena is nearly full: start it over once no batch in flight reads or
// writes it (finishing them first, as a pool flush does).  Runs before a
// batch's lookups, so a batch never mixes entries of two arena lifetimes.
void Context::ccache_maybe_reset(Slot &self) {
  if (!opt_.ccache_cap || (!ccache_full_ && ccache_off_ <= opt_.ccache_cap / 8 * 7)) return;
  for (Slot &o : slots_) {
    if (&o == &self || !o.batch || o.batch->done || !o.batch->uses_ccache) continue;
    if (finish(o)) return;  // keep the arena as it is; the next batch tries again
  }
  ccache_clear(false);
  stat_ccache_resets_++;
}

// Forget every entry; free_arena: give the device arena back too (the next lookup allocates it again).
void Context::ccache_clear(bool free_arena) {
  ccache_index_clear();
  ccache_.clear();
  ccache_off_ = 0;
  ccache_full_ = false;
  if (free_arena && d_ccache_.p) {
    hipFree(d_ccache_.p);
    d_ccache_.p = nullptr;
    d_ccache_.cap = 0;
  }
}

void Context::ccache_index_clear() { ccache_slot_.assign((size_t)1 << kCIdxBits, -1); }

int Context::ccache_find(const CKey &k, uint32_t &slot) const {
  const uint32_t mask = (1u << kCIdxBits) - 1u;
  slot = (uint32_t)CKeyHash()(k) & mask;
  for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
    const int32_t e = ccache_slot_[slot];
    if (e < 0) return -1;
    if (ccache_[e].key == k) return e;
  }
  return -1;
}

void Context::ccache_rollback(size_t n0, size_t off0) {
  if (ccache_.size() <= n0) return;
  ccache_.resize(n0);  // (rare: a submit that installed no batch) rebuild the index
  ccache_index_clear();
  for (size_t i = 0; i < ccache_.size(); i++) {
    uint32_t slot;
    ccache_find(ccache_[i].key, slot);
    ccache_slot_[slot] = (int32_t)i;
  }
  ccache_off_ = std::min(ccache_off_, off0);
}

int Context::ccache_lookup(const ResizePass &ps, Batch &b, bool &hit) {
  hit = false;
  if (!opt_.ccache_cap || opt_.max_dev_bytes && opt_.ccache_cap > opt_.max_dev_bytes / 8) return -1;
  CKey k;
  memcpy(&k.in0, &ps.in0, 8);
  memcpy(&k.in1, &ps.in1, 8);
  k.in_size = ps.in_size;
  k.out_size = ps.out_size;
  k.ksize = ps.ksize;
  if (ccache_slot_.empty()) ccache_index_clear();
  uint32_t slot;
  const int found = ccache_find(k, slot);
  if (found >= 0) {
    if (!ccache_[found].ready) return -1;  // a batch in flight is writing it: compute our own copy
    hit = true;
    b.uses_ccache = true;
    stat_ccache_hits_++;
    return found;
  }
  const size_t bytes = align_up((size_t)ps.out_size * 8 + (size_t)ps.out_size * ps.ksize * 2, 256);
  // full (arena, or the index at 3/4 load): the next submit starts the arena over
  if (ccache_off_ + bytes > opt_.ccache_cap || ccache_.size() >= ((size_t)3 << kCIdxBits) / 4) {
    ccache_full_ = true;
    return -1;
  }
  if (!d_ccache_.p) {
    if (hipMalloc(&d_ccache_.p, opt_.ccache_cap) != hipSuccess) {
      (void)hipGetLastError();
      d_ccache_.p = nullptr;
      opt_.ccache_cap = 0;  // no cache on this device
      return -1;
    }
    d_ccache_.cap = opt_.ccache_cap;
  }
  const int idx = (int)ccache_.size();
  ccache_.push_back(CEntry{k, ccache_off_, 0, false});
  ccache_slot_[slot] = idx;
  ccache_off_ += bytes;
  b.uses_ccache = true;
  stat_ccache_new_++;
  return idx;
}

// An idle slot's device buffers (no batch, or its batch finished).
void Context::free_slot_buffers(Slot &o) {
  if (o.views) {  // carved from the arena
    for (DevBuf *b : {&o.scratch, &o.input, &o.coef}) {
      b->p = nullptr;
      b->cap = 0;
    }
    o.views = false;
  }
  for (DevBuf *b : {&o.scratch, &o.meta, &o.input, &o.coef, &o.arena}) {
    if (!b->p) continue;
    hipFree(b->p);
    b->p = nullptr;
    b->cap = 0;
    stat_budget_frees_++;
  }
}

// mu_ held.  Planned budget (option "budget_plan"): the first baseline batch
// under the budget decides how many batches fit in flight and sizes every
// slot then -- an even share of the budget left after the table pools, the
// Lanczos cache and a 1/32 reserve for the descriptor buffers, split over
// scratch / coefficients / input in the first batch's proportions, at least
// 1.25x what that batch needs -- so that a loader sharing its GPU (ranks, or
// training) allocates and frees nothing after its first batch: hipMalloc took
// ~170 ms and hipFree synchronised the device inside the timed window of the
// 8-ranks-on-one-GPU rehearsal.  A later batch that does
// not fit its slot is split (kNeedSplit), never grown; its input arena
// (host-in submissions after device-in ones) is the one buffer added later.
dg_status Context::budget_planned_fit(Slot &sl, size_t rs, size_t rc, size_t ri) {
  const size_t MB = (size_t)1 << 20;
  budget_room_ = 0;
  // this batch's scratch / coefficient / input views of the slot's arena
  const size_t os = 0, oc = align_up(rs, 256), oi = oc + align_up(rc, 256), need = oi + ri;
  auto carve = [&]() {
    char *a = (char *)sl.arena.p;
    sl.scratch = DevBuf{a + os, rs};
    sl.coef = DevBuf{a + oc, rc};
    sl.input = DevBuf{ri ? a + oi : nullptr, ri};
    sl.views = true;
    const size_t fp = dev_footprint();
    budget_room_ = fp < opt_.max_dev_bytes ? (opt_.max_dev_bytes - fp) / 2 : 0;
  };
  if (budget_planned_) {
    if (need > plan_arena_) return kNeedSplit;
    if (!sl.arena.p) {  // a planned slot without its arena (a progressive batch took the room): take it back
      if (sl.scratch.p || sl.coef.p || sl.input.p) free_slot_buffers(sl);
      if (dev_footprint() + plan_arena_ > opt_.max_dev_bytes || ensure(sl.arena, plan_arena_, sl.st, true))
        return kNeedSplit;
    }
    carve();
    return DG_OK;
  }
  // first sizing: every other slot gives its buffers back (a budget set on a
  // context that ran without one), then the plan
  for (int j = 0; j < kAllSlots; j++) {
    Slot &o = slots_[j];
    if (&o == &sl) continue;
    if (o.batch && !o.batch->done && finish(o)) return DG_ERR_DEVICE;
    free_slot_buffers(o);
  }
  free_slot_buffers(sl);
  if (!retired_dev_.empty() && sync_all() == DG_OK) free_retired();
  const size_t others = dev_footprint(&sl) + sl.meta.cap + sl.wgt.cap;
  if (others >= opt_.max_dev_bytes) return kNeedSplit;
  // descriptor / weight buffers of the planned slots grow into the reserve
  const size_t reserve =
      std::min<size_t>(std::max<size_t>(opt_.max_dev_bytes / 32, 64 * MB), (opt_.max_dev_bytes - others) / 4);
  size_t avail = opt_.max_dev_bytes - others - reserve;
  {  // a budget above what the device has free plans for what it has (less 1/8 for the others on it)
    size_t dfree = 0, dtotal = 0;
    if (hipMemGetInfo(&dfree, &dtotal) == hipSuccess) avail = std::min(avail, dfree - std::min(dfree, dtotal / 8));
  }
  if (need + need / 4 > avail) return kNeedSplit;  // the halves plan the budget
  const int ns = (int)std::max<size_t>(1, std::min<size_t>((size_t)opt_.nslots, avail / (need + need / 4)));
  plan_arena_ = (avail / (size_t)ns) & ~(MB - 1);
  if (ensure(sl.arena, plan_arena_, sl.st, true)) {
    set_error("device allocation of the planned budget failed");
    return DG_ERR_OOM;
  }
  budget_slots_ = ns;
  stat_budget_slots_min_ = std::min<int64_t>(stat_budget_slots_min_, ns);
  budget_planned_ = true;
  next_slot_ = 1 % ns;
  carve();
  budget_room_ = reserve / 2;
  return DG_OK;
}

// mu_ held.  The device budget (option "max_device_mb"): make room for a
// batch of `self` whose scratch / coefficient / input arenas need rs / rc /
// ri bytes.  In order: keep self's buffers if they already fit; free the
// retired buffers; give back the buffers of baseline slots the budget took
// out of turn; then take the highest other baseline slot out of turn
// (budget_slots_: pick_slot cycles over fewer slots from now on), finishing
// its batch (waiting for its GPU work, as a dg_wait would) and freeing its
// buffers, and likewise the progressive slots; finally drop self's own
// oversized buffers (idle: the slot's previous batch is finished) for
// exact-size ones.  So a budget below what "slots" batches need settles on
// fewer batches in flight instead of trading buffers between slots batch
// after batch (each trade a hipFree + hipMalloc).  False: the batch alone
// does not fit -- the caller splits it (submit_split).  budget_room_: what
// growth may add on top.  (The descriptor buffer, a few MB, grows after this
// check.)
bool Context::budget_fit(Slot &self, size_t rs, size_t rc, size_t ri) {
  budget_room_ = 0;
  if (!opt_.max_dev_bytes) return true;
  const size_t fixed = self.meta.cap + self.wgt.cap;
  const size_t keep = std::max(self.scratch.cap, rs) + std::max(self.coef.cap, rc) + std::max(self.input.cap, ri) + fixed;
  const size_t tight = rs + rc + ri + fixed;
  const int si = (int)(&self - slots_);
  auto others = [&] { return dev_footprint(&self); };
  auto give_back = [&](Slot &o) {
    if (o.batch && !o.batch->done && finish(o)) return;
    free_slot_buffers(o);
  };
  auto has_buffers = [](const Slot &o) { return o.scratch.p || o.coef.p || o.input.p || o.arena.p; };
  if (others() + keep > opt_.max_dev_bytes && !retired_dev_.empty() && sync_all() == DG_OK) free_retired();
  if (budget_planned_) {  // (a progressive slot) the planned baseline slots keep their buffers
    for (int j = kMaxInflight; j < kAllSlots && others() + keep > opt_.max_dev_bytes; j++)
      if (j != si) give_back(slots_[j]);
    if (others() + keep <= opt_.max_dev_bytes) {
      budget_room_ = opt_.max_dev_bytes - others() - keep;
      return true;
    }
    if (others() + tight > opt_.max_dev_bytes) return false;
    free_slot_buffers(self);
    budget_room_ = opt_.max_dev_bytes - others() - tight;
    return true;
  }
  for (int j = std::max(1, budget_slots_); j < kMaxInflight && others() + keep > opt_.max_dev_bytes; j++)
    if (j != si && has_buffers(slots_[j])) give_back(slots_[j]);
  while (others() + keep > opt_.max_dev_bytes) {
    int j = kMaxInflight - 1;
    while (j >= 0 && (j == si || !has_buffers(slots_[j]))) j--;
    if (j < 0) break;
    give_back(slots_[j]);
    if (has_buffers(slots_[j])) break;  // its batch failed to finish: nothing more to take
    budget_slots_ = std::max(1, std::min(budget_slots_, std::max(j, si + 1)));
    stat_budget_slots_min_ = std::min<int64_t>(stat_budget_slots_min_, budget_slots_);
  }
  for (int j = kMaxInflight; j < kAllSlots && others() + keep > opt_.max_dev_bytes; j++)
    if (j != si) give_back(slots_[j]);
  if (others() + keep <= opt_.max_dev_bytes) {
    budget_room_ = opt_.max_dev_bytes - others() - keep;
    return true;
  }
  if (others() + tight > opt_.max_dev_bytes) return false;
  free_slot_buffers(self);
  budget_room_ = opt_.max_dev_bytes - others() - tight;
  return true;
}

dg_status Context::ensure_pinned(PinBuf &b, size_t bytes, hipStream_t user, bool exact) {
  (void)user;
  if (b.cap >= bytes) return DG_OK;
  if (b.p) {
    retire(b.p, b.cap, true);
    b.p = nullptr;
    b.cap = 0;
  }
  size_t cap = exact ? align_up(bytes, (size_t)1 << 20) : grow_cap(bytes, true);
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipHostMalloc(&b.p, cap, hipHostMallocDefault);
  if (e != hipSuccess && !exact && reclaim()) {
    cap = grow_cap(bytes, false);
    e = hipHostMalloc(&b.p, cap, hipHostMallocDefault);
  }
  note_alloc(t0, cap);
  if (e != hipSuccess && exact) {
    (void)hipGetLastError();
    b.p = nullptr;
    return DG_ERR_OOM;
  }
  if (e != hipSuccess) {
    set_error("pinned host allocation failed");
    b.p = nullptr;
    return DG_ERR_OOM;
  }
  b.cap = cap;
  return DG_OK;
}

// Table pools.  Huffman and quantisation tables are de-duplicated by content
// into per-context pools that the kernels index with 16-bit slots.  Pools are
// not grow-only: once a pool holds more than kPoolKeep tables (a long-running
// loader over per-image-optimised JPEGs adds ~4 new tables per image; a
// progressive file ~10-12, one per scan), the next submit starts the pools
// over in the next of kPoolGens device generations, waiting only for batches
// that still read that generation (round 2 drained every batch in flight
// here -- with progressive aggregates that was a ~1 s stall of every slot,
// and it serialised the aggregates).  Only a single batch that alone needs
// more than kPoolMax tables sends its overflow images back as
// DG_ERR_UNSUPPORTED (the caller's CPU path), never as CORRUPT.
// (kPoolKeep and kPoolMax are in pipeline_util.h: the planner checks them too)

dg_status Context::flush_pools() {
  const int next = (pool_gen_ + 1) % kPoolGens;
  for (int s = 0; s < kAllSlots; s++) {  // batches in flight still reading (and may resync with) that generation
    Slot &o = slots_[s];
    if (o.batch && !o.batch->done && o.batch->pool_gen == next) {
      dg_status st = finish(o);
      if (st) return st;
    }
  }
  hpool_.clear();
  hpool_idx_.clear();
  qpool_.clear();
  qpool_idx_.clear();
  for (RecentTab &r : hrecent_) r.idx = -1;
  for (RecentTab &r : qrecent_) r.idx = -1;
  hpool_uploaded_ = qpool_uploaded_ = 0;
  pool_gen_ = next;
  stat_pool_flush_++;
  return DG_OK;
}

// Table de-duplication.  Loaders mostly see a handful of distinct tables
// (the encoder's standard ones), so a few recently pooled tables are compared
// byte for byte first; only a miss builds the key string and hashes it (the
// per-table string and hash were 0.65 ms of a 1,024-image WebDataset submit).
static int recent_find(RecentTab *r, int n, const uint8_t *key, uint32_t len) {
  for (int i = 0; i < n; i++)
    if (r[i].idx >= 0 && r[i].len == len && memcmp(r[i].key, key, len) == 0) return r[i].idx;
  return -1;
}

static void recent_put(RecentTab *r, int n, uint32_t &next, const uint8_t *key, uint32_t len, int idx) {
  RecentTab &e = r[next++ % (uint32_t)n];
  e.len = len;
  memcpy(e.key, key, len);
  e.idx = idx;
}

int Context::pool_huff(const HuffSpec &s) {
  uint8_t raw[17 + 256];
  memcpy(raw, s.bits, 17);
  const uint32_t len = 17 + (uint32_t)std::max(0, std::min(256, s.nvals));
  memcpy(raw + 17, s.vals, len - 17);
  int idx = recent_find(hrecent_, kRecentTabs, raw, len);
  if (idx >= 0) return idx;
  std::string key((const char *)raw, len);
  auto it = hpool_idx_.find(key);
  if (it != hpool_idx_.end()) {
    idx = it->second;
  } else {
    HuffTable t;
    if (!build_huff_table(s, t)) return -1;
    if (hpool_.size() >= kPoolMax) return -2;
    hpool_.push_back(t);
    idx = (int)hpool_.size() - 1;
    hpool_idx_[key] = idx;
  }
  recent_put(hrecent_, kRecentTabs, hrecent_next_, raw, len, idx);
  return idx;
}

int Context::pool_quant(const uint16_t *q) {
  int idx = recent_find(qrecent_, kRecentTabs, (const uint8_t *)q, 128);
  if (idx >= 0) return idx;
  std::string key((const char *)q, 128);
  auto it = qpool_idx_.find(key);
  if (it != qpool_idx_.end()) {
    idx = it->second;
  } else {
    QuantTable t;
    memcpy(t.q, q, 128);
    if (qpool_.size() >= kPoolMax) return -2;
    qpool_.push_back(t);
    idx = (int)qpool_.size() - 1;
    qpool_idx_[key] = idx;
  }
  recent_put(qrecent_, kRecentTabs, qrecent_next_, (const uint8_t *)q, 128, idx);
  return idx;
}

dg_status Context::upload_pools() {
  DevBuf &hb = d_hpool_[pool_gen_], &qb = d_qpool_[pool_gen_];
  if (!hb.p) {  // each generation is allocated once, at full capacity: no reallocation, no device sync
    if (dg_status st = ensure(hb, kPoolMax * sizeof(HuffTable))) return st;
    if (dg_status st = ensure(qb, kPoolMax * sizeof(QuantTable))) return st;
  }
  // appends only: entries below *_uploaded_ may be in use by batches in flight
  if (hpool_.size() != hpool_uploaded_) {
    HIPCHK(hipMemcpyAsync((char *)hb.p + hpool_uploaded_ * sizeof(HuffTable), &hpool_[hpool_uploaded_],
                          (hpool_.size() - hpool_uploaded_) * sizeof(HuffTable), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipStreamSynchronize(stream_));  // the host vector may reallocate later
    hpool_uploaded_ = hpool_.size();
  }
  if (qpool_.size() != qpool_uploaded_) {
    HIPCHK(hipMemcpyAsync((char *)qb.p + qpool_uploaded_ * sizeof(QuantTable), &qpool_[qpool_uploaded_],
                          (qpool_.size() - qpool_uploaded_) * sizeof(QuantTable), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    qpool_uploaded_ = qpool_.size();
  }
  return DG_OK;
}

// The 16-bit resize of a W x H x C image to its ow x oh bucket (option
// "resize16"): resize_to_fill's geometry, the tap counts of both passes and
// the samples of a decoded row that the f32 intermediate holds -- it covers
// the crop window's rows and the columns the cropped outputs' taps read.
// False (p.png.why set) where the GPU path does not take the image.
static bool plan_r16(uint32_t W, uint32_t H, uint32_t C, uint32_t ow, uint32_t oh, ImagePlan &p) {
  p.r16 = true;
  if (!r16_geom(W, H, ow, oh, p.r16g)) {
    p.png.why = "PNG: 16-bit resize whose scaled size does not cover the bucket";
    return false;
  }
  const R16Geom &g = p.r16g;
  p.r16_passes = !(g.w2 == W && g.h2 == H);
  if (!p.r16_passes) return true;  // a pure crop: the source's own samples
  int32_t cmin = (int32_t)W, cmax = 0, kh = 0, kv = 0;
  for (uint32_t x = 0; x < ow; x++) {
    const R16Window b = r16_window(W, g.w2, g.x0 + x);
    cmin = std::min(cmin, b.left);
    cmax = std::max(cmax, b.right);
    kh = std::max(kh, b.right - b.left);
  }
  for (uint32_t y = 0; y < oh; y++) {
    const R16Window b = r16_window(H, g.h2, g.y0 + y);
    kv = std::max(kv, b.right - b.left);
  }
  // whole quads of samples (k_r16_v: 8 bytes in, 16 out per lane); the decoded
  // row's stride is a multiple of 8 samples, so the last quad stays inside it
  p.r16_s0 = ((uint32_t)cmin * C) & ~3u;
  p.r16_ns = (uint32_t)align_up((size_t)cmax * C, 4) - p.r16_s0;
  p.r16_kv = (uint32_t)kv;
  p.r16_kh = (uint32_t)kh;
  // the intermediate and the tap tables stay 32-bit addressable, like the decoder's working set
  if ((uint64_t)p.r16_ns * 4 * oh >= (1ull << 31) || (uint64_t)oh * p.r16_kv * 4 >= (1ull << 31) ||
      (uint64_t)ow * p.r16_kh * 4 >= (1ull << 31)) {
    p.png.why = "PNG: 16-bit resize whose f32 intermediate is too large for the GPU path";
    return false;
  }
  return true;
}

// Decide what the GPU will do with one image: header, bucket, output size.
dg_status Context::plan_image(const uint8_t *h, size_t len, int32_t forced, ImagePlan &p) {
  p = ImagePlan();
  if (!h || len == 0) {
    p.status = DG_ERR_CORRUPT;
    return DG_OK;
  }
  uint32_t W, H, C;
  if (is_png(h, len)) {
    p.fmt = kFmtPng;
    parse_png_header(h, len, p.png, opt_.png16);
    if (p.png.status != PH_OK) {
      p.status = p.png.status == PH_UNSUPPORTED ? DG_ERR_UNSUPPORTED : DG_ERR_CORRUPT;
      return DG_OK;
    }
    // the decoder's working set (raw + unfiltered + expanded) must stay 32-bit addressable
    const uint64_t raw = p.png.rawlen;
    const uint64_t sb = p.png.depth == 16 ? 2 : 1;  // bytes per expanded sample
    if (raw >= (1ull << 31) || (uint64_t)p.png.width * p.png.height * 4ull * sb >= (1ull << 31) ||
        p.png.zlen >= (1ull << 28)) {
      if (sb == 2) p.png.why = "PNG: 16-bit image too large for the GPU path";
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
    W = p.png.width;
    H = p.png.height;
    C = (uint32_t)p.png.out_c;
  } else if (opt_.gif && is_gif(h, len)) {  // option "gif"
    p.fmt = kFmtGif;
    parse_gif_header(h, len, p.gif);
    if (p.gif.status != GH_OK) {
      p.status = p.gif.status == GH_UNSUPPORTED ? DG_ERR_UNSUPPORTED : DG_ERR_CORRUPT;
      return DG_OK;
    }
    // the working set (code bytes, index plane, Rgba8 screen) stays 32-bit addressable, as the PNG path's
    if ((uint64_t)p.gif.width * p.gif.height * 4ull >= (1ull << 31) || (uint64_t)p.gif.fw * p.gif.fh >= (1ull << 31) ||
        p.gif.nbytes >= (1ull << 28)) {
      p.gif.why = "GIF: image too large for the GPU path";
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
    W = p.gif.width;
    H = p.gif.height;
    C = 4;
  } else if (opt_.bmp && is_bmp(h, len)) {  // option "bmp"
    p.fmt = kFmtBmp;
    parse_bmp_header(h, len, p.bmp);
    if (p.bmp.status != BH_OK) {
      p.status = p.bmp.status == BH_UNSUPPORTED ? DG_ERR_UNSUPPORTED : DG_ERR_CORRUPT;
      return DG_OK;
    }
    // the limits of the GIF path: the pixel buffer, the index plane and the stream stay 32-bit addressable
    if ((uint64_t)p.bmp.width * p.bmp.height * 4ull >= (1ull << 31) || p.bmp.data_len >= (1ull << 31) ||
        ((p.bmp.compression == BMP_RLE8 || p.bmp.compression == BMP_RLE4) && p.bmp.data_len >= (1ull << 28))) {
      p.bmp.why = "BMP: image too large for the GPU path";
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
    W = p.bmp.width;
    H = p.bmp.height;
    C = (uint32_t)p.bmp.out_c;
  } else if (opt_.webp_lossy && is_webp_lossy(h, len) && (parse_webp_lossy(h, len, p.vp8, opt_.webp_alpha), p.vp8.claim)) {
    // option "webp_lossy": a file whose image chunk is VP8L is not claimed and goes on to "webp" below
    p.fmt = kFmtVp8;
    if (p.vp8.status != WH_OK) {
      p.status = p.vp8.status == WH_UNSUPPORTED ? DG_ERR_UNSUPPORTED : DG_ERR_CORRUPT;
      return DG_OK;
    }
    // the limits of the GIF path
    if ((uint64_t)p.vp8.width * p.vp8.height * 4ull >= (1ull << 31) || p.vp8.chunk_len >= (1u << 28)) {
      p.vp8.why = "WebP: image too large for the GPU path";
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
    W = p.vp8.width;
    H = p.vp8.height;
    C = (opt_.webp_alpha && p.vp8.has_alph) ? 4 : 3;  // option "webp_alpha"
  } else if (opt_.webp && is_webp(h, len)) {  // option "webp"
    p.fmt = kFmtWebp;
    parse_webp_header(h, len, p.webp);
    if (p.webp.status != WH_OK) {
      p.status = p.webp.status == WH_UNSUPPORTED ? DG_ERR_UNSUPPORTED : DG_ERR_CORRUPT;
      return DG_OK;
    }
    // the limits of the GIF path: the pixel buffer and the bit count stay 32-bit addressable
    if ((uint64_t)p.webp.width * p.webp.height * 4ull >= (1ull << 31) || p.webp.nbytes >= (1ull << 28)) {
      p.webp.why = "WebP: image too large for the GPU path";
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
    W = p.webp.width;
    H = p.webp.height;
    C = p.webp.alpha ? 4 : 3;
  } else {
    if (!is_jpeg(h, len)) {
      p.status = DG_ERR_CORRUPT;
      return DG_OK;
    }
    // options "jpeg_h1v2", "jpeg_cmyk", "jpeg_multiscan"
    parse_jpeg_header(h, len, p.hdr, opt_.jpeg_h1v2, opt_.jpeg_cmyk, opt_.jpeg_multiscan);
    if (p.hdr.status != JH_OK) {
      p.status = p.hdr.status == JH_UNSUPPORTED ? DG_ERR_UNSUPPORTED : DG_ERR_CORRUPT;
      return DG_OK;
    }
    if (p.hdr.progressive && !opt_.progressive) {  // see option "progressive"
      p.hdr.why = "progressive JPEG (context option \"progressive\" decodes it on the GPU)";
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
    if (p.hdr.incomplete_refinement && opt_.decode_sem == 0) {
      // libjpeg-turbo would smooth these blocks (jdcoefct.c smoothing_ok); zune-jpeg does not
      p.hdr.why = "incomplete progressive refinement (libjpeg block smoothing; decodes with decode_semantics 1)";
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
    W = p.hdr.width;
    H = p.hdr.height;
    C = p.hdr.ncomp == 1 ? 1 : 3;
    // component planes (padded to whole MCUs) must stay below 4 GiB: the
    // upsampling kernels address rows with 24-bit multiplies.  The reference's
    // decoder refuses far smaller images already (image's 512 MiB max_alloc).
    if ((uint64_t)(W + 32) * (H + 32) >= (1ull << 32)) {
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
  }
  p.channels = (int32_t)C;  // pre-transform (image_processing.rs:349-351)
  const bool deep = p.fmt == kFmtPng && p.png.depth == 16;  // option "png16" (parse_png_header refuses them without)
  p.bit_depth = deep && !cfg_.image_to_rgb8 ? 16 : 8;       // to_rgb8 (:367-372) leaves Rgb8
  uint32_t ow = W, oh = H;
  if (has_cfg_) {
    int b = forced;
    if (b == -1) {
      b = buckets_->closest((int32_t)W, (int32_t)H);
    } else if (b < -1 || b >= (int)buckets_->buckets().size()) {  // -2: "NaN" key (dg_sample_align)
      p.status = DG_ERR_BAD_BUCKET;
      return DG_OK;
    }
    p.bucket = b;
    ow = buckets_->buckets()[b].w;
    oh = buckets_->buckets()[b].h;
  }
  p.out_w = ow;
  p.out_h = oh;
  p.out_c = cfg_.image_to_rgb8 ? 3 : C;  // convert_to_rgb8 (:163-186)
  if (cfg_.image_to_rgb8) p.channels = 3;  // image_processing.rs:367-372
  p.out_bytes = (uint64_t)ow * oh * p.out_c * (p.bit_depth == 16 ? 2 : 1);
  p.img_bytes = p.out_bytes;
  if (deep && has_cfg_ && !(W == ow && H == oh)) {
    // the reference resizes non-U8 pixel types with image's own f32 Lanczos3
    // (resize_to_fill), not the fast_image_resize path restated here
    if (!opt_.resize16) {
      p.png.why = "PNG: 16-bit resize (only a 16-bit image of its bucket's size decodes on the GPU)";
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
    if (!plan_r16(W, H, C, ow, oh, p)) {
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
  }
  const bool deep_enc = deep && cfg_.pre_encode_images && !cfg_.image_to_rgb8;  // 16-bit samples at an encoder
  if (deep_enc && !opt_.penc16) {
    p.png.why = "PNG: 16-bit image to an encoder (the GPU encoders take 8-bit samples)";
    p.status = DG_ERR_UNSUPPORTED;
    return DG_OK;
  }
  if (deep_enc && cfg_.encode_format != 0) {  // image 0.25's JpegEncoder rejects 16-bit colour types: the reference drops the sample
    p.png.why = "PNG: 16-bit image to the JPEG encoder (it takes 8-bit samples only; option \"penc16\" covers encode_format png)";
    p.status = DG_ERR_UNSUPPORTED;
    return DG_OK;
  }
  if (cfg_.pre_encode_images) {  // image_processing.rs:374-419
    p.encode = true;
    p.enc_png = cfg_.encode_format == 0;
    // a resized LA image is a GrayImage over its LA bytes by now (image_to_dyn_image);
    // a resized LA16 image went through resize_to_fill instead and is still LumaA16
    p.enc_la_gray = !deep_enc && p.out_c == 2 && has_cfg_ && !(W == p.out_w && H == p.out_h);
    p.out_bytes = p.enc_png ? png_enc_bound(ow, oh, p.enc_la_gray ? 1 : p.out_c, deep_enc ? 2 : 1)
                            : jpeg_enc_bound(ow, oh, p.out_c);
    p.channels = -1;  // :416
    // the encoders count bits in 32-bit offsets (~400 MB of output): larger
    // images stay on the caller's CPU encoder
    if (p.out_bytes >= (1ull << 29)) {
      p.status = DG_ERR_UNSUPPORTED;
      return DG_OK;
    }
  }
  return DG_OK;
}

dg_status Context::output_size(const uint8_t *bytes, size_t len, int32_t forced, uint64_t *nbytes) {
  ImagePlan p;
  plan_image(bytes, len, forced, p);
  *nbytes = p.out_bytes;
  if (p.status)
    set_error(p.fmt == kFmtPng    ? p.png.why
              : p.fmt == kFmtGif  ? p.gif.why
              : p.fmt == kFmtBmp  ? p.bmp.why
              : p.fmt == kFmtWebp ? p.webp.why
              : p.fmt == kFmtVp8  ? p.vp8.why
                                  : (p.hdr.why ? p.hdr.why : "unsupported"));
  return (dg_status)p.status;
}

// The first batches (no budget): the idle baseline slots in turn take the
// buffers and streams the submitting slot has, exactly sized, while its batch
// runs -- so a slot's first batch does not pay for its streams, hipMalloc /
// hipHostMalloc and growth steps (the headline's fourth slot did, inside the
// first timed window: 110 vs 115-117 Gpx/s in the other four windows).
void Context::prewarm_slots(const Slot &self) {
  if (&self - slots_ >= kMaxInflight) return;
  const int ns = opt_.max_dev_bytes ? std::max(1, std::min(opt_.nslots, budget_slots_)) : opt_.nslots;
  for (int j = 0; j < ns; j++) {
    Slot &o = slots_[j];
    if (&o == &self || (o.batch && !o.batch->done)) continue;
    if (slot_streams(o)) return;
    if (self.views) {  // planned budget: the slot's arena
      if (ensure(o.arena, self.arena.cap, nullptr, true) || ensure(o.meta, self.meta.cap, nullptr, true) ||
          ensure(o.wgt, self.wgt.cap, nullptr, true) || ensure_pinned(o.stage, self.stage.cap, nullptr, true) ||
          ensure_pinned(o.out, self.out.cap, nullptr, true))
        return;
      continue;
    }
    if (ensure(o.scratch, self.scratch.cap, nullptr, true) || ensure(o.coef, self.coef.cap, nullptr, true) ||
        ensure(o.input, self.input.cap, nullptr, true) || ensure(o.meta, self.meta.cap, nullptr, true) ||
        ensure(o.wgt, self.wgt.cap, nullptr, true) || ensure_pinned(o.stage, self.stage.cap, nullptr, true) ||
        ensure_pinned(o.out, self.out.cap, nullptr, true))
      return;
  }
}

// A slot for the next batch: the next in turn, whose batch the caller then
// finishes first.  Progressive batches have slots of their own
// (pick_prog_slot), so every baseline slot cycles at the baseline pace.
int Context::pick_slot() {
  // the planned budget's first sizing runs on slot 0 (budget_planned_fit sizes
  // slots [0, budget_slots_)); submissions split before it keep that slot
  if (opt_.max_dev_bytes && opt_.budget_plan && !budget_planned_) {
    next_slot_ = 0;
    return 0;
  }
  const int ns = opt_.max_dev_bytes ? std::max(1, std::min(opt_.nslots, budget_slots_)) : opt_.nslots;
  const int i = next_slot_ % ns;
  next_slot_ = (i + 1) % ns;
  return i;
}

// A progressive slot: the first idle one, else the next in turn (whose batch
// the caller then waits for: backpressure on the progressive lane only).
int Context::pick_prog_slot() {
  for (int j = 0; j < kProgSlots; j++) {
    const int k = kMaxInflight + (next_pslot_ + j) % kProgSlots;
    const Slot &s = slots_[k];
    if (!s.batch || s.batch->done || hipEventQuery(s.done) == hipSuccess) {
      next_pslot_ = (next_pslot_ + j + 1) % kProgSlots;
      return k;
    }
  }
  const int k = kMaxInflight + next_pslot_;
  next_pslot_ = (next_pslot_ + 1) % kProgSlots;
  return k;
}

// Work items of the pipelined progressive launch (dg_prog.hip k_prog_scan).
// Scans of one image that share no (component, coefficient band) never wait
// on each other, so the connected groups of the dependency graph -- for a
// colour file the DC scans, and the AC scans of each component -- can each
// run back to back in one wave (a chain, ProgScan::next).  A chained scan
// never waits: its deps ran before it in the same wave.  That is the whole
// point: with one wave per scan, an image's later scans sit resident for its
// whole duration waiting on their producers' rows (10 waves per image for
// libjpeg's default script), and the batch's LDS-bound residency went to
// waiting waves.  A group whose decode costs more than prog_chain % of the
// batch's longest single scan (the long pole when every scan is pipelined)
// keeps one wave per scan and the row pipeline, so chaining never lengthens
// the batch.  Cost model: coded bytes + blocks / 2.  Items needing more than
// one Huffman table in LDS (DC-first scans of several components) go last
// (prog_dc_n) and run in a launch of their own with four tables.  Order:
// pipelined scans first (image by image, largest first, each in level order:
// a scan only ever waits on one with a lower ticket), then chains, costliest
// first.
void Context::plan_prog_items(Batch &b) {
  auto &list = b.lists[L_PROG];
  list.clear();
  const uint32_t n = (uint32_t)b.pscans.size();
  if (!n) return;
  std::vector<double> cost(n);
  double longest = 0;
  for (uint32_t j = 0; j < n; j++) {
    const ProgScan &sc = b.pscans[j];
    const ImageDesc &d = b.descs[sc.image];
    uint64_t blocks;
    if (sc.ns == 1) {
      const uint32_t c = sc.comp[0];
      blocks = (uint64_t)((d.cdsw[c] + 7) / 8) * ((d.cdsh[c] + 7) / 8);
    } else {
      blocks = (uint64_t)d.mcux * d.mcuy * d.bpm;
    }
    cost[j] = (double)sc.len + 0.5 * (double)blocks;
    longest = std::max(longest, cost[j]);
  }
  std::vector<uint32_t> par(n);
  for (uint32_t j = 0; j < n; j++) par[j] = j;
  auto find = [&](uint32_t x) {
    while (par[x] != x) x = par[x] = par[par[x]];
    return x;
  };
  // groups: scans of one image sharing a component and an overlapping band
  // (the deps relation, computed directly: files with more than
  // kProgMaxDepScans scans have no deps mask and run chained only)
  std::vector<uint8_t> nodeps(b.descs.size(), 0);
  for (uint32_t j = 0; j < n; j++) {
    const ProgScan &sj = b.pscans[j];
    if (sj.image < nodeps.size() && b.descs[sj.image].prog > kProgMaxDepScans) nodeps[sj.image] = 1;
    for (uint32_t e = sj.first; e < j; e++) {
      const ProgScan &se_ = b.pscans[e];
      if (se_.se < sj.ss || sj.se < se_.ss) continue;
      bool share = false;
      for (uint32_t x = 0; x < se_.ns && x < 4; x++)
        for (uint32_t y = 0; y < sj.ns && y < 4; y++) share |= se_.comp[x] == sj.comp[y];
      if (!share) continue;
      const uint32_t a = find(j), c = find(e);
      if (a != c) par[std::max(a, c)] = std::min(a, c);
    }
  }
  struct Group {
    std::vector<uint32_t> scans;  // ascending: every dep of a scan comes before it
    double cost = 0;
    bool dc = false;
  };
  std::vector<Group> groups;
  std::vector<int32_t> gi(n, -1);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t r = find(j);
    if (gi[r] < 0) {
      gi[r] = (int32_t)groups.size();
      groups.emplace_back();
    }
    Group &g = groups[gi[r]];
    const ProgScan &sc = b.pscans[j];
    g.scans.push_back(j);
    g.cost += cost[j];
    g.dc |= (sc.ss == 0 && sc.ah == 0 ? sc.ns : (sc.ss == 0 ? 0u : 1u)) > 1;
  }
  const double limit = longest * (double)opt_.prog_chain / 100.0;
  std::vector<uint32_t> split[2];            // pipelined scans, AC / DC launch
  std::vector<std::pair<double, uint32_t>> chains[2];  // (cost, group)
  std::vector<double> img_cost(b.descs.size(), 0.0);
  for (uint32_t j = 0; j < n; j++) img_cost[b.pscans[j].image] += cost[j];
  for (uint32_t g = 0; g < (uint32_t)groups.size(); g++) {
    Group &G = groups[g];
    if ((opt_.prog_chain > 0 && G.cost <= limit) || nodeps[b.pscans[G.scans[0]].image]) {
      for (size_t i = 0; i < G.scans.size(); i++) {
        ProgScan &sc = b.pscans[G.scans[i]];
        sc.pflags |= kProgChained;
        sc.next = i + 1 < G.scans.size() ? G.scans[i + 1] : kProgNoScan;
      }
      chains[G.dc].push_back({G.cost, g});
    } else {
      for (uint32_t j : G.scans) split[G.dc].push_back(j);
    }
  }
  for (int dc = 0; dc < 2; dc++) {
    std::stable_sort(split[dc].begin(), split[dc].end(), [&](uint32_t x, uint32_t y) {
      const ProgScan &a = b.pscans[x], &c = b.pscans[y];
      if (a.image != c.image) {
        if (img_cost[a.image] != img_cost[c.image]) return img_cost[a.image] > img_cost[c.image];
        return a.image < c.image;
      }
      if (a.level != c.level) return a.level < c.level;
      return x < y;
    });
    std::stable_sort(chains[dc].begin(), chains[dc].end(),
                     [](const auto &x, const auto &y) { return x.first > y.first; });
  }
  for (int dc = 0; dc < 2; dc++) {
    for (uint32_t j : split[dc]) list.push_back(WgItem{b.pscans[j].image, j});
    for (const auto &c : chains[dc]) {
      const uint32_t j = groups[c.second].scans[0];
      list.push_back(WgItem{b.pscans[j].image, j});
    }
  }
  b.prog_dc_n = (uint32_t)(split[1].size() + chains[1].size());
  stat_prog_items_ += list.size();
  stat_prog_chains_ += chains[0].size() + chains[1].size();
}

dg_status Context::launch_all(Slot &sl, bool from_fix) {
  Batch &b = *sl.batch;
  char *M = (char *)sl.meta.p;
  const ImageDesc *dd = (const ImageDesc *)(M + b.desc_off);
  ImageDesc *dm = (ImageDesc *)(M + b.desc_off);
  BatchFlags *fl = (BatchFlags *)(M + b.flags_off);
  SubState *subs = (SubState *)((char *)sl.scratch.p + sl.subs_off);
  const HuffTable *hp = b.hp;  // the pool generation this batch was planned against
  const QuantTable *qp = b.qp;
  auto lst = [&](int l) { return (const WgItem *)(M + b.list_off[l]); };
  auto cnt = [&](int l) { return (uint32_t)b.lists[l].size(); };
  auto ev = [&](int i) -> dg_status {
    if (opt_.timing) HIPCHK(hipEventRecord(sl.ev[i], sl.st));
    return DG_OK;
  };
  if (from_fix) HIPCHK(hipMemsetAsync(fl, 0, kFlagCounters, sl.st));
  int evi = 1;  // event i closes stage i-1 (kStageNames)
  auto next = [&]() -> dg_status { return ev(evi++); };
  // a resync round re-runs everything downstream of the entropy decode; the
  // decoded images themselves (PNG, alpha programs on them) are not redone
  const int alpha_flags = from_fix ? 1 : 0;
  if (next()) return DG_ERR_DEVICE;
  if (!from_fix && cnt(L_R16T)) {  // 16-bit resize: tap tables depend only on the plan (beside the inflate / unfilter)
    if (opt_.side_stream) {
      HIPCHK(hipEventRecord(sl.ev_meta, sl.st));
      HIPCHK(hipStreamWaitEvent(sl.side, sl.ev_meta, 0));
    }
    launch_r16_taps(opt_.side_stream ? sl.side : sl.st, dd, lst(L_R16T), cnt(L_R16T));
  }
  if (!from_fix && b.any_png) {
    launch_png_gather(sl.st, (const GatherJob *)(M + b.gjob_off), lst(L_GATHER), cnt(L_GATHER));
    if (!b.ichunks.empty()) {
      // streams too small to chunk (masks) inflate serially on the side stream,
      // beside the chunked kernels (which leave most CUs idle); chunked images
      // the resolve gives up on follow on the main stream
      const bool beside = opt_.side_stream;
      if (beside) {
        HIPCHK(hipEventRecord(sl.ev_png0, sl.st));
        HIPCHK(hipStreamWaitEvent(sl.side, sl.ev_png0, 0));
        launch_png_inflate(sl.side, dm, lst(L_PNG), cnt(L_PNG), 0, fl, ncu_);
        HIPCHK(hipEventRecord(sl.ev_png1, sl.side));
      }
      InfChunk *ich = (InfChunk *)(M + b.ichunk_off);
      launch_inf_find(sl.st, dd, ich, lst(L_INF_FIND), cnt(L_INF_FIND), opt_.inf_stage3);
      launch_inf_decode(sl.st, dd, ich, (uint32_t)b.ichunks.size(), opt_.inf_decode);
      launch_inf_resolve(sl.st, dm, ich, lst(L_INF_RES), cnt(L_INF_RES));
      launch_png_inflate(sl.st, dm, lst(L_PNG), cnt(L_PNG), beside ? 1 : 2, fl, ncu_);
      if (beside) HIPCHK(hipStreamWaitEvent(sl.st, sl.ev_png1, 0));
    } else {
      launch_png_inflate(sl.st, dm, lst(L_PNG), cnt(L_PNG), 2, fl, ncu_);  // serial: every stream
    }
  }
  if (!from_fix && b.any_gif) {  // GIF: code stream -> index plane (the entropy stage of these images)
    launch_gif_gather(sl.st, (const GatherJob *)(M + b.gjob_off), lst(L_GIF_GATHER), cnt(L_GIF_GATHER));
    launch_gif_lzw(sl.st, dm, lst(L_GIF_LZW), cnt(L_GIF_LZW));
  }
  if (!from_fix && b.any_bmp) launch_bmp_rle(sl.st, dm, lst(L_BMP_RLE), cnt(L_BMP_RLE));  // BMP: RLE stream -> index plane
  if (!from_fix && b.any_webp) {  // lossless WebP: bitstream -> ARGB plane -> inverse transforms
    launch_vp8l_decode(sl.st, dm, lst(L_VP8L), cnt(L_VP8L));
    launch_vp8l_inverse(sl.st, dm, lst(L_VP8L), cnt(L_VP8L));
  }
  if (!from_fix && b.any_vp8) {  // lossy WebP: partitions -> records and coefficients -> planes -> loop filter
    launch_vp8_parse(sl.st, dm, lst(L_VP8), cnt(L_VP8));
    launch_vp8_recon(sl.st, dm, lst(L_VP8), cnt(L_VP8));
    launch_vp8_filter(sl.st, dm, lst(L_VP8), cnt(L_VP8));
  }
  // their alpha planes, after the VP8L kernels have decoded the VP8L-coded ones
  if (!from_fix && b.any_alph) launch_alph_plane(sl.st, dm, lst(L_ALPH), cnt(L_ALPH));
  if (next()) return DG_ERR_DEVICE;
  if (!from_fix && b.any_gif) launch_gif_expand(sl.st, dm, lst(L_GIF_EXPAND), cnt(L_GIF_EXPAND));
  if (!from_fix && b.any_bmp) launch_bmp_expand(sl.st, dm, lst(L_BMP_EXPAND), cnt(L_BMP_EXPAND));
  if (!from_fix && b.any_webp) launch_vp8l_store(sl.st, dm, lst(L_VP8L_STORE), cnt(L_VP8L_STORE));
  if (!from_fix && b.any_vp8) launch_vp8_rgb(sl.st, dm, lst(L_VP8_RGB), cnt(L_VP8_RGB));
  if (!from_fix && b.any_png) {
    if (b.uf_n) {
      uint32_t *uf = (uint32_t *)((char *)sl.scratch.p + b.uf_flags_off);
      HIPCHK(hipMemsetAsync(uf, 0, (size_t)(b.uf_n + 1) * 4, sl.st));
      launch_png_unfilter(sl.st, dm, lst(L_UNF), cnt(L_UNF), uf, ncu_, b.uf_maxbpp, (uint32_t)(opt_.debug_flags >> 18) & 1u,
                          opt_.uf_units, (uint32_t)opt_.uf_per_cu);
    }
    launch_png_expand(sl.st, dd, lst(L_EXPAND), cnt(L_EXPAND));
    launch_png_expand16(sl.st, dd, lst(L_EXPAND16), cnt(L_EXPAND16));
  }
  if (next()) return DG_ERR_DEVICE;
  if (!from_fix) {
    // Lanczos coefficient tables depend only on the plan: compute them on a
    // side stream, overlapped with the entropy decode.
    hipStream_t cs = opt_.side_stream ? sl.side : sl.st;
    HIPCHK(hipEventRecord(sl.ev_meta, sl.st));
    HIPCHK(hipStreamWaitEvent(cs, sl.ev_meta, 0));

    launch_coeffs(cs, dm, lst(L_COEF), cnt(L_COEF));
    HIPCHK(hipEventRecord(sl.ev_coef, cs));
    if (b.ds_state_off) {  // one pass, decoupled look-back (option "destuff_one")
      uint64_t *dst = (uint64_t *)((char *)sl.scratch.p + b.ds_state_off);
      HIPCHK(hipMemsetAsync(dst, 0, (size_t)(b.ds_n + 1) * 8, sl.st));
      launch_destuff_one(sl.st, dm, lst(L_DESTUFF), cnt(L_DESTUFF), dst);
    } else {
      launch_destuff_count(sl.st, dd, lst(L_DESTUFF_WG), cnt(L_DESTUFF_WG));
      launch_destuff_scan(sl.st, dm, lst(L_SCAN), cnt(L_SCAN));
      launch_destuff_write(sl.st, dd, lst(L_DESTUFF_WG), cnt(L_DESTUFF_WG));
    }
  }
  if (next()) return DG_ERR_DEVICE;
  // progressive JPEG: zero, then the scans (one pipelined launch, or level by
  // level).  On the side stream, beside the baseline images' entropy decode
  // (the main stream waits for it before the IDCT), except with stage timing
  // on, where every stage runs on the main stream so its events bracket it.
  const bool pside = opt_.side_stream && opt_.prog_side && !opt_.timing && !b.pscans.empty();
  bool dc_side = false;  // DC items on the side stream, AC items on the main one
  if (!from_fix && !b.pscans.empty()) {
    hipStream_t pst = pside ? sl.side : sl.st;
    launch_prog_zero(pst, dd, lst(L_PROG_ZERO), cnt(L_PROG_ZERO));
    const ProgScan *ps = (const ProgScan *)(M + b.pscan_off);
    const uint32_t prog_dbg = ((uint32_t)(opt_.debug_flags >> 19) & 1u) << 1;  // forced wait timeouts (tests)
    uint64_t *pt = b.ptime_off ? (uint64_t *)((char *)sl.wgt.p + b.ptime_off) : nullptr;
    if (opt_.prog_pipe) {
      // AC items (one Huffman table in LDS) and DC items (four) in launches of
      // their own; no scan of one waits on a scan of the other
      uint32_t *pf = (uint32_t *)((char *)sl.scratch.p + b.pf_off);
      HIPCHK(hipMemsetAsync(pf, 0, (size_t)(b.pf_n + 2) * 4, pst));
      const uint32_t nac = cnt(L_PROG) - b.prog_dc_n, sflags = (opt_.prog_serial ? 1u : 0u) | prog_dbg;
      hipStream_t dst = pst;
      if (!pside && opt_.side_stream && b.prog_dc_n && nac) {  // DC items beside the AC launch (also when timing:
                                                          // the IDCT stage then holds what the DC items outlast)
        HIPCHK(hipEventRecord(sl.ev_zero, pst));
        HIPCHK(hipStreamWaitEvent(sl.side, sl.ev_zero, 0));
        dst = sl.side;
        dc_side = true;
      }
      launch_prog_scan(pst, dd, ps, lst(L_PROG), nac, hp, sflags, pf, pf, pt, 1);
      launch_prog_scan(dst, dd, ps, lst(L_PROG) + nac, b.prog_dc_n, hp, sflags, pf, pf + b.pf_n + 1, pt, 4);
      if (dc_side) HIPCHK(hipEventRecord(sl.ev_prog, sl.side));
    } else {
      uint32_t at = 0;
      for (uint32_t nl : b.prog_level_n) {
        launch_prog_scan(pst, dd, ps, lst(L_PROG) + at, nl, hp, opt_.prog_serial ? 1u : 0u, nullptr, nullptr, pt, 4);
        at += nl;
      }
    }
    if (pside) HIPCHK(hipEventRecord(sl.ev_prog, sl.side));
  }
  if (next()) return DG_ERR_DEVICE;
  Ckpt *ck = (Ckpt *)((char *)sl.scratch.p + sl.ckpt_off);
  if (!from_fix)
    launch_huff_sync(sl.st, dd, lst(L_SYNC), cnt(L_SYNC), hp, subs, ck, fl, b.stage_on, b.max_slots,
                     opt_.multi_lead ? b.max_ac : 0u, opt_.sync_pair, opt_.sync2, (uint32_t)opt_.sync_chain, b.nc4);
  if (next()) return DG_ERR_DEVICE;
  launch_huff_fix(sl.st, dd, lst(L_SYNC), cnt(L_SYNC), hp, subs, ck, fl, b.stage_on, b.max_slots, b.nc4);
  if (next()) return DG_ERR_DEVICE;
  launch_huff_scan(sl.st, dm, lst(L_SCAN), cnt(L_SCAN), subs, b.nc4);
  if (next()) return DG_ERR_DEVICE;
  // multiscan parents: every padding block cleared, in front of the write pass on the same stream, which
  // stores over those an interleaved scan codes
  launch_ms_zero(sl.st, dd, lst(L_MS_ZERO), cnt(L_MS_ZERO));
  if (b.stage_on)
    launch_huff_scatter(sl.st, dd, lst(L_HUFF), cnt(L_HUFF), subs);
  else
    launch_huff_write(sl.st, dm, lst(L_HUFF), cnt(L_HUFF), hp, subs, fl, b.max_slots, qp, (uint32_t)opt_.write_pair, ck,
                      b.nc4, b.ms);
  if (next()) return DG_ERR_DEVICE;
  if (next()) return DG_ERR_DEVICE;  // coeffs (side stream)
  if (pside || dc_side) HIPCHK(hipStreamWaitEvent(sl.st, sl.ev_prog, 0));  // progressive coefficients
  if (b.any_fused) launch_idct_list(sl.st, dd, qp, fl, std::min<uint32_t>(2048u, (b.idct_cap + 31) / 32));
  if (opt_.idct_thread)
    launch_idct_t(sl.st, dd, lst(L_IDCT), cnt(L_IDCT), qp);
  else
    launch_idct(sl.st, dd, lst(L_IDCT), cnt(L_IDCT), qp);
  if (next()) return DG_ERR_DEVICE;
  launch_color(sl.st, dd, lst(L_COLOR), cnt(L_COLOR));
  launch_cmyk(sl.st, dd, lst(L_CMYK), cnt(L_CMYK));
  if (next()) return DG_ERR_DEVICE;
  HIPCHK(hipStreamWaitEvent(sl.st, sl.ev_coef, 0));
  launch_alpha(sl.st, dd, lst(L_ALPHA0), cnt(L_ALPHA0), 0 | (alpha_flags << 8));
  launch_band_dec(sl.st, dd, lst(L_DEC), b.decclass, qp, opt_.dec_strips | (opt_.dec_dbg << 16));
  launch_resize_hm(sl.st, dd, lst(L_RM0), b.hmclass[0], 0);
  launch_resize_hb(sl.st, dd, lst(L_RH0), b.hclass[0], 0, opt_.h_prefetch, opt_.h_planar, b.h_zune != 0);
  launch_resize_hv(sl.st, dd, lst(L_RHV), b.hvclass);
  launch_resize_h(sl.st, dd, lst(L_RHX0), cnt(L_RHX0), 0 | ((opt_.debug_flags & 0xFF) << 8));
  if (!from_fix) launch_r16_v(sl.st, dd, lst(L_R16V), cnt(L_R16V));  // (PNG only: nothing a resync round redoes)
  if (next()) return DG_ERR_DEVICE;
  launch_resize_v(sl.st, dd, lst(L_RV1), cnt(L_RV1), 1, opt_.v_units);
  launch_resize_vt(sl.st, dd, lst(L_RVT1), cnt(L_RVT1), 1, b.v_tile);
  if (!from_fix) launch_r16_h(sl.st, dd, lst(L_R16H), cnt(L_R16H));
  launch_alpha(sl.st, dd, lst(L_ALPHA1), cnt(L_ALPHA1), 1 | (alpha_flags << 8));
  if (next()) return DG_ERR_DEVICE;
  launch_resize_hm(sl.st, dd, lst(L_RM2), b.hmclass[1], 2);
  launch_resize_hb(sl.st, dd, lst(L_RH2), b.hclass[1], 2, opt_.h_prefetch, opt_.h_planar, b.h_zune != 0);
  launch_resize_h(sl.st, dd, lst(L_RHX2), cnt(L_RHX2), 2 | ((opt_.debug_flags & 0xFF) << 8));
  if (next()) return DG_ERR_DEVICE;
  launch_resize_v(sl.st, dd, lst(L_RV3), cnt(L_RV3), 3, opt_.v_units);
  launch_resize_vt(sl.st, dd, lst(L_RVT3), cnt(L_RVT3), 3, b.v_tile);
  launch_alpha(sl.st, dd, lst(L_ALPHA2), cnt(L_ALPHA2), 2 | (alpha_flags << 8));
  if (next()) return DG_ERR_DEVICE;
  launch_copy(sl.st, dd, lst(L_COPY), cnt(L_COPY));
  if (next()) return DG_ERR_DEVICE;
  if (b.any_enc) {
    HIPCHK(hipMemsetAsync((char *)sl.scratch.p + b.words_off, 0, b.words_bytes, sl.st));
    launch_enc_fdct(sl.st, dd, lst(L_ENC_MCU), cnt(L_ENC_MCU));
    if (b.jenc_opt) {  // per-image Huffman tables: count, write and stuff then go by the image's own
      launch_enc_hist(sl.st, dd, lst(L_ENC_BLK), cnt(L_ENC_BLK));
      launch_enc_tree(sl.st, dm, lst(L_ENC_IMG), cnt(L_ENC_IMG));
    }
    launch_enc_count(sl.st, dd, lst(L_ENC_BLK), cnt(L_ENC_BLK));
    launch_penc_filter(sl.st, dd, lst(L_PENC_ROW), cnt(L_PENC_ROW));
    launch_penc_filter16(sl.st, dd, lst(L_PENC_ROW16), cnt(L_PENC_ROW16));
    launch_penc_count(sl.st, dd, lst(L_PENC_PIECE), cnt(L_PENC_PIECE), b.penc_dyn);
    if (b.penc_dyn) {  // per-image codes and the block choice, then the chosen images' pieces under their codes
      launch_penc_tree(sl.st, dm, lst(L_PENC_IMG), cnt(L_PENC_IMG));
      launch_penc_count_dyn(sl.st, dd, lst(L_PENC_PIECE), cnt(L_PENC_PIECE));
    }
    launch_enc_scan(sl.st, dm, lst(L_ENC_IMG), cnt(L_ENC_IMG));
    launch_enc_write(sl.st, dd, lst(L_ENC_BLK), cnt(L_ENC_BLK));
    launch_penc_write(sl.st, dd, lst(L_PENC_PIECE), cnt(L_PENC_PIECE), b.penc_dyn);
    launch_enc_stuff(sl.st, dm, lst(L_ENC_IMG), cnt(L_ENC_IMG));
    launch_penc_final(sl.st, dm, lst(L_PENC_IMG), cnt(L_PENC_IMG));
  }
  if (next()) return DG_ERR_DEVICE;
  HIPCHK(hipGetLastError());
  // read back flags + per-image status (descs) for finish(), then outputs (host path)
  size_t back = b.desc_off + b.descs.size() * sizeof(ImageDesc);
  size_t total = align_up(back, 256);
  if (b.host_io)
    for (int i = 0; i < b.n; i++)
      if (b.desc_of[i] >= 0 && !b.plans[i].encode && !b.out_direct[i]) total += align_up(b.plans[i].out_bytes, 16);
  dg_status st = ensure_pinned(sl.out, total + 256, sl.st);
  if (st) return st;
  HIPCHK(hipMemcpyAsync(sl.out.p, M, back, hipMemcpyDeviceToHost, sl.st));
  if (b.host_io) {
    size_t off = align_up(back, 256);
    for (int i = 0; i < b.n; i++) {
      if (b.desc_of[i] < 0 || b.plans[i].encode) continue;  // encoded: exact size copied in finish()
      if (b.out_direct[i]) {  // DMA straight into the caller's page-locked buffer
        HIPCHK(hipMemcpyAsync(b.host_outs[i], (char *)sl.scratch.p + b.out_dev_off[i], b.plans[i].out_bytes,
                              hipMemcpyDeviceToHost, sl.st));
        continue;
      }
      HIPCHK(hipMemcpyAsync((char *)sl.out.p + off, (char *)sl.scratch.p + b.out_dev_off[i], b.plans[i].out_bytes,
                            hipMemcpyDeviceToHost, sl.st));
      off += align_up(b.plans[i].out_bytes, 16);
    }
  }
  if (next()) return DG_ERR_DEVICE;  // download
  HIPCHK(hipEventRecord(sl.done, sl.st));
  HIPCHK(hipEventRecord(b.fin->e, sl.st));
  return DG_OK;
}

// A batch that cannot complete (a launch, resync or copy-back failure): no
// kernel of it is left running, every image not already failed reads `st`,
// deferred metas are published, and the batch counts as done -- a later
// submit on the slot must not finish() it again and publish planning-time
// metas over the error.
void Context::fail_batch(Slot &sl, dg_status st) {
  if (!sl.batch || sl.batch->done) return;
  for (hipStream_t q : {sl.st, sl.side})
    if (q) (void)hipStreamSynchronize(q);
  (void)hipGetLastError();
  Batch &b = *sl.batch;
  for (int i = 0; i < b.n && i < (int)b.mptr.size(); i++)
    if (b.mptr[i] && b.mptr[i]->status == DG_OK) b.mptr[i]->status = st;
  for (size_t i = 0; i < b.pub.size(); i++) *b.pub[i] = b.local_meta[i];
  // Lanczos tables this batch was producing never become ready: retire their
  // keys (the index slot stays as a tombstone, probes pass it) so that a later
  // batch produces them again instead of recomputing its own copy every time
  // until the arena starts over
  for (const Batch::CProd &pr : b.ccache_prod)
    if (pr.entry < (int)ccache_.size() && !ccache_[pr.entry].ready) {
      ccache_[pr.entry].key.ksize = 0xFFFFFFFFu;
      ccache_[pr.entry].key.in_size = 0;
    }
  b.done = true;
}

dg_status Context::finish(Slot &sl) {
  const dg_status st = finish_body(sl);
  if (st) fail_batch(sl, st);
  return st;
}

dg_status Context::finish_body(Slot &sl) {
  Batch &b = *sl.batch;
  for (;;) {
    HIPCHK(hipEventSynchronize(sl.done));
    memcpy(&b.flags, (char *)sl.out.p + b.flags_off, sizeof(BatchFlags));
    stat_fix_ += b.flags.fix_count;
    stat_mismatch_ += b.flags.write_mismatch;
    stat_iters_ = std::max<int64_t>(stat_iters_, b.flags.sync_iters_max);
    if (b.flags.idct_late > b.idct_cap) {  // never seen; would leave blocks without pixels
      b.unsettled = true;
      set_error("fused IDCT list overflow: the batch's JPEGs are returned DG_ERR_UNSUPPORTED");
    }
    if (b.flags.chain_changed == 0) break;
    if (b.resync_rounds >= kMaxResyncRounds) {
      // The boundary repair did not settle: some entropy chain of this batch
      // may be wrong, and nothing tells which image it belongs to.  Every
      // sequential JPEG not already failed goes back to the caller's CPU
      // decoder (DG_ERR_UNSUPPORTED) instead of returning pixels that may
      // be wrong.
      stat_unsettled_++;
      b.unsettled = true;
      set_error("entropy resync did not converge: the batch's JPEGs are returned DG_ERR_UNSUPPORTED");
      break;
    }
    // a workgroup's last exit state changed during the boundary repair: repeat
    // repair + everything downstream until the chain is stable
    b.resync_rounds++;
    stat_resync_++;
    dg_status st = launch_all(sl, true);
    if (st) return st;
  }
  if (b.ptime_off) {  // debug: one line per progressive scan (option wg_timing, env DG_PROG_DUMP)
    std::vector<uint64_t> rec(2 * b.pscans.size());
    HIPCHK(hipMemcpy(rec.data(), (char *)sl.wgt.p + b.ptime_off, rec.size() * 8, hipMemcpyDeviceToHost));
    if (const char *dump = getenv("DG_PROG_DUMP")) {
      if (FILE *f = fopen(dump, "a")) {
        uint64_t lo = ~0ull;
        for (size_t i = 0; i < b.pscans.size(); i++) lo = std::min(lo, rec[2 * i]);
        for (size_t i = 0; i < b.pscans.size(); i++) {
          const ProgScan &sc = b.pscans[i];
          const ImageDesc &d = b.descs[sc.image];
          fprintf(f, "%zu %u %u %u %u %u %u %u %u %u %u %llu %llu %u %u\n", i, sc.image, sc.ns, sc.comp[0], sc.ss, sc.se,
                  sc.ah, sc.al, sc.len, sc.level, (uint32_t)sc.pflags, (unsigned long long)(rec[2 * i] - lo),
                  (unsigned long long)(rec[2 * i + 1] - lo), d.total_blocks, d.width * d.height);
        }
        fprintf(f, "end\n");
        fclose(f);
      }
    }
  }
  if (b.flags.wgtime) {
    const size_t ns = b.lists[L_SYNC].size(), nw = b.lists[L_HUFF].size();
    std::vector<uint64_t> rec(2 * (ns + nw));
    HIPCHK(hipMemcpy(rec.data(), sl.wgt.p, rec.size() * 8, hipMemcpyDeviceToHost));
    if (const char *dump = getenv("DG_WG_DUMP")) {  // debug: one line per entropy workgroup
      if (FILE *f = fopen(dump, "a")) {
        uint64_t lo = ~0ull;
        for (size_t i = 0; i < ns + nw; i++) lo = std::min(lo, rec[2 * i]);
        for (size_t i = 0; i < ns + nw; i++) {
          const WgItem &w = b.lists[i < ns ? L_SYNC : L_HUFF][i < ns ? i : i - ns];
          const ImageDesc &d = b.descs[w.image];
          fprintf(f, "%d %zu %u %u %llu %llu %u %u %u %u %u %u\n", i < ns ? 0 : 1, i, w.image, w.item0,
                  (unsigned long long)(rec[2 * i] - lo), (unsigned long long)(rec[2 * i + 1] - lo), d.scan_len,
                  d.total_blocks, d.sub_bits, d.nsub, d.lead_bits, d.width * d.height);
        }
        fprintf(f, "end\n");
        fclose(f);
      }
    }
    for (int a = 0; a < 2; a++) {
      const size_t r0 = a ? ns : 0, n = a ? nw : ns;
      if (!n) continue;
      uint64_t lo = ~0ull, hi = 0;
      std::vector<double> d(n);
      double sum = 0;
      for (size_t i = 0; i < n; i++) {
        const uint64_t t0 = rec[2 * (r0 + i)], t1 = rec[2 * (r0 + i) + 1];
        lo = std::min(lo, t0);
        hi = std::max(hi, t1);
        d[i] = (double)(t1 - t0) * 0.01;  // 100 MHz ticks -> us
        sum += d[i];
      }
      std::sort(d.begin(), d.end());
      wgstat_[a][0] = (double)(hi - lo) * 0.01;
      wgstat_[a][1] = sum / (double)n;
      wgstat_[a][2] = d[(size_t)(0.9 * (double)(n - 1))];
      wgstat_[a][3] = d.back();
    }
  }
  if (opt_.timing) {
    last_ms_.assign(kNumStages, 0.f);
    for (int i = 0; i < kNumStages; i++) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, sl.ev[i], sl.ev[i + 1]) == hipSuccess) last_ms_[i] = ms;
    }
  }
  const ImageDesc *back = (const ImageDesc *)((char *)sl.out.p + b.desc_off);
  size_t off = align_up(b.desc_off + b.descs.size() * sizeof(ImageDesc), 256);
  if (b.host_io && b.any_enc) {
    // Re-encoded payloads are known in length only now: copy all of them
    // with one async D2H each into pinned staging behind the raw outputs and
    // wait once, instead of a synchronous hipMemcpy per image.
    size_t enc_total = 0;
    for (int i = 0; i < b.n; i++)
      if (b.desc_of[i] >= 0 && b.plans[i].encode && !back[b.desc_of[i]].status)
        enc_total += align_up(back[b.desc_of[i]].enc.enc_bytes, 16);
    if (enc_total) {
      size_t raw_end = off;
      for (int i = 0; i < b.n; i++)
        if (b.desc_of[i] >= 0 && !b.plans[i].encode) raw_end += align_up(b.plans[i].out_bytes, 16);
      if (sl.out.cap < raw_end + enc_total) {  // grow keeping the read-back descriptors and raw outputs
        std::vector<char> keep((char *)sl.out.p, (char *)sl.out.p + raw_end);
        dg_status st = ensure_pinned(sl.out, raw_end + enc_total + 256, sl.st);
        if (st) return st;
        memcpy(sl.out.p, keep.data(), keep.size());
        back = (const ImageDesc *)((char *)sl.out.p + b.desc_off);
      }
      size_t eo = raw_end;
      for (int i = 0; i < b.n; i++) {
        if (b.desc_of[i] < 0 || !b.plans[i].encode || back[b.desc_of[i]].status) continue;
        const uint32_t nb = back[b.desc_of[i]].enc.enc_bytes;
        HIPCHK(hipMemcpyAsync((char *)sl.out.p + eo, (char *)sl.scratch.p + b.out_dev_off[i], nb,
                              hipMemcpyDeviceToHost, sl.st));
        b.enc_host_off.resize(b.n, 0);
        b.enc_host_off[i] = eo;
        eo += align_up(nb, 16);
      }
      HIPCHK(hipStreamSynchronize(sl.st));
    }
  }
  for (const Batch::CProd &pr : b.ccache_prod) {  // tables this batch wrote into the cache: hits from now on
    if (pr.entry >= (int)ccache_.size()) continue;
    CEntry &e = ccache_[pr.entry];
    e.precision = back[pr.desc].pass[pr.stage].precision;
    e.ready = e.precision > 0;
  }
  std::vector<CopyJob> copies;
  for (int i = 0; i < b.n; i++) {
    if (b.desc_of[i] < 0) continue;
    int status = back[b.desc_of[i]].status;
    // a multiscan image takes its scan descriptors' status (truncated data, a write mismatch): corrupt first
    if (back[b.desc_of[i]].ms.role == kMsParent)
      for (const Batch::MsScan &ms : b.ms_scans)
        if (ms.parent == b.desc_of[i] && back[ms.desc].status > status) status = back[ms.desc].status;
    if (back[b.desc_of[i]].fmt == kFmtPng && back[b.desc_of[i]].png.nchunks) {
      stat_png_chunks_ += back[b.desc_of[i]].png.nchunks;
      stat_png_serial_ += back[b.desc_of[i]].png.serial ? 1 : 0;
    } else if (back[b.desc_of[i]].fmt == kFmtPng) {
      stat_png_small_++;
    }
    if (!status && b.unsettled && b.plans[i].fmt == kFmtJpeg && !b.plans[i].hdr.progressive)
      status = DG_ERR_UNSUPPORTED;
    if (status && back[b.desc_of[i]].fmt == kFmtGif) {  // what k_gif_lzw / k_gif_expand met in the stream
      const uint32_t f = back[b.desc_of[i]].gif.fail;
      set_error(f == kGifFailCode    ? "GIF: LZW code above the next free code"
                : f == kGifFailShort ? "GIF: image data ends before the frame is complete"
                : f == kGifFailPalette ? "GIF: pixel index past the colour table"
                                       : "GIF: decode failed");
    }
    if (status && back[b.desc_of[i]].fmt == kFmtBmp) {  // what k_bmp_rle / k_bmp_expand met in the stream
      const uint32_t f = back[b.desc_of[i]].bmp.fail;
      set_error(f == kBmpFailRow       ? "BMP: RLE run or absolute block passes its row's end"
                : f == kBmpFailDelta   ? "BMP: RLE delta, early end-of-line or end-of-bitmap leaves pixels unwritten"
                : f == kBmpFailShort   ? "BMP: RLE data ends before the bitmap is complete"
                : f == kBmpFailPalette ? "BMP: pixel index past the colour table"
                                       : "BMP: decode failed");
    }
    if (status && back[b.desc_of[i]].fmt == kFmtWebp) {  // what k_vp8l_decode met in the stream
      const uint32_t f = back[b.desc_of[i]].vp8l.fail;
      set_error(f == kVp8lFailBits        ? "WebP: image data ends before the image is complete"
                : f == kVp8lFailCode      ? "WebP: prefix code neither complete nor single-symbol"
                : f == kVp8lFailCopy      ? "WebP: copy reaches before the first or past the last pixel"
                : f == kVp8lFailCache     ? "WebP: colour-cache index or size outside the format"
                : f == kVp8lFailTransform ? "WebP: transform used twice"
                : f == kVp8lFailGroups    ? "WebP: more prefix-code groups than the GPU path holds"
                                          : "WebP: decode failed");
    }
    if (back[b.desc_of[i]].fmt == kFmtVp8 && !back[b.desc_of[i]].vp8.fail)  // a failed alpha stream fails its image
      for (const Batch::AlphStream &as : b.alph_streams)
        if (as.parent == b.desc_of[i] && back[as.desc].status > status) status = back[as.desc].status;
    if (status && back[b.desc_of[i]].fmt == kFmtVp8) {  // what k_vp8_parse met in the stream, or k_vp8l_decode in the alpha's
      const uint32_t f = back[b.desc_of[i]].vp8.fail;
      set_error(f == kVp8FailBits    ? "WebP: VP8 data ends before the image is complete"
                : f == kVp8FailParts ? "WebP: VP8 token-partition table reaches past the chunk"
                : status == DG_ERR_UNSUPPORTED ? "WebP: ALPH stream with more prefix-code groups than the GPU path holds"
                                               : "WebP: ALPH lossless stream does not decode");
    }
    if (status) b.mptr[i]->status = status;
    if (b.plans[i].encode) {
      const uint32_t nb = back[b.desc_of[i]].enc.enc_bytes;
      b.mptr[i]->nbytes = nb;
      if (b.host_io && !status && nb) copies.push_back({b.host_outs[i], (char *)sl.out.p + b.enc_host_off[i], nb});
      continue;
    }
    if (b.host_io && b.out_direct[i]) {
      stat_direct_d2h_++;
    } else if (b.host_io) {
      if (!status) copies.push_back({b.host_outs[i], (char *)sl.out.p + off, b.plans[i].out_bytes});
      off += align_up(b.plans[i].out_bytes, 16);
    }
  }
  parallel_copy(copies, opt_.copy_threads);
  for (size_t i = 0; i < b.pub.size(); i++) *b.pub[i] = b.local_meta[i];  // defer_meta: publish now
  b.done = true;
  return DG_OK;
}

Slot *Context::find(uint64_t ticket) {
  for (Slot &sl : slots_)
    if (sl.batch && sl.batch->ticket == ticket) return &sl;
  return nullptr;
}

dg_status Context::wait(uint64_t ticket) {
  std::shared_ptr<BatchEvent> fin;
  {
    std::lock_guard<std::mutex> lk(mu_);
    HIPCHK(hipSetDevice(device_));
    Slot *sl = find(ticket);
    if (!sl) return ticket < next_ticket_ ? DG_OK : DG_ERR_INVALID;  // already recycled => completed
    if (sl->batch->done) return DG_OK;
    fin = sl->batch->fin;
  }
  // block on the GPU without holding the context lock, so other threads can
  // plan and submit meanwhile (the batch's own event: if the slot is
  // recycled first, the ticket then reads as completed)
  HIPCHK(hipEventSynchronize(fin->e));
  std::lock_guard<std::mutex> lk(mu_);
  Slot *sl = find(ticket);
  if (!sl) return ticket < next_ticket_ ? DG_OK : DG_ERR_INVALID;
  if (sl->batch->done) return DG_OK;
  const dg_status st = finish(*sl);
  if (!st) free_retired_if_idle();
  return st;
}

dg_status Context::flush_batch(std::vector<OneReq *> &batch, bool prog) {
  const int n = (int)batch.size();
  std::vector<const uint8_t *> srcs(n);
  std::vector<size_t> lens(n);
  std::vector<int32_t> forced(n);
  std::vector<uint8_t *> outs(n);
  std::vector<uint64_t> caps(n);
  std::vector<dg_payload_meta> metas(n);
  for (int i = 0; i < n; i++) {
    srcs[i] = batch[i]->src;
    lens[i] = batch[i]->len;
    forced[i] = batch[i]->forced;
    outs[i] = batch[i]->out;
    caps[i] = batch[i]->cap;
  }
  std::vector<dg_payload_meta *> mp(n);
  for (int i = 0; i < n; i++) mp[i] = &metas[i];
  std::vector<uint64_t> ts;
  dg_status st = submit_split(n, srcs.data(), nullptr, lens.data(), forced.data(), outs.data(), caps.data(), mp.data(),
                              true, ts, prog, false);
  for (uint64_t t : ts) {
    const dg_status s1 = wait(t);
    if (!st) st = s1;
  }
  for (int i = 0; i < n; i++) {
    *batch[i]->meta = metas[i];
    batch[i]->st = st ? st : (dg_status)metas[i].status;
  }
  return st;
}

dg_status Context::decode_one(const uint8_t *src, size_t len, int32_t forced, uint8_t *out, uint64_t cap,
                              dg_payload_meta *meta) {
  OneReq r{src, len, forced, out, cap, meta, false, DG_OK, false};
  if (opt_.coalesce_max <= 1) {
    std::vector<OneReq *> one{&r};
    flush_batch(one, false);
    return r.st;
  }
  // Progressive JPEGs decode their scans serially (one wave per scan, ~0.1-1 s
  // for a large file), so they coalesce into batches of their own: a
  // baseline caller never waits behind a progressive chain, and up to
  // prog_lanes progressive batches run beside the baseline ones.
  r.prog = opt_.progressive && opt_.prog_lanes > 0 && jpeg_sniff_progressive(src, len);
  std::unique_lock<std::mutex> lk(cmu_);
  callers_++;
  std::vector<OneReq *> &q = r.prog ? ppending_ : pending_;
  q.push_back(&r);
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(opt_.coalesce_us);
  for (;;) {
    if (r.done) break;
    // flush when the batch is full, when every caller in here is already
    // waiting (nobody else can add), or at the deadline; nslots baseline
    // batches (+ prog_lanes progressive ones) in flight at most
    const int waiting = callers_ - inflight_reqs_;
    const bool ready = !q.empty() && ((int)q.size() >= opt_.coalesce_max ||
                                      (int)(pending_.size() + ppending_.size()) >= waiting ||
                                      std::chrono::steady_clock::now() >= deadline);
    const bool room = r.prog ? pinflight_ < opt_.prog_lanes : inflight_ < (opt_.coalesce_inflight ? opt_.coalesce_inflight : opt_.nslots);
    if (ready && room && std::find(q.begin(), q.end(), &r) != q.end()) {
      std::vector<OneReq *> batch;
      const size_t take = std::min(q.size(), (size_t)opt_.coalesce_max);
      batch.assign(q.begin(), q.begin() + take);
      q.erase(q.begin(), q.begin() + take);
      (r.prog ? pinflight_ : inflight_)++;
      inflight_reqs_ += (int)batch.size();
      stat_coalesced_batches_++;
      stat_coalesced_images_ += (int64_t)batch.size();
      lk.unlock();
      flush_batch(batch, r.prog);
      lk.lock();
      for (OneReq *x : batch) x->done = true;
      (r.prog ? pinflight_ : inflight_)--;
      inflight_reqs_ -= (int)batch.size();
      ccv_.notify_all();
      continue;
    }
    if (ready)
      ccv_.wait(lk);
    else
      ccv_.wait_until(lk, deadline);
  }
  callers_--;
  ccv_.notify_all();
  return r.st;
}

dg_status Context::poll(uint64_t ticket) {
  std::lock_guard<std::mutex> lk(mu_);
  Slot *sl = find(ticket);
  if (!sl || sl->batch->done) return DG_OK;
  hipError_t e = hipEventQuery(sl->done);
  if (e == hipErrorNotReady) return DG_ERR_NOT_READY;
  return DG_OK;
}

// ---- progressive split (dg_submit / dg_submit_device / dg_wait / dg_poll / dg_wait_ready)
//
// A refinement scan is one serial chain (dg_prog.hip): a large progressive
// file takes ~0.1-1 s, and a batch lasts as long as its longest chain.  So a
// submission with progressive members is split: its other members run as a
// batch of their own (back at the baseline pace), and its progressive members
// join the open progressive aggregate, which is submitted as one batch on a
// progressive slot once it holds prog_batch images, once it is older than
// prog_flush_us at a submit / poll / wait_ready, or as soon as a caller blocks
// on one of its members (dg_wait).  An aggregate of ~1024 files keeps
// thousands of scan chains in flight at once, where a 256-image batch with a
// few progressive members idles the GPU behind one chain.  dg_wait(ticket)
// completes both parts (the ABI's contract is unchanged); dg_wait_ready
// returns once the non-progressive part is done and leaves the progressive
// members' metas at DG_ERR_NOT_READY until a later dg_wait(ticket).

// Launch the open aggregate early (before prog_batch images) only when it is
// older than prog_flush_us AND a progressive slot is idle: while both run,
// the aggregate keeps growing (a larger launch hides more of its long pole).
bool Context::pagg_stale_locked() {
  if (pagg_.empty() || std::chrono::steady_clock::now() - pagg_t0_ < std::chrono::microseconds(opt_.prog_flush_us))
    return false;
  std::lock_guard<std::mutex> lk(mu_);
  for (int j = 0; j < kProgSlots; j++) {
    const Slot &sl = slots_[kMaxInflight + j];
    if (!sl.batch || sl.batch->done || hipEventQuery(sl.done) == hipSuccess) return true;
  }
  return false;
}

dg_status Context::submit_split(int n, const uint8_t *const *h_srcs, const uint8_t *const *d_srcs,
                                const size_t *lens, const int32_t *forced, uint8_t *const *outs,
                                const uint64_t *caps, dg_payload_meta *const *mptrs, bool host_io,
                                std::vector<uint64_t> &tickets, bool prog, bool defer_meta, bool whole_failed) {
  if (n <= 0) return DG_OK;
  int slot = -1;
  if (prog) {
    std::lock_guard<std::mutex> lk(mu_);
    slot = pick_prog_slot();
  }
  dg_status st = kNeedSplit;
  if (!whole_failed) {  // (the caller already planned the whole submission and saw kNeedSplit)
    uint64_t t = 0;
    st = submit(n, h_srcs, d_srcs, lens, forced, outs, caps, nullptr, host_io, &t, mptrs, slot, defer_meta);
    if (st != kNeedSplit) {
      if (!st) tickets.push_back(t);
      return st;
    }
  }
  if (n == 1) {  // one image larger than the device budget: that sample fails, not the worker
    dg_payload_meta &m = *mptrs[0];
    memset(&m, 0, sizeof(m));
    m.status = DG_ERR_OOM;
    m.bucket = -1;
    stat_budget_oom_++;
    set_error("image does not fit the device memory budget (max_device_mb)");
    return DG_OK;
  }
  stat_budget_splits_++;
  const int h = n / 2;
  st = submit_split(h, h_srcs, d_srcs, lens, forced, outs, caps, mptrs, host_io, tickets, prog, defer_meta);
  if (st) return st;
  if (opt_.debug_flags & (1 << 24)) {  // test switch: the second part fails after the first launched
    set_error("forced failure of a split submission's second part (debug_flags bit 24)");
    return DG_ERR_DEVICE;
  }
  return submit_split(n - h, h_srcs + h, d_srcs ? d_srcs + h : nullptr, lens + h, forced ? forced + h : nullptr,
                      outs + h, caps + h, mptrs + h, host_io, tickets, prog, defer_meta);
}

dg_status Context::flush_pagg_locked() {
  if (pagg_.empty()) return DG_OK;
  const int n = (int)pagg_.size();
  std::vector<const uint8_t *> h(n), d(n);
  std::vector<size_t> lens(n);
  std::vector<int32_t> forced(n);
  std::vector<uint8_t *> outs(n);
  std::vector<uint64_t> caps(n);
  std::vector<dg_payload_meta *> mp(n);
  for (int i = 0; i < n; i++) {
    const PEntry &e = pagg_[i];
    h[i] = e.host.data();
    d[i] = e.dsrc;
    lens[i] = e.len;
    forced[i] = e.forced;
    outs[i] = e.out;
    caps[i] = e.cap;
    mp[i] = e.meta;
  }
  std::vector<uint64_t> ts;
  dg_status st = submit_split(n, h.data(), pagg_host_ ? nullptr : d.data(), lens.data(), forced.data(), outs.data(),
                              caps.data(), mp.data(), pagg_host_, ts, true, true);
  if (st) {  // the members of parts that did not launch fail now; dg_wait on their tickets returns st
    for (PEntry &e : pagg_)
      if (e.meta->status == DG_ERR_NOT_READY) e.meta->status = st;
  }
  stat_prog_aggs_++;
  stat_prog_agg_images_ += n;
  pgen_[pagg_gen_] = PGen{ts, pagg_refs_, st};
  pagg_refs_ = 0;
  pagg_gen_++;
  pagg_.clear();
  return st;
}

// A split submission failed part-way: the parts that launched
// before the failure still write into the caller's outputs (and a host-out
// part copies to them at its finish), so they complete before the error is
// returned -- the caller may free its buffers as soon as this call fails.
dg_status Context::fail_split_parts(const std::vector<uint64_t> &launched, dg_status st) {
  const std::string why = g_last_error;
  for (uint64_t t : launched) wait(t);
  set_error(why);
  return st;
}

dg_status Context::submit_user(int n, const uint8_t *const *h_srcs, const uint8_t *const *d_srcs, const size_t *lens,
                               const int32_t *forced, uint8_t *const *outs, const uint64_t *caps,
                               dg_payload_meta *metas, bool host_io, uint64_t *ticket) {
  if (!ticket) return DG_ERR_INVALID;
  std::vector<uint8_t> isp(n > 0 ? n : 0, 0);
  int np = 0;
  if (opt_.progressive && opt_.prog_split && n > 0 && h_srcs && lens && outs && caps && metas && (host_io || d_srcs))
    for (int i = 0; i < n; i++) {
      isp[i] = h_srcs[i] && jpeg_sniff_progressive(h_srcs[i], lens[i]) ? 1 : 0;
      np += isp[i];
    }
  if (!np) {
    dg_status st = submit(n, h_srcs, d_srcs, lens, forced, outs, caps, metas, host_io, ticket);
    if (st == kNeedSplit) {  // over the device budget: parts under one user ticket
      std::vector<dg_payload_meta *> mp(n);
      for (int i = 0; i < n; i++) mp[i] = &metas[i];
      SplitRec rec;
      st = submit_split(n, h_srcs, d_srcs, lens, forced, outs, caps, mp.data(), host_io, rec.tbs, false, false, true);
      if (st) return fail_split_parts(rec.tbs, st);
      std::lock_guard<std::mutex> lk(pmu_);
      {
        std::lock_guard<std::mutex> lk2(mu_);
        *ticket = next_ticket_++;
      }
      split_[*ticket] = rec;
      return DG_OK;
    }
    // a stale aggregate is launched by whoever comes by, but a baseline
    // submitter never queues behind a thread that holds the aggregate (its
    // launch may wait for a busy progressive slot)
    std::unique_lock<std::mutex> lk(pmu_, std::try_to_lock);
    if (lk.owns_lock() && pagg_stale_locked()) flush_pagg_locked();
    return st;
  }
  SplitRec rec;
  if (np < n) {  // the other members: a batch of their own
    std::vector<const uint8_t *> h, d;
    std::vector<size_t> ln;
    std::vector<int32_t> fb;
    std::vector<uint8_t *> ou;
    std::vector<uint64_t> cp;
    std::vector<dg_payload_meta *> mp;
    for (int i = 0; i < n; i++) {
      if (isp[i]) continue;
      h.push_back(h_srcs[i]);
      d.push_back(d_srcs ? d_srcs[i] : nullptr);
      ln.push_back(lens[i]);
      fb.push_back(forced ? forced[i] : -1);
      ou.push_back(outs[i]);
      cp.push_back(caps[i]);
      mp.push_back(&metas[i]);
    }
    dg_status st = submit_split((int)h.size(), h.data(), host_io ? nullptr : d.data(), ln.data(), fb.data(),
                                ou.data(), cp.data(), mp.data(), host_io, rec.tbs, false, false);
    if (st) return fail_split_parts(rec.tbs, st);
  }
  std::lock_guard<std::mutex> lk(pmu_);
  if (!pagg_.empty() && pagg_host_ != host_io) flush_pagg_locked();  // an aggregate is host- or device-fed
  if (pagg_.empty()) pagg_t0_ = std::chrono::steady_clock::now();
  pagg_host_ = host_io;
  for (int i = 0; i < n; i++) {
    if (!isp[i]) continue;
    PEntry e;
    e.host.assign(h_srcs[i], h_srcs[i] + lens[i]);  // the caller's host bytes are only valid during the call
    e.dsrc = host_io ? nullptr : d_srcs[i];
    e.len = lens[i];
    e.forced = forced ? forced[i] : -1;
    e.out = outs[i];
    e.cap = caps[i];
    e.meta = &metas[i];
    memset(e.meta, 0, sizeof(*e.meta));
    e.meta->status = DG_ERR_NOT_READY;
    e.meta->bucket = -1;
    pagg_.push_back(std::move(e));
  }
  rec.gen = pagg_gen_;
  rec.nprog = np;
  pagg_refs_++;
  {
    std::lock_guard<std::mutex> lk2(mu_);
    *ticket = next_ticket_++;  // a ticket of its own, in the batch tickets' sequence
  }
  split_[*ticket] = rec;
  // The caller's members are queued and its ticket is live.  An aggregate
  // launch started here may carry other submissions' members too: its
  // failure is recorded for their dg_wait (pgen_) and in their metas, never
  // returned from this call, whose non-progressive part is already in flight.
  if ((int)pagg_.size() >= opt_.prog_batch || pagg_stale_locked()) flush_pagg_locked();
  return DG_OK;
}

// A user ticket of a split submission: its baseline part(s) (several when
// the device budget split them) and, when gen != 0, the progressive
// aggregate holding its progressive members.
dg_status Context::wait_user(uint64_t ticket) {
  SplitRec rec;
  std::vector<uint64_t> tps;
  dg_status agg_st = DG_OK;
  {
    std::lock_guard<std::mutex> lk(pmu_);
    auto it = split_.find(ticket);
    if (it == split_.end()) return wait(ticket);
    rec = it->second;
    if (rec.gen && rec.gen == pagg_gen_) flush_pagg_locked();  // someone blocks on the open aggregate: launch it now
    if (rec.gen) {
      const PGen &g = pgen_[rec.gen];
      tps = g.tickets;
      agg_st = g.st;
    }
  }
  dg_status st = DG_OK;
  for (uint64_t t : rec.tbs) {
    const dg_status s1 = wait(t);
    if (!st) st = s1;
  }
  dg_status st2 = agg_st;
  for (uint64_t t : tps) {
    const dg_status s1 = wait(t);
    if (!st2) st2 = s1;
  }
  std::lock_guard<std::mutex> lk(pmu_);
  if (split_.erase(ticket) && rec.gen) {
    auto g = pgen_.find(rec.gen);
    if (g != pgen_.end() && --g->second.refs <= 0) pgen_.erase(g);
  }
  return st ? st : st2;
}

dg_status Context::wait_ready(uint64_t ticket, int32_t *pending) {
  SplitRec rec;
  {
    std::lock_guard<std::mutex> lk(pmu_);
    if (pagg_stale_locked()) flush_pagg_locked();
    auto it = split_.find(ticket);
    if (it == split_.end()) {
      if (pending) *pending = 0;
      return wait(ticket);
    }
    rec = it->second;
  }
  dg_status st = DG_OK;
  for (uint64_t t : rec.tbs) {
    const dg_status s1 = wait(t);
    if (!st) st = s1;
  }
  if (pending) {  // progressive members not complete yet (their metas read DG_ERR_NOT_READY)
    std::vector<uint64_t> tps;
    bool busy = false;
    dg_status agg_st = DG_OK;
    if (rec.gen) {
      std::lock_guard<std::mutex> lk(pmu_);
      if (rec.gen != pagg_gen_) {
        auto g = pgen_.find(rec.gen);
        if (g != pgen_.end()) {
          tps = g->second.tickets;
          agg_st = g->second.st;
        }
      }
      busy = rec.gen == pagg_gen_;
      for (uint64_t t : tps) busy = busy || poll(t) == DG_ERR_NOT_READY;
    }
    // The aggregate's kernels are done: complete it (outputs copied to host
    // buffers, statuses written, metas published) before reporting 0 pending,
    // so pending == 0 means the progressive members are ready to read.  The
    // events have completed, so this does not block (bar a rare entropy
    // resync); it runs outside pmu_, like wait_user's, so polls and waits on
    // other tickets do not queue behind the aggregate's output copies.
    dg_status st2 = agg_st;
    if (!busy)
      for (uint64_t t : tps) {
        const dg_status s1 = wait(t);
        if (!st2) st2 = s1;
      }
    *pending = busy ? rec.nprog : 0;
    if (!st) st = st2;
  }
  return st;
}

dg_status Context::poll_user(uint64_t ticket) {
  SplitRec rec;
  std::vector<uint64_t> tps;
  {
    std::lock_guard<std::mutex> lk(pmu_);
    if (pagg_stale_locked()) flush_pagg_locked();
    auto it = split_.find(ticket);
    if (it == split_.end()) return poll(ticket);
    rec = it->second;
    if (rec.gen && rec.gen == pagg_gen_) return DG_ERR_NOT_READY;
    if (rec.gen) tps = pgen_[rec.gen].tickets;
  }
  for (uint64_t t : rec.tbs)
    if (poll(t) == DG_ERR_NOT_READY) return DG_ERR_NOT_READY;
  for (uint64_t t : tps)
    if (poll(t) == DG_ERR_NOT_READY) return DG_ERR_NOT_READY;
  return DG_OK;
}

}  // namespace dg
