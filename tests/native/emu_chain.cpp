// CPU check of the chained multi steps of the state-only decodes (option
// "sync_chain": multi_chain in dg_entropy.h; test infrastructure).  For one
// image and one chain setting it runs the product's lead_in and
// decode_range<false> over every range the way k_huff_sync does -- lead-in
// guess, first decode with checkpoints, re-decode with checkpoint merging
// where the guess was wrong -- then the scan and the write pass, and hands
// back every state it produced, so that the test can compare chain 1..3 with
// chain 0 word for word and the coefficients with the oracle.  It also counts
// the loop iterations of the two state-only decodes (DG_STEP_STATS).
#define DG_STEP_STATS 1
#include <stdint.h>
#include <string.h>

#include <vector>

#include "dg_entropy.h"
#include "host/jpeg_header.h"

using namespace dg;

// rec: per range 7 words (in, out, m, n, dc[3]) + 6 per checkpoint after the
// first decode of every range, then the same again after the re-decodes.
// stats: nsub, lead-in steps, first-decode steps, chained entries taken (all
// state-only decodes), steps over 32 bits, write-pass exit mismatches,
// blocks decoded, blocks of the image, re-decoded ranges, re-decode steps.
extern "C" int emu_chain_decode(const uint8_t *data, size_t len, uint32_t sub_bits, uint32_t lead, uint32_t chain,
                                int16_t *out, size_t cap_blocks, size_t *nblocks, uint32_t *rec, size_t cap_rec,
                                size_t *nrec, int64_t *stats) {
  JpegHeader h;
  parse_jpeg_header(data, len, h);
  if (h.status != JH_OK) return h.status;
  ImageDesc d;
  memset(&d, 0, sizeof(d));
  const uint32_t W = h.width, H = h.height;
  d.ncomp = (uint8_t)h.ncomp;
  d.hmax = h.hmax;
  d.vmax = h.vmax;
  d.mcux = (W + 8 * d.hmax - 1) / (8 * d.hmax);
  d.mcuy = (H + 8 * d.vmax - 1) / (8 * d.vmax);
  uint32_t bpm = 0, cbw0 = 0, cbh0 = 0;
  for (int c = 0; c < h.ncomp; c++) {
    if (h.ncomp == 1) {
      const uint32_t dsw = (W * h.comp[c].h + d.hmax - 1) / d.hmax, dsh = (H * h.comp[c].v + d.vmax - 1) / d.vmax;
      cbw0 = (dsw + 7) / 8;
      cbh0 = (dsh + 7) / 8;
      d.blk_comp[0] = 0;
      bpm = 1;
    } else {
      for (int j = 0; j < h.comp[c].h * h.comp[c].v; j++) d.blk_comp[bpm + j] = (uint8_t)c;
      bpm += h.comp[c].h * h.comp[c].v;
    }
  }
  d.bpm = bpm;
  for (uint32_t k = 0; k < bpm; k++) d.comp_bits |= (uint32_t)d.blk_comp[k] << (2 * k);
  d.total_blocks = h.ncomp == 1 ? cbw0 * cbh0 : d.mcux * d.mcuy * bpm;
  d.restart = h.restart;
  d.blocks_per_seg = d.restart * bpm;
  std::vector<HuffTable> tabs;
  for (int c = 0; c < h.ncomp; c++) {
    HuffTable t;
    build_huff_table(h.dc[h.comp[c].td], t);
    d.slotmap |= (uint32_t)tabs.size() << ((2 * c) * 4);
    tabs.push_back(t);
    build_huff_table(h.ac[h.comp[c].ta], t);
    d.slotmap |= (uint32_t)tabs.size() << ((2 * c + 1) * 4);
    tabs.push_back(t);
  }
  // k_huff_sync's multi-symbol lookups: one per component's AC table (slots 2c + 1)
  std::vector<uint16_t> mt;
  uint32_t acm = 0xFFu;
  for (int c = 0; c < h.ncomp && c < (int)kMultiLuts; c++) {
    for (uint32_t p = 0; p < (1u << kMultiBits); p++) mt.push_back((uint16_t)multi_entry(tabs[2 * c + 1], p));
    acm = (acm & ~(3u << (2 * c))) | ((uint32_t)c << (2 * c));
  }
  d.scan_len = (uint32_t)(h.scan_end - h.scan_off);
  const uint8_t *raw = data + h.scan_off;
  std::vector<uint8_t> ds;  // destuffed as k_destuff_* do
  std::vector<uint32_t> mk;
  for (uint32_t i = 0; i < d.scan_len; i++) {
    const uint32_t prev = i ? raw[i - 1] : 0, next = i + 1 < d.scan_len ? raw[i + 1] : 0xD9;
    uint32_t m;
    const uint32_t keep = destuff_keep(prev, raw[i], next, i == 0, &m);
    if (m) mk.push_back((uint32_t)ds.size() * 8);
    if (keep) ds.push_back(raw[i]);
  }
  d.ds_bits = (uint32_t)ds.size() * 8;
  d.nmk = (uint32_t)mk.size();
  ds.resize(((ds.size() + 3) & ~(size_t)3) + 64, 0);
  d.sub_bits = sub_bits;
  d.lead_bits = lead;
  d.nsub = d.scan_len ? (uint32_t)(((uint64_t)d.scan_len * 8 + sub_bits - 1) / sub_bits) : 1;
  while ((32u << d.ds_lsw) < sub_bits) d.ds_lsw++;
  std::vector<uint32_t> phys((size_t)ds_words_alloc(d.nsub, d.ds_lsw), 0u);  // the kernels' interleaved layout
  for (size_t wi = 0; wi * 4 < ds.size(); wi++) {
    uint32_t v;
    memcpy(&v, &ds[wi * 4], 4);
    const uint32_t pi = ds_word_index((uint32_t)wi, d.ds_lsw);
    if (pi < phys.size()) phys[pi] = v;
  }
  const uint8_t *scan = (const uint8_t *)phys.data();
  const uint32_t *mkp = mk.data();
  const uint32_t NCK = num_ckpt(d.sub_bits);
  std::vector<Ckpt> ck((size_t)d.nsub * (NCK ? NCK : 1));  // zeroed: records a decode does not reach stay 0
  auto ckp = [&](uint32_t s) { return NCK ? &ck[(size_t)s * NCK] : (Ckpt *)nullptr; };
  std::vector<uint32_t> ins(d.nsub), ex(d.nsub);
  std::vector<RangeAcc> acc(d.nsub);
  size_t nr = 0;
  auto put = [&](uint32_t v) {
    if (nr < cap_rec) rec[nr] = v;
    nr++;
  };
  auto dump = [&]() {
    for (uint32_t s = 0; s < d.nsub; s++) {
      put(ins[s]), put(ex[s]), put(acc[s].m), put(acc[s].n);
      for (int c = 0; c < 3; c++) put((uint32_t)acc[s].dc[c]);
      for (uint32_t j = 0; j < NCK; j++) {
        const Ckpt &c = ckp(s)[j];
        put(c.st), put(c.m), put(c.n), put((uint32_t)c.dc[0]), put((uint32_t)c.dc[1]), put((uint32_t)c.dc[2]);
      }
    }
  };
  g_step_stats = StepStats{0, 0, 0, 0};
  // ---- k_huff_sync: lead-in guess and first decode of every range
  for (uint32_t s = 0; s < d.nsub; s++) {
    ins[s] = lead_in(d, tabs.data(), scan, mkp, s, d.lead_bits, mt.data(), acm, false, chain);
    decode_range<false>(d, tabs.data(), scan, mkp, s, ins[s], acc[s], nullptr, ckp(s), false, 0, nullptr, mt.data(),
                        acm, 0u, kInf, kInf, chain);
    ex[s] = acc[s].out;
  }
  const uint64_t lead_steps = g_step_stats.lead_steps, first_steps = g_step_stats.range_steps;
  dump();
  // ---- its verification loop (and k_huff_fix): re-decode from the predecessor's exit, merging at checkpoints
  int64_t redo = 0;
  for (uint32_t s = 1; s < d.nsub; s++)
    if (ins[s] != ex[s - 1]) {
      decode_range<false>(d, tabs.data(), scan, mkp, s, ex[s - 1], acc[s], nullptr, ckp(s), true, ex[s], nullptr,
                          mt.data(), acm, 0u, kInf, kInf, chain);
      ins[s] = ex[s - 1];
      ex[s] = acc[s].out;
      redo++;
    }
  dump();
  const StepStats ss = g_step_stats;
  // ---- k_huff_scan (segmented exclusive scan) and k_huff_write
  std::vector<int16_t> coef((size_t)d.total_blocks * 64, (int16_t)0x7777);  // poison: every slot must be written
  uint32_t cm = 0, cn = 0;
  int32_t cd[3] = {0, 0, 0};
  int64_t mismatch = 0;
  int16_t blk[64];
  for (uint32_t s = 0; s < d.nsub; s++) {
    WriteCtx w;
    w.blk = blk;
    w.coef = coef.data();
    w.seg = cm;
    w.nin = cn;
    for (int c = 0; c < 3; c++) w.pred[c] = cd[c];
    w.blocks_per_seg = d.blocks_per_seg;
    w.total_blocks = d.total_blocks;
    w.cur = -1;
    w.zs = 0;
    RangeAcc a;
    decode_range<true>(d, tabs.data(), scan, mkp, s, ins[s], a, &w, nullptr, false, 0, nullptr, nullptr, 0xFFu, 3u);
    if (a.out != ex[s]) mismatch++;
    if (acc[s].m) {
      cm += acc[s].m;
      cn = acc[s].n;
      for (int c = 0; c < 3; c++) cd[c] = acc[s].dc[c];
    } else {
      cn += acc[s].n;
      for (int c = 0; c < 3; c++) cd[c] += acc[s].dc[c];
    }
  }
  const uint64_t decoded = d.blocks_per_seg ? (uint64_t)cm * d.blocks_per_seg + cn : cn;
  static const int nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  *nblocks = d.total_blocks;
  for (size_t b = 0; b < d.total_blocks && b < cap_blocks; b++)
    for (int k = 0; k < 64; k++) out[b * 64 + nat[k]] = coef[b * 64 + k];
  *nrec = nr;
  stats[0] = d.nsub;
  stats[1] = (int64_t)lead_steps;
  stats[2] = (int64_t)first_steps;
  stats[3] = (int64_t)ss.chained;
  stats[4] = (int64_t)ss.over32;
  stats[5] = mismatch;
  stats[6] = (int64_t)decoded;
  stats[7] = d.total_blocks;
  stats[8] = redo;
  stats[9] = (int64_t)(ss.range_steps - first_steps);
  return nr <= cap_rec ? 0 : -1;
}
