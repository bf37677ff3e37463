// Non-interleaved baseline JPEGs (context option "jpeg_multiscan") without a GPU
// (test infrastructure, tests/test_jpeg_multiscan_cpu.py): the header parser's
// allow_multiscan flag, the scan -> parent block map of dg_types.h (ms_scan_map /
// ms_index, what k_huff_write's multiscan instantiation applies) and every
// scan's entropy stream through the product's own lead_in + decode_range,
// written through that map into one MCU-interleaved buffer.
//
// Built as a shared library for the tests, and with -DMS_MAIN as a stand-alone
// program (also under -fsanitize=address,undefined) that runs the same entry
// points over one file and every truncation of it.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dg_entropy.h"
#include "host/jpeg_header.h"

using namespace dg;

static int64_t fnv(const HuffSpec &t) {  // FNV-1a over bits[1..16] and the values
  uint32_t x = 2166136261u;
  for (int i = 1; i <= 16; i++) x = (x ^ t.bits[i]) * 16777619u;
  for (int i = 0; i < t.nvals; i++) x = (x ^ t.vals[i]) * 16777619u;
  return (int64_t)x;
}

// status of parse_jpeg_header; its `why` into why[cap]; when JH_OK: info[0] = scans (0: a single-scan file),
// info[1] = multiscan, then 10 values per scan: ns, comp0, comp1, restart, off, end, hash of the DC and AC
// table of its first and of its second component
extern "C" int ms_parse(const uint8_t *data, size_t len, int allow_multiscan, int allow_h1v2, int allow_cmyk, char *why,
                        size_t cap, int64_t *info, size_t info_cap) {
  JpegHeader h;
  if (allow_multiscan || allow_h1v2 || allow_cmyk)
    parse_jpeg_header(data, len, h, allow_h1v2 != 0, allow_cmyk != 0, allow_multiscan != 0);
  else
    parse_jpeg_header(data, len, h);  // the default arguments, as capi.cpp and the tools call it
  if (cap) {
    strncpy(why, h.why, cap - 1);
    why[cap - 1] = 0;
  }
  if (info && info_cap >= 2 && h.status == JH_OK) {
    info[0] = (int64_t)h.scans.size();
    info[1] = h.multiscan ? 1 : 0;
    for (size_t j = 0; j < h.scans.size() && 2 + 10 * (j + 1) <= info_cap; j++) {
      const JpegScan &sc = h.scans[j];
      int64_t *o = info + 2 + 10 * j;
      o[0] = sc.ns;
      o[1] = sc.comp[0];
      o[2] = sc.ns > 1 ? sc.comp[1] : -1;
      o[3] = sc.restart;
      o[4] = (int64_t)sc.off;
      o[5] = (int64_t)sc.end;
      for (int q = 0; q < 2; q++) {
        const bool on = h.multiscan && q < sc.ns;
        o[6 + 2 * q] = on ? fnv(h.tables[sc.dc_tab[q]]) : -1;
        o[7 + 2 * q] = on ? fnv(h.tables[sc.ac_tabs[q]]) : -1;
      }
    }
  }
  return h.status;
}

// The parent descriptor's geometry, as the planner's layout_jpeg sets it for a colour file.
static void parent_geometry(uint32_t W, uint32_t H, const int *hs, const int *vs, ImageDesc &d) {
  memset(&d, 0, sizeof(d));
  d.width = W;
  d.height = H;
  d.ncomp = 3;
  for (int c = 0; c < 3; c++) {
    if ((uint32_t)hs[c] > d.hmax) d.hmax = hs[c];
    if ((uint32_t)vs[c] > d.vmax) d.vmax = vs[c];
  }
  d.mcux = (W + 8 * d.hmax - 1) / (8 * d.hmax);
  d.mcuy = (H + 8 * d.vmax - 1) / (8 * d.vmax);
  uint32_t bpm = 0;
  for (int c = 0; c < 3; c++) {
    d.ch[c] = hs[c];
    d.cv[c] = vs[c];
    d.cdsw[c] = (uint32_t)(((uint64_t)W * hs[c] + d.hmax - 1) / d.hmax);
    d.cdsh[c] = (uint32_t)(((uint64_t)H * vs[c] + d.vmax - 1) / d.vmax);
    d.cbw[c] = d.mcux * hs[c];
    d.cbh[c] = d.mcuy * vs[c];
    d.cfirst[c] = bpm;
    bpm += hs[c] * vs[c];
  }
  d.bpm = bpm;
  d.total_blocks = d.mcux * d.mcuy * bpm;
}

// ms_index(g) for every block g of a scan of components comp[0..ns) of a W x H frame with factors hs / vs;
// returns the scan's block count (-1: more than cap), *parent_total = the parent's blocks
extern "C" int64_t ms_map(uint32_t W, uint32_t H, const int *hs, const int *vs, int ns, const int *comp, uint32_t *out,
                          size_t cap, uint32_t *parent_total) {
  ImageDesc par;
  parent_geometry(W, H, hs, vs, par);
  uint32_t total = 0;
  const ScanMap m = ms_scan_map(par, (uint32_t)ns, comp, total);
  *parent_total = par.total_blocks;
  if (total > cap) return -1;
  for (uint32_t g = 0; g < total; g++) out[g] = ms_index(m, g);
  return total;
}

// ms_div against the machine's division, over the divisors and dividends the map can meet and the edges
extern "C" int64_t ms_div_errors() {
  int64_t bad = 0;
  const uint32_t gs[] = {0u,      1u,       2u,          7u,          8191u,       8192u,
                         65535u,  1u << 24, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (uint32_t d = 1; d <= 8200; d++) {
    const uint32_t r = ms_recip(d);
    for (uint32_t g : gs)
      for (uint32_t e = 0; e < 3; e++) {
        const uint32_t x = g - e * d;  // (wraps: any value will do)
        uint32_t rem;
        const uint32_t q = ms_div(x, d, r, rem);
        bad += q != x / d || rem != x % d;
      }
    if (d > 40 && d % 97) continue;
    for (uint32_t x = 0; x < 70000; x += 1 + d % 7) {
      uint32_t rem;
      const uint32_t q = ms_div(x, d, r, rem);
      bad += q != x / d || rem != x % d;
    }
  }
  return bad;
}

// Every scan of a multiscan file as a stream of its own: destuffed as k_destuff_* do, its subsequences'
// entry states by lead_in, the state-only decode_range over the exact chain, the segmented scan, and the
// write pass's decode_range in its multiscan instantiation into one zeroed MCU-interleaved buffer.
// out: the parent's blocks in MCU-interleaved (decode) order, natural coefficient order.
// stats: [0] subsequences, [1] lead-in guesses that were the true state, [2] write exits that differ from the
// chain, [3] blocks the scans decoded, [4] blocks they were to decode
extern "C" int ms_emu(const uint8_t *data, size_t len, uint32_t sub_bits, uint32_t lead, int allow_h1v2, int16_t *out,
                      size_t cap_blocks, size_t *nblocks, int64_t *stats) {
  JpegHeader h;
  parse_jpeg_header(data, len, h, allow_h1v2 != 0, false, true);
  if (h.status != JH_OK) return h.status;
  if (!h.multiscan) return -1;
  int hs[3], vs[3];
  for (int c = 0; c < 3; c++) {
    hs[c] = h.comp[c].h;
    vs[c] = h.comp[c].v;
  }
  ImageDesc par;
  parent_geometry(h.width, h.height, hs, vs, par);
  std::vector<int16_t> coef((size_t)par.total_blocks * 64, 0);
  int64_t nsub_all = 0, guessed = 0, mismatch = 0, decoded_all = 0, want_all = 0;
  for (const JpegScan &sc : h.scans) {
    ImageDesc d;
    memset(&d, 0, sizeof(d));
    d.ncomp = (uint8_t)sc.ns;
    d.ms = ms_scan_map(par, (uint32_t)sc.ns, sc.comp, d.total_blocks);
    uint32_t bpm = 0;
    std::vector<HuffTable> tabs;
    for (int q = 0; q < sc.ns; q++) {
      const uint32_t nb = sc.ns == 1 ? 1u : par.ch[sc.comp[q]] * par.cv[sc.comp[q]];
      for (uint32_t k = 0; k < nb; k++) d.comp_bits |= (uint32_t)q << (2 * (bpm + k));
      bpm += nb;
      HuffTable t;
      if (!build_huff_table(h.tables[sc.dc_tab[q]], t)) return JH_CORRUPT;
      d.slotmap |= (uint32_t)tabs.size() << ((2 * q) * 4);
      tabs.push_back(t);
      if (!build_huff_table(h.tables[sc.ac_tabs[q]], t)) return JH_CORRUPT;
      d.slotmap |= (uint32_t)tabs.size() << ((2 * q + 1) * 4);
      tabs.push_back(t);
    }
    d.bpm = bpm;
    d.restart = (uint32_t)sc.restart;
    d.blocks_per_seg = d.restart * bpm;
    d.scan_len = (uint32_t)(sc.end - sc.off);
    const uint8_t *raw = data + sc.off;
    std::vector<uint8_t> ds;
    std::vector<uint32_t> mk;
    for (uint32_t i = 0; i < d.scan_len; i++) {
      uint32_t prev = i ? raw[i - 1] : 0, next = i + 1 < d.scan_len ? raw[i + 1] : 0xD9, m;
      uint32_t keep = destuff_keep(prev, raw[i], next, i == 0, &m);
      if (m) mk.push_back((uint32_t)ds.size() * 8);
      if (keep) ds.push_back(raw[i]);
    }
    d.ds_bits = (uint32_t)ds.size() * 8;
    d.nmk = (uint32_t)mk.size();
    ds.resize(((ds.size() + 3) & ~(size_t)3) + 64, 0);
    d.sub_bits = sub_bits;
    d.lead_bits = lead;
    d.nsub = d.scan_len ? (uint32_t)(((uint64_t)d.scan_len * 8 + sub_bits - 1) / sub_bits) : 1;
    d.ds_lsw = 0;
    while ((32u << d.ds_lsw) < sub_bits) d.ds_lsw++;
    std::vector<uint32_t> phys((size_t)ds_words_alloc(d.nsub, d.ds_lsw), 0u);
    for (size_t wi = 0; wi * 4 < ds.size(); wi++) {
      uint32_t v;
      memcpy(&v, &ds[wi * 4], 4);
      const uint32_t pi = ds_word_index((uint32_t)wi, d.ds_lsw);
      if (pi < phys.size()) phys[pi] = v;
    }
    const uint8_t *scan = (const uint8_t *)phys.data();
    const uint32_t *mkp = mk.data();
    std::vector<SubState> subs(d.nsub);
    uint32_t prev_out = pack_state(0, 0, 0);
    for (uint32_t s = 0; s < d.nsub; s++) {
      const uint32_t guess = lead_in(d, tabs.data(), scan, mkp, s, d.lead_bits);
      const uint32_t in = s ? prev_out : pack_state(0, 0, 0);
      guessed += guess == in;
      RangeAcc a;
      decode_range<false>(d, tabs.data(), scan, mkp, s, in, a, nullptr);
      SubState &o = subs[s];
      memset(&o, 0, sizeof(o));
      o.in = in;
      o.out = a.out;
      o.m = a.m;
      o.n = a.n;
      for (int c = 0; c < 3; c++) o.dc[c] = a.dc[c];
      prev_out = a.out;
    }
    uint32_t cm = 0, cn = 0;
    int32_t cd[3] = {0, 0, 0};
    for (uint32_t i = 0; i < d.nsub; i++) {  // k_huff_scan
      subs[i].seg = cm;
      subs[i].nin = cn;
      for (int c = 0; c < 3; c++) subs[i].dcin[c] = cd[c];
      if (subs[i].m) {
        cm += subs[i].m;
        cn = subs[i].n;
        for (int c = 0; c < 3; c++) cd[c] = subs[i].dc[c];
      } else {
        cn += subs[i].n;
        for (int c = 0; c < 3; c++) cd[c] += subs[i].dc[c];
      }
    }
    decoded_all += d.blocks_per_seg ? (int64_t)cm * d.blocks_per_seg + cn : cn;
    want_all += d.total_blocks;
    int16_t blk[64];
    for (uint32_t s = 0; s < d.nsub; s++) {  // k_huff_write<3, true>
      WriteCtx w;
      w.blk = blk;
      w.coef = coef.data();
      w.seg = subs[s].seg;
      w.nin = subs[s].nin;
      for (int c = 0; c < 3; c++) w.pred[c] = subs[s].dcin[c];
      w.blocks_per_seg = d.blocks_per_seg;
      w.total_blocks = d.total_blocks;
      w.cur = -1;
      w.zs = 0;
      RangeAcc acc;
      decode_range<true, HuffTable, false, 3, true>(d, tabs.data(), scan, mkp, s, subs[s].in, acc, &w, nullptr, false, 0,
                                                    nullptr, nullptr, 0xFFu, 3u);
      if (acc.out != subs[s].out) mismatch++;
    }
    nsub_all += d.nsub;
  }
  static const int nat[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  *nblocks = par.total_blocks;
  for (size_t b = 0; b < par.total_blocks && b < cap_blocks; b++)
    for (int k = 0; k < 64; k++) out[b * 64 + nat[k]] = coef[b * 64 + k];
  if (stats) {
    stats[0] = nsub_all;
    stats[1] = guessed;
    stats[2] = mismatch;
    stats[3] = decoded_all;
    stats[4] = want_all;
  }
  return 0;
}

#ifdef MS_MAIN
// multiscan_main FILE [REFUSED...]: the parser with and without the flag over the file and over every truncation of it, the
// emulator over the file and the division check; then every REFUSED file and its truncations through the parser
// with every flag on (exit 4 if one parses); prints one line of counts.  Exit status 0 unless the whole
// file does not parse as a multiscan file.
int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> d;
  uint8_t buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + n);
  fclose(f);
  char why[160];
  int64_t info[2 + 10 * 8];
  int count[3] = {0, 0, 0};
  for (size_t cut = 0; cut <= d.size(); cut++) {
    std::vector<uint8_t> part(d.begin(), d.begin() + cut);  // its own allocation: a read past the cut is an error
    const int st = ms_parse(part.data(), part.size(), 1, 0, 0, why, sizeof(why), info, sizeof(info) / sizeof(info[0]));
    if (st < 0 || st > 2) return 3;
    count[st]++;
    (void)ms_parse(part.data(), part.size(), 0, 0, 0, why, sizeof(why), info, sizeof(info) / sizeof(info[0]));
  }
  const int st = ms_parse(d.data(), d.size(), 1, 0, 0, why, sizeof(why), info, sizeof(info) / sizeof(info[0]));
  if (st != JH_OK || !info[1]) return 1;
  std::vector<int16_t> out((size_t)1 << 20);
  size_t nb = 0;
  int64_t stats[5] = {0, 0, 0, 0, 0};
  const int es = ms_emu(d.data(), d.size(), 256, 128, 0, out.data(), out.size() / 64, &nb, stats);
  // further files (refusal cases): every flag on, the whole file and every truncation of it
  for (int a = 2; a < argc; a++) {
    FILE *g = fopen(argv[a], "rb");
    if (!g) return 2;
    std::vector<uint8_t> e;
    for (size_t n; (n = fread(buf, 1, sizeof(buf), g)) > 0;) e.insert(e.end(), buf, buf + n);
    fclose(g);
    for (size_t cut = 0; cut <= e.size(); cut++) {
      std::vector<uint8_t> part(e.begin(), e.begin() + cut);
      const int r = ms_parse(part.data(), part.size(), 1, 1, 1, why, sizeof(why), info, sizeof(info) / sizeof(info[0]));
      if (r < 0 || r > 2) return 3;
      if (cut == e.size() && r == JH_OK) return 4;  // a refusal case that parses
    }
  }
  printf("ok %d unsupported %d corrupt %d scans %lld emu %d blocks %zu mismatch %lld div_errors %lld\n", count[0],
         count[1], count[2], (long long)info[0], es, nb, (long long)stats[2], (long long)ms_div_errors());
  return 0;
}
#endif
