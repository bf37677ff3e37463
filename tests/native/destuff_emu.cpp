// destuff_emu.cpp — the lane routines of the destuff count and write passes
// (datago_amd/csrc/dg_destuff.h) on the CPU, against a plain byte loop built
// on destuff_keep.  A program of its own: exit status 0 when every case
// agrees, else 1 with the first differences on stderr.  Built plain and with
// -fsanitize=address,undefined by tests/test_destuff_cpu.py.
//
// The scan is held in an allocation of exactly offset + length bytes, so a
// load outside it is a sanitizer error; every window load is also checked
// against the scan's bounds here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dg_destuff.h"

using namespace dg;

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

static int g_fail = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      if (g_fail < 20) {                        \
        fprintf(stderr, "FAIL %s: ", #cond);    \
        fprintf(stderr, __VA_ARGS__);           \
        fprintf(stderr, "\n");                  \
      }                                         \
      g_fail++;                                 \
    }                                           \
  } while (0)

struct Ref {
  std::vector<uint8_t> kept;
  std::vector<uint32_t> mk;                // bit positions
  std::vector<uint32_t> cnt, mkc;          // per chunk
};

static Ref reference(const uint8_t *raw, uint32_t n) {
  Ref R;
  const uint32_t nchunk = n ? (n + kDestuffChunk - 1) / kDestuffChunk : 1u;
  R.cnt.assign(nchunk, 0);
  R.mkc.assign(nchunk, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t prev = i ? raw[i - 1] : 0u, next = i + 1 < n ? raw[i + 1] : 0xD9u;
    uint32_t m;
    const uint32_t k = destuff_keep(prev, raw[i], next, i == 0, &m);
    if (m) {
      R.mk.push_back((uint32_t)R.kept.size() * 8u);
      R.mkc[i / kDestuffChunk]++;
    }
    if (k) {
      R.kept.push_back(raw[i]);
      R.cnt[i / kDestuffChunk]++;
    }
  }
  return R;
}

// the kernel's ds_load_span, with loads that check the scan's bounds
static uint32_t load_span(const uint8_t *raw, uint32_t n, uint32_t i0, uint32_t r[16], uint32_t *prev,
                          uint32_t *next) {
  const uint32_t nv = i0 < n ? (n - i0 < kDsLane ? n - i0 : kDsLane) : 0u;
  if (ds_window_in_scan(i0, n)) {
    const uintptr_t a0 = (uintptr_t)(raw + i0 - 1) & ~(uintptr_t)3;
    const uint32_t sh = (uint32_t)((uintptr_t)(raw + i0 - 1) & 3);
    CHECK(a0 >= (uintptr_t)raw && a0 + 72 <= (uintptr_t)raw + n, "window of byte %u leaves the scan of %u", i0, n);
    uint32_t x[18];
    memcpy(x, (const void *)a0, 72);
    ds_window(x, sh, r, prev, next);
  } else if (nv) {
    ds_span_bytes(raw + i0, nv, i0 > 0u, i0 + kDsLane < n, r, prev, next);
  } else {
    for (int m = 0; m < 16; m++) r[m] = 0u;
    *prev = 0u;
  }
  if (i0 + kDsLane >= n) *next = 0xD9u;
  return nv;
}

static void run_case(const std::vector<uint8_t> &scan, uint32_t off, const char *what) {
  const uint32_t n = (uint32_t)scan.size();
  // a 16-aligned allocation of exactly off + n bytes with the scan at its end:
  // the scan starts at an address that is off mod 16, and the byte after it
  // is the sanitizer's
  void *mem = nullptr;
  if (posix_memalign(&mem, 16, (size_t)off + n + (off + n == 0)) != 0) abort();
  memset(mem, 0xFF, (size_t)off + n);
  uint8_t *raw = (uint8_t *)mem + off;
  if (n) memcpy(raw, scan.data(), n);
  struct Free {
    void *p;
    ~Free() { free(p); }
  } guard{mem};

  const Ref R = reference(raw, n);
  const uint32_t nchunk = (uint32_t)R.cnt.size();

  // count pass
  std::vector<uint32_t> cnt(nchunk), mkc(nchunk), offs(nchunk), mkoff(nchunk);
  for (uint32_t c = 0; c < nchunk; c++) {
    uint32_t v = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
      uint32_t r[16], prev, next;
      const uint32_t nv = load_span(raw, n, c * kDestuffChunk + lane * kDsLane, r, &prev, &next);
      if (nv == kDsLane) {
        uint32_t K[16];
        const uint32_t any = ds_keep_flags64(r, prev, next, K);
        v += ds_count_flags64(K);
        if (any) {
          uint32_t M[16];
          ds_marker_flags64(r, next, M);
          v += ds_count_flags64(M) << 16;
        }
        // the byte routine agrees with the flags
        uint64_t km, mm;
        ds_classify64(r, prev, next, nv, &km, &mm);
        for (uint32_t j = 0; j < 64; j++)
          CHECK(((K[j >> 2] >> (8 * (j & 3) + 7)) & 1u) == ((km >> j) & 1u), "%s off %u n %u: keep flag of byte %u", what,
                off, n, c * kDestuffChunk + lane * kDsLane + j);
      } else {
        uint64_t km, mm;
        ds_classify64(r, prev, next, nv, &km, &mm);
        v += ds_popc64(km) | (ds_popc64(mm) << 16);
      }
    }
    cnt[c] = v & 0xFFFFu;
    mkc[c] = v >> 16;
    CHECK(cnt[c] == R.cnt[c] && mkc[c] == R.mkc[c], "%s off %u n %u chunk %u: counts %u/%u, expected %u/%u", what, off, n,
          c, cnt[c], mkc[c], R.cnt[c], R.mkc[c]);
  }
  // per-image scan
  uint32_t ck = 0, cm = 0;
  for (uint32_t c = 0; c < nchunk; c++) {
    offs[c] = ck;
    mkoff[c] = cm;
    ck += cnt[c];
    cm += mkc[c];
  }
  CHECK(ck == R.kept.size() && cm == R.mk.size(), "%s off %u n %u: totals", what, off, n);
  if (g_fail) return;

  // write pass, one workgroup of kDsWgChunks chunks at a time
  std::vector<uint32_t> mk(cm + 1, 0xFFFFFFFFu);
  std::vector<uint8_t> out(ck, 0);
  std::vector<uint32_t> st(kDsStageAlloc);
  for (uint32_t c0 = 0; c0 < nchunk; c0 += kDsWgChunks) {
    const uint32_t nc = nchunk - c0 < kDsWgChunks ? nchunk - c0 : kDsWgChunks;
    const uint32_t O = offs[c0], E = offs[c0 + nc - 1] + cnt[c0 + nc - 1], wbase = O >> 2;
    for (auto &w : st) w = 0xA5A5A5A5u;
    for (uint32_t wave = 0; wave < nc; wave++) {
      uint32_t ex = 0;
      for (uint32_t lane = 0; lane < 64; lane++) {
        uint32_t r[16], prev, next;
        const uint32_t nv = load_span(raw, n, (c0 + wave) * kDestuffChunk + lane * kDsLane, r, &prev, &next);
        uint32_t K[16], any = 0, own;
        uint64_t km = 0, mm = 0;
        if (nv == kDsLane) {
          any = ds_keep_flags64(r, prev, next, K);
          own = ds_count_flags64(K);
          if (any) {
            uint32_t M[16];
            ds_marker_flags64(r, next, M);
            own |= ds_count_flags64(M) << 16;
          }
        } else {
          ds_classify64(r, prev, next, nv, &km, &mm);
          own = ds_popc64(km) | (ds_popc64(mm) << 16);
        }
        const uint32_t pos = offs[c0 + wave] - 4u * wbase + (ex & 0xFFFFu);
        CHECK(pos + (own & 0xFFFFu) <= 4u * kDsStageWords, "%s: staging position %u", what, pos);
        uint32_t mo = mkoff[c0 + wave] + (ex >> 16);
        auto mark = [&](uint32_t p) {
          if (mo < cm) mk[mo] = (4u * wbase + p) * 8u;
          mo++;
        };
        if (nv == kDsLane) {
          if (own >> 16) {
            uint32_t M[16];
            ds_marker_flags64(r, next, M);
            ds_mark64(pos, K, M, mark);
          }
          if ((own & 0xFFFFu) != kDsLane) ds_compact64(r, K);
          ds_put_bytes(st.data(), pos, r, own & 0xFFFFu);
        } else {
          ds_emit64(st.data(), pos, r, km, mm, mark);
        }
        ex += own;
      }
    }
    for (uint32_t q = O; q < E; q++) out[q] = (uint8_t)ds_get_byte(st.data(), q - 4u * wbase);
    // nothing of the staging buffer outside [O, E) was written
    for (uint32_t q = 4u * wbase; q < 4u * wbase + 4u * kDsStageWords; q++)
      if (q < O || q >= E) CHECK(ds_get_byte(st.data(), q - 4u * wbase) == 0xA5u, "%s off %u n %u: staging byte %u written", what, off, n, q);
  }
  CHECK(out == R.kept, "%s off %u n %u: kept bytes differ", what, off, n);
  mk.resize(cm);
  CHECK(mk == R.mk, "%s off %u n %u: marker positions differ", what, off, n);
}

// positions whose byte is the last of a lane, a wave (= chunk) and the scan
static std::vector<uint32_t> boundaries(uint32_t n) {
  std::vector<uint32_t> b;
  for (uint32_t p = 63; p < n; p += 64)
    if (p < 512 || p % kDestuffChunk == kDestuffChunk - 1 || p + 256 > n) b.push_back(p);
  if (n) b.push_back(n - 1);
  return b;
}

static void put(std::vector<uint8_t> &s, int64_t at, const uint8_t *seq, uint32_t len) {
  for (uint32_t k = 0; k < len; k++)
    if (at + k >= 0 && at + k < (int64_t)s.size()) s[at + k] = seq[k];
}

int main() {
  static const uint32_t lens[] = {0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5,
                                  5 * 4096 + 7};  // the last one: a second workgroup, its output off the dword grid
  static const uint8_t seq_fill[] = {0xFF, 0xFF, 0xD3}, seq_mark[] = {0xFF, 0xD5}, seq_stuff[] = {0xFF, 0x00},
                       seq_other[] = {0xFF, 0x5A};
  uint32_t cases = 0;
  for (uint32_t n : lens)
    for (uint32_t off = 0; off < 16; off++) {
      std::vector<uint8_t> s(n);
      // random bytes
      for (auto &v : s) v = (uint8_t)rnd();
      run_case(s, off, "random"), cases++;
      // a dense alphabet: every pair and triple of FF / 00 / Dn / other occurs
      for (auto &v : s) {
        static const uint8_t al[] = {0xFF, 0xFF, 0xFF, 0x00, 0x00, 0xD0, 0xD7, 0xD8, 0xCF, 0x5A, 0x01};
        v = al[rnd() % sizeof(al)];
      }
      run_case(s, off, "dense"), cases++;
      // all FF 00, in both phases
      for (uint32_t ph = 0; ph < 2; ph++) {
        for (uint32_t i = 0; i < n; i++) s[i] = ((i + ph) & 1u) ? 0x00 : 0xFF;
        run_case(s, off, "ff00"), cases++;
      }
      // a sequence across every boundary, at every phase, in quiet data
      const struct {
        const uint8_t *seq;
        uint32_t len;
        const char *name;
      } seqs[] = {{seq_stuff, 2, "stuff@edge"}, {seq_fill, 3, "fill+marker@edge"}, {seq_mark, 2, "marker@edge"},
                  {seq_other, 2, "ff+other@edge"}};
      for (const auto &q : seqs)
        for (uint32_t ph = 0; ph < q.len; ph++) {
          for (auto &v : s) v = (uint8_t)(rnd() % 0xC0);  // neither FF nor a marker code
          for (uint32_t p : boundaries(n)) put(s, (int64_t)p - ph, q.seq, q.len);
          run_case(s, off, q.name), cases++;
        }
      if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
      }
    }
  printf("ok %u cases\n", cases);
  return 0;
}
