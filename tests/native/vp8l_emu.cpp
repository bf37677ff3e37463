// vp8l_emu.cpp — the lossless WebP path of context option "webp" on the CPU: the
// host parser (datago_amd/csrc/host/webp_header.cpp), the wave-uniform walk of
// datago_amd/csrc/dg_vp8l.h over an environment that restates k_vp8l_decode's
// wave-wide steps with the 64 lanes as arrays (source window, table build, copy
// and cache inserts, group maximum, colour-table scan), k_vp8l_inverse's
// transforms (the predictor's wavefront included) and k_vp8l_store.  A shared
// library for tests/test_webp_cpu.py (which compares it with tests/ref_webp.py),
// and with -DVP8L_MAIN a program of its own that runs every file it is given and
// its truncations (see main; built with -fsanitize=address,undefined by the same test).
//
// Every source byte is read from an allocation of exactly the file's size, every
// pixel from a work arena and every table word from a table area of exactly the
// sizes layout_webp gives them, with the kernel's own guards, so a load or store
// outside them is a sanitizer error.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dg_vp8l.h"
#include "host/webp_header.h"

using namespace dg;

namespace {

constexpr uint32_t NL = 64;

struct Emu {
  uintptr_t a0, src_end;
  std::vector<uint32_t> work, tabs;
  uint32_t win[kVp8lWinDwords];
  uint32_t win0 = ~0u, cur = ~0u;
  uint32_t firstL[6][256], cntL[6][16], cl_sorted[32];
  uint32_t cache[1u << kVp8lMaxCache], tag[1u << kVp8lMaxCache];
  uint8_t lens[kVp8lLensBytes];

  uint32_t &W(uint64_t at) {
    if (at >= work.size()) abort();
    return work[at];
  }
  uint32_t &T(uint64_t at) {
    if (at >= tabs.size()) abort();
    return tabs[at];
  }

  uint32_t src_dword(uint32_t i) {
    if (win0 == ~0u || i - win0 >= kVp8lWinDwords) {
      win0 = i;
      for (uint32_t j = 0; j < kVp8lWinDwords; j++) {  // lanes x rounds
        const uintptr_t ad = a0 + 4u * ((uintptr_t)i + j);
        uint32_t v = 0;
        if (ad + 4u <= src_end) {
          memcpy(&v, (const void *)ad, 4);
        } else {
          for (uint32_t q = 0; q < 4; q++)
            if (ad + q < src_end) v |= (uint32_t) * (const uint8_t *)(ad + q) << (8u * q);
        }
        win[j] = v;
      }
    }
    return win[i - win0];
  }
  void lens_fill(uint32_t at, uint32_t n, uint32_t v) {
    for (uint32_t i = 0; i < n; i++)
      if (at + i < kVp8lLensBytes) lens[at + i] = (uint8_t)v;
  }
  uint32_t first(uint32_t k, uint32_t i) { return firstL[k][i]; }
  uint32_t cnt(uint32_t k, uint32_t l) { return cntL[k][l]; }
  uint32_t sorted(uint32_t k, uint32_t i) {
    if (k == 5u) return cl_sorted[i & 31u];
    return T((size_t)cur * kVp8lGroupWords + 5u * 256u + 5u * 16u + kVp8lSortedOff[k] + i);
  }
  bool build(uint32_t k, uint32_t nsym, uint32_t grp) {
    uint32_t cn[16] = {0};
    for (uint32_t i = 0; i < nsym; i++)
      if (lens[i]) cn[lens[i]]++;
    const uint32_t kind = vp8l_code_kind(cn);
    if (!kind) return false;
    for (uint32_t l = 0; l < 16u; l++) cntL[k][l] = cn[l];
    for (uint32_t i = 0; i < 256u; i++) firstL[k][i] = 0u;
    const size_t so = (size_t)grp * kVp8lGroupWords + 5u * 256u + 5u * 16u + (k < 5u ? kVp8lSortedOff[k] : 0u);
    uint32_t code = 0, off = 0;
    for (uint32_t l = 1; l < 16u; l++) {
      code = (code + cn[l - 1u]) << 1;
      if (!cn[l]) continue;
      uint32_t run = 0;
      for (uint32_t base = 0; base < nsym; base += NL) {
        uint64_t m = 0;
        for (uint32_t lane = 0; lane < NL; lane++)
          if (base + lane < nsym && lens[base + lane] == l) m |= 1ull << lane;
        for (uint32_t lane = 0; lane < NL; lane++) {
          if (!((m >> lane) & 1u)) continue;
          const uint32_t sym = base + lane;
          const uint32_t r = run + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
          if (k == 5u)
            cl_sorted[(off + r) & 31u] = sym;
          else
            T(so + off + r) = sym;
          if (kind == 1u) {
            for (uint32_t j = 0; j < 256u; j++) firstL[k][j] = kVp8lValid | sym;
          } else if (l <= 8u) {
            const uint32_t ent = kVp8lValid | (l << 16) | sym;
            for (uint32_t j = vp8l_rev(code + r, l); j < 256u; j += 1u << l) {
              if (firstL[k][j]) abort();  // two codes on one entry: not prefix-free
              firstL[k][j] = ent;
            }
          }
        }
        run += (uint32_t)__builtin_popcountll(m);
      }
      off += cn[l];
    }
    return true;
  }
  void save(uint32_t g) {
    for (uint32_t i = 0; i < 5u * 256u; i++) T((size_t)g * kVp8lGroupWords + i) = (&firstL[0][0])[i];
    for (uint32_t i = 0; i < 5u * 16u; i++) T((size_t)g * kVp8lGroupWords + 5u * 256u + i) = (&cntL[0][0])[i];
    cur = g;
  }
  void select(uint32_t g) {
    if (g == cur) return;
    for (uint32_t i = 0; i < 5u * 256u; i++) (&firstL[0][0])[i] = T((size_t)g * kVp8lGroupWords + i);
    for (uint32_t i = 0; i < 5u * 16u; i++) (&cntL[0][0])[i] = T((size_t)g * kVp8lGroupWords + 5u * 256u + i);
    cur = g;
  }
  void work_store(uint64_t at, uint32_t v) { W(at) = v; }
  uint32_t meta_load(uint64_t at) { return W(at); }
  void cache_clear(uint32_t bits) {
    for (uint32_t i = 0; i < (1u << bits); i++) cache[i] = tag[i] = 0u;
  }
  uint32_t cache_get(uint32_t i) { return cache[i]; }
  void cache_put(uint32_t i, uint32_t v) { cache[i] = v; }
  void copy(uint64_t dst, uint32_t pos, uint32_t dist, uint32_t len, uint32_t cache_bits) {
    for (uint32_t t0 = 0; t0 < len; t0 += NL) {
      uint32_t v[NL], slot[NL];
      bool on[NL];
      for (uint32_t lane = 0; lane < NL; lane++) {  // the step's loads come before its stores
        const uint32_t t = t0 + lane;
        on[lane] = t < len;
        v[lane] = 0;
        if (on[lane]) {
          const uint32_t si = vp8l_copy_src(pos, dist, t);
          if (si >= pos) abort();  // a source inside the copy itself
          v[lane] = W(dst + si);
        }
      }
      for (uint32_t lane = 0; lane < NL; lane++)
        if (on[lane]) W(dst + pos + t0 + lane) = v[lane];
      if (!cache_bits) continue;
      for (uint32_t lane = 0; lane < NL; lane++) {
        slot[lane] = vp8l_cache_slot(v[lane], cache_bits);
        if (on[lane] && tag[slot[lane]] < lane + 1u) tag[slot[lane]] = lane + 1u;  // atomic max
      }
      for (uint32_t lane = 0; lane < NL; lane++)
        if (on[lane] && tag[slot[lane]] == lane + 1u) cache[slot[lane]] = v[lane];
      for (uint32_t lane = 0; lane < NL; lane++)
        if (on[lane]) tag[slot[lane]] = 0u;
    }
  }
  uint32_t max_group(uint64_t at, uint32_t n) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t g = (W(at + i) >> 8) & 0xffffu;
      m = g > m ? g : m;
    }
    return m;
  }
  void pal_delta(uint64_t at, uint32_t n) {
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += NL) {
      uint32_t v[NL];
      for (uint32_t lane = 0; lane < NL; lane++) v[lane] = b0 + lane < n ? W(at + b0 + lane) : 0u;
      for (uint32_t d = 1; d < NL; d <<= 1) {
        uint32_t o[NL];
        for (uint32_t lane = 0; lane < NL; lane++) o[lane] = lane >= d ? v[lane - d] : 0u;
        for (uint32_t lane = 0; lane < NL; lane++)
          if (lane >= d) v[lane] = vp8l_add(v[lane], o[lane]);
      }
      for (uint32_t lane = 0; lane < NL; lane++) {
        v[lane] = vp8l_add(v[lane], carry);
        if (b0 + lane < n) W(at + b0 + lane) = v[lane];
      }
      carry = v[NL - 1];
    }
  }
};

// vp8l_inv_predictor of dg_vp8l.hip, the lanes as arrays.
void emu_predictor(Emu &e, uint64_t px, uint64_t sub, uint32_t w, uint32_t h, uint32_t bits) {
  const uint32_t bw = vp8l_div_up(w, bits), steps = vp8l_strip_steps(w);
  for (uint32_t y0 = 0; y0 < h; y0 += NL) {
    uint32_t h1[NL] = {0}, h2[NL] = {0}, h3[NL] = {0}, firstpx[NL] = {0};
    const bool above = y0 != 0u;  // lane 0
    uint32_t a1 = above ? e.W(px + (uint64_t)(y0 - 1u) * w) : 0u, a2 = 0;
    for (uint32_t t = 0; t < (steps + 7u) / 8u * 8u; t++) {
      uint32_t TRs[NL], Ts[NL], TLs[NL];
      for (uint32_t lane = 0; lane < NL; lane++) {  // the shuffles read the step's old values
        TRs[lane] = lane ? h1[lane - 1] : h1[0];
        Ts[lane] = lane ? h2[lane - 1] : h2[0];
        TLs[lane] = lane ? h3[lane - 1] : h3[0];
      }
      for (uint32_t lane = 0; lane < NL; lane++) {
        const uint32_t y = y0 + lane, x = t - 2u * lane;
        const bool on = y < h && x < w;
        uint32_t TR = TRs[lane], T = Ts[lane], TL = TLs[lane], up = 0;
        if (lane == 0 && above) {
          up = (on && x + 1u < w) ? e.W(px + (uint64_t)(y - 1u) * w + x + 1u) : 0u;
          TR = up;
          T = a1;
          TL = a2;
        }
        uint32_t v = 0;
        if (on) {
          if (x + 1u == w) TR = firstpx[lane];
          uint32_t p;
          if (y == 0u)
            p = x ? h1[lane] : 0xff000000u;
          else if (x == 0u)
            p = T;
          else
            p = vp8l_predict((e.W(sub + (uint64_t)(y >> bits) * bw + (x >> bits)) >> 8) & 15u, h1[lane], T, TL, TR);
          v = vp8l_add(e.W(px + (uint64_t)y * w + x), p);
          e.W(px + (uint64_t)y * w + x) = v;
          if (x == 0u) firstpx[lane] = v;
          if (lane == 0) {
            a2 = a1;
            a1 = up;
          }
        }
        h3[lane] = h2[lane];
        h2[lane] = h1[lane];
        h1[lane] = v;
      }
    }
  }
}

const char *fail_text(uint32_t f) {
  return f == kVp8lFailBits        ? "WebP: image data ends before the image is complete"
         : f == kVp8lFailCode      ? "WebP: prefix code neither complete nor single-symbol"
         : f == kVp8lFailCopy      ? "WebP: copy reaches before the first or past the last pixel"
         : f == kVp8lFailCache     ? "WebP: colour-cache index or size outside the format"
         : f == kVp8lFailTransform ? "WebP: transform used twice"
                                   : "WebP: more prefix-code groups than the GPU path holds";
}

}  // namespace

extern "C" {

// fields: status, extended, alpha, canvas_w, canvas_h, width, height, data_off, nbytes
int webp_parse(const uint8_t *d, size_t n, int64_t *f, const char **why) {
  WebpHeader h;
  parse_webp_header(d, n, h);
  const int64_t v[9] = {h.status, h.extended, h.alpha, h.canvas_w, h.canvas_h, h.width, h.height, h.data_off, (int64_t)h.nbytes};
  memcpy(f, v, sizeof(v));
  *why = h.why;
  return h.status;
}

// The whole path.  out: width x height x (3 or 4) bytes (cap checked).  Returns 0 / 1 (unsupported) / 2 (corrupt).
int webp_decode(const uint8_t *d, size_t n, uint8_t *out, size_t cap, const char **why, int *channels) {
  WebpHeader h;
  parse_webp_header(d, n, h);
  *why = h.why;
  if (h.status != WH_OK) return h.status;
  const uint32_t W = h.width, H = h.height, C = h.alpha ? 4u : 3u;
  *channels = (int)C;
  static Emu *ep = nullptr;
  if (!ep) ep = new Emu();
  Emu &e = *ep;
  const uintptr_t src = (uintptr_t)d + h.data_off;
  e.a0 = src & ~(uintptr_t)3;
  e.src_end = src + (uintptr_t)h.nbytes;
  e.win0 = e.cur = ~0u;
  e.work.assign(vp8l_work_words(W, H), 0xdeadbeefu);
  e.tabs.assign((size_t)vp8l_groups_cap(W, H) * kVp8lGroupWords, 0u);
  Vp8lBits b;
  vp8l_open(e, b, (uint32_t)(src & 3u), (uint32_t)h.nbytes);
  Vp8lWalk o;
  const uint32_t f = vp8l_walk(e, b, W, H, vp8l_groups_cap(W, H), o);
  if (f) {
    *why = fail_text(f);
    return f == kVp8lFailGroups ? 1 : 2;
  }
  uint32_t cur = 0;  // k_vp8l_inverse
  for (uint32_t ti = o.ntrans; ti-- > 0u;) {
    const uint32_t t = o.trans[ti], type = t & 3u, bits = (t >> 2) & 15u, xs = t >> 8;
    const uint64_t px = vp8l_plane_off(W, H, cur);
    const uint32_t np = xs * H;
    if (type == kVp8lPredictor) {
      emu_predictor(e, px, vp8l_sub_off(W, H, 0u), xs, H, bits);
    } else if (type == kVp8lColor) {
      const uint32_t bw = vp8l_div_up(xs, bits);
      for (uint32_t i = 0; i < np; i++) {
        const uint32_t y = i / xs, x = i - y * xs;
        e.W(px + i) = vp8l_color_inv(e.W(vp8l_sub_off(W, H, 1u) + (y >> bits) * bw + (x >> bits)), e.W(px + i));
      }
    } else if (type == kVp8lGreenT) {
      for (uint32_t i = 0; i < np; i++) e.W(px + i) = vp8l_green_inv(e.W(px + i));
    } else {
      const uint64_t dst = vp8l_plane_off(W, H, cur ^ 1u);
      const uint32_t pw = vp8l_div_up(xs, bits);
      for (uint32_t i = 0; i < np; i++) {
        const uint32_t y = i / xs, x = i - y * xs;
        const uint32_t k = vp8l_index_of(e.W(px + y * pw + (x >> bits)), x, bits);
        e.W(dst + i) = k < o.npal ? e.W(vp8l_pal_off(W, H) + k) : 0u;
      }
      cur ^= 1u;
    }
  }
  if ((size_t)W * H * C > cap) return -1;
  for (uint32_t i = 0; i < W * H; i++) {  // k_vp8l_store
    const uint32_t p = e.W(vp8l_plane_off(W, H, cur) + i);
    out[(size_t)i * C + 0] = (uint8_t)(p >> 16);
    out[(size_t)i * C + 1] = (uint8_t)(p >> 8);
    out[(size_t)i * C + 2] = (uint8_t)p;
    if (C == 4u) out[(size_t)i * C + 3] = (uint8_t)(p >> 24);
  }
  return 0;
}

}  // extern "C"

#ifdef VP8L_MAIN
// Every file through the parser and the emulator at every length (a cut that the file's own RIFF size
// refuses at once), and, since only that gets past the RIFF check into the bitstream walk, at its cuts
// with the RIFF and chunk sizes made to fit, so that the bitstream itself ends early: every such length
// of the files named after --dense, 64 evenly spaced ones of the files named after --sampled.
int main(int argc, char **argv) {
  uint64_t runs = 0, ok = 0, unsup = 0, corrupt = 0, fitted = 0;
  bool dense = false;
  for (int a = 1; a < argc; a++) {
    if (!strcmp(argv[a], "--dense") || !strcmp(argv[a], "--sampled")) {
      dense = argv[a][2] == 'd';
      continue;
    }
    FILE *fp = fopen(argv[a], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(fp);
    WebpHeader h0;
    parse_webp_header(file.data(), file.size(), h0);
    const size_t stride = dense ? 1 : file.size() / 64 + 1;
    for (size_t n = 0; n <= file.size(); n++)
      for (int fit = 0; fit < 2; fit++) {
        if (fit && (h0.status != WH_OK || n < h0.data_off || n == file.size() || (n - h0.data_off) % stride)) continue;
        std::vector<uint8_t> cut(file.begin(), file.begin() + n);  // an allocation of exactly n bytes
        if (fit) {
          const uint32_t riff = (uint32_t)(n - 8), len = (uint32_t)(n - h0.data_off + 5);
          memcpy(cut.data() + 4, &riff, 4);
          memcpy(cut.data() + h0.data_off - 9, &len, 4);
          fitted++;
        }
        WebpHeader h;
        parse_webp_header(cut.data(), cut.size(), h);
        std::vector<uint8_t> px(h.status == WH_OK ? (size_t)h.width * h.height * 4 : 0);
        const char *why = "";
        int ch = 0;
        const int st = webp_decode(cut.data(), cut.size(), px.data(), px.size(), &why, &ch);
        runs++;
        ok += st == 0;
        unsup += st == 1;
        corrupt += st == 2;
        if (st < 0 || st > 2) return 3;
      }
  }
  printf("ok runs %llu decoded %llu unsupported %llu corrupt %llu fitted %llu\n", (unsigned long long)runs,
         (unsigned long long)ok, (unsigned long long)unsup, (unsigned long long)corrupt, (unsigned long long)fitted);
  return 0;
}
#endif
