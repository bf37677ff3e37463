// alph_emu.cpp — the lossy WebP path with context options "webp_lossy" and "webp_alpha" on
// the CPU: the host parser (datago_amd/csrc/host/webp_header.cpp) with the alpha rules on,
// the frame through vp8_emu.cpp's emulation of dg_vp8.h, a VP8L-coded alpha stream through
// vp8l_emu.cpp's environment and the walk of dg_vp8l.h with its ALPH end-of-data rule, and
// the statements of datago_amd/csrc/dg_alph.h over an environment with the 64 lanes as a
// loop, item by item as k_alph_plane runs them.  A stand-alone program for
// tests/test_alph_cpu.py, which builds it with g++ (once plain, once with
// -fsanitize=address,undefined):
//
//   alph_emu --decode OUTDIR FILE...   writes OUTDIR/<n>.out for the n-th file: a line
//                                      "status width height channels why", then the pixels
//   alph_emu --cuts FILE...            every file with its ALPH payload cut by k bytes (every k
//                                      up to 48, then 64 evenly spaced ones) and at 64 evenly
//                                      spaced file lengths; prints "okcut <file> <k>" for an
//                                      ALPH cut that decodes, and a summary line
//
// The two other emulations are compiled into this program as they stand (their source files
// are included, each in a namespace of its own), so the frame and the stream run the code
// their own tests hold to ref_vp8 and ref_webp.  Every source byte is read from an allocation
// of exactly its size, the alpha plane is of exactly width x height bytes, every access is
// checked, and every pixel of the plane must be stored exactly once.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dg_alph.h"
#include "dg_vp8.h"
#include "dg_vp8l.h"
#include "host/webp_header.h"

namespace lossless {
#include "vp8l_emu.cpp"
}
namespace lossy {
#define main vp8_emu_main
#include "vp8_emu.cpp"
#undef main
}

using namespace dg;

namespace {

struct AlphEmu {
  std::vector<uint8_t> raw;          // the raw filtered plane: exactly the payload after the header byte
  const uint32_t *argb = nullptr;    // or the VP8L plane, npx words
  uint32_t npx = 0;
  std::vector<uint8_t> out, stored;
  uint32_t shw[kAlphShWords];
  bool flip = false;

  // The wave's lanes run together: a section whose lanes depended on each other's order would differ
  // between the two directions, which alternate here.
  template <class F>
  void lanes(F f) {
    flip = !flip;
    for (uint32_t k = 0; k < 64u; k++) f(flip ? k : 63u - k);
  }
  template <class F>
  void lanes_sh(F f) {
    lanes(f);
  }
  uint32_t g(uint32_t i) {
    if (argb) {
      if (i >= npx) abort();
      return (argb[i] >> 8) & 255u;
    }
    if (i >= raw.size()) abort();
    return raw[i];
  }
  void put(uint32_t i, uint32_t v) {
    if (i >= out.size() || stored[i] || v > 255u) abort();
    out[i] = (uint8_t)v;
    stored[i] = 1;
  }
  uint32_t get(uint32_t i) {
    if (i >= out.size() || !stored[i]) abort();
    return out[i];
  }
  uint32_t &sh(uint32_t k) {
    if (k >= kAlphShWords) abort();
    return shw[k];
  }
};

void put_le32(std::vector<uint8_t> &v, uint32_t x) {
  for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k)));
}

// The VP8L stream of an ALPH chunk -> the final ARGB plane inside e.work; 0, or 1 / 2 as the library's statuses.
int alpha_stream(lossless::Emu &e, const std::vector<uint8_t> &src, uint32_t W, uint32_t H, uint64_t &plane) {
  const uintptr_t s = (uintptr_t)src.data();
  e.a0 = s & ~(uintptr_t)3;
  e.src_end = s + src.size();
  e.win0 = e.cur = ~0u;
  e.work.assign(vp8l_work_words(W, H), 0xdeadbeefu);
  e.tabs.assign((size_t)vp8l_groups_cap(W, H) * kVp8lGroupWords, 0u);
  Vp8lBits b;
  vp8l_open(e, b, (uint32_t)(s & 3u), (uint32_t)src.size());
  Vp8lWalk o;
  const uint32_t f = vp8l_walk(e, b, W, H, vp8l_groups_cap(W, H), o, true);
  if (f) return f == kVp8lFailGroups ? 1 : 2;
  uint32_t cur = 0;  // k_vp8l_inverse, as vp8l_emu.cpp's webp_decode restates it
  for (uint32_t ti = o.ntrans; ti-- > 0u;) {
    const uint32_t t = o.trans[ti], type = t & 3u, bits = (t >> 2) & 15u, xs = t >> 8;
    const uint64_t px = vp8l_plane_off(W, H, cur);
    const uint32_t np = xs * H;
    if (type == kVp8lPredictor) {
      lossless::emu_predictor(e, px, vp8l_sub_off(W, H, 0u), xs, H, bits);
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
  plane = vp8l_plane_off(W, H, cur);
  return 0;
}

// 0 / 1 (unsupported) / 2 (corrupt); px: width x height x channels
int decode(const uint8_t *d, size_t n, std::vector<uint8_t> &px, uint32_t &W, uint32_t &H, uint32_t &C, const char *&why) {
  Vp8Header h;
  parse_webp_lossy(d, n, h, true);
  why = h.claim ? h.why : "";
  W = H = C = 0;
  if (!h.claim) return 2;
  if (h.status != WH_OK) return h.status;
  // the VP8 chunk as a simple file of its own: what "webp_lossy" alone decodes
  std::vector<uint8_t> simple = {'R', 'I', 'F', 'F'};
  put_le32(simple, 12u + h.chunk_len + (h.chunk_len & 1u));
  for (const char *c = "WEBPVP8 "; *c; c++) simple.push_back((uint8_t)*c);
  put_le32(simple, h.chunk_len);
  simple.insert(simple.end(), d + h.chunk_off, d + h.chunk_off + h.chunk_len);
  if (h.chunk_len & 1u) simple.push_back(0);
  std::vector<uint8_t> rgb;
  const int st = lossy::decode(simple.data(), simple.size(), rgb, W, H, why);
  if (st) return st;
  C = h.has_alph ? 4u : 3u;
  if (!h.has_alph) {
    px = rgb;
    return 0;
  }
  static AlphEmu *ep = nullptr;
  static lossless::Emu *lp = nullptr;
  if (!ep) ep = new AlphEmu();
  if (!lp) lp = new lossless::Emu();
  AlphEmu &e = *ep;
  e.raw.clear();
  e.argb = nullptr;
  e.npx = W * H;
  std::vector<uint8_t> src(d + h.alph_off + 1, d + h.alph_off + h.alph_len);  // an allocation of exactly the payload
  if (alph_compression(h.alph_hdr) == kAlphRaw) {
    e.raw = src;
  } else {
    uint64_t plane = 0;
    const int as = alpha_stream(*lp, src, W, H, plane);
    if (as) {
      why = as == 1 ? "WebP: ALPH stream with more prefix-code groups than the GPU path holds" : "WebP: ALPH lossless stream does not decode";
      return as;
    }
    if (plane + e.npx > lp->work.size()) abort();
    e.argb = lp->work.data() + plane;
  }
  e.out.assign(e.npx, 0xa5);
  e.stored.assign(e.npx, 0);
  for (uint32_t k = 0; k < kAlphShWords; k++) e.shw[k] = 0xdeadbeefu;
  const uint32_t filter = alph_filter(h.alph_hdr);
  for (uint32_t item = alph_items(filter, W, H); item-- > 0u;) alph_unfilter(e, filter, W, H, item);  // the items in no order
  px.resize((size_t)e.npx * 4);
  for (uint32_t i = 0; i < e.npx; i++) {
    if (!e.stored[i]) abort();
    memcpy(&px[(size_t)i * 4], &rgb[(size_t)i * 3], 3);  // k_vp8_rgb with dec_c 4
    px[(size_t)i * 4 + 3] = e.out[i];
  }
  return 0;
}

bool read_all(const char *path, std::vector<uint8_t> &file) { return lossy::read_file(path, file); }

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "--decode")) {
    for (int a = 3; a < argc; a++) {
      std::vector<uint8_t> file, px;
      if (!read_all(argv[a], file)) return 2;
      std::vector<uint8_t> exact(file.begin(), file.end());
      uint32_t W, H, C;
      const char *why = "";
      const int st = decode(exact.data(), exact.size(), px, W, H, C, why);
      const std::string out = std::string(argv[2]) + "/" + std::to_string(a - 3) + ".out";
      FILE *fp = fopen(out.c_str(), "wb");
      if (!fp) return 2;
      fprintf(fp, "%d %u %u %u %s\n", st, W, H, C, why);
      if (st == 0) fwrite(px.data(), 1, px.size(), fp);
      fclose(fp);
    }
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "--cuts")) {
    uint64_t runs = 0, ok = 0, unsup = 0, corrupt = 0, alph_cuts = 0;
    for (int a = 2; a < argc; a++) {
      std::vector<uint8_t> file, px;
      if (!read_all(argv[a], file)) return 2;
      Vp8Header h0;
      parse_webp_lossy(file.data(), file.size(), h0, true);
      uint32_t W, H, C;
      const char *why = "";
      auto run = [&](const std::vector<uint8_t> &cut) {
        const int st = decode(cut.data(), cut.size(), px, W, H, C, why);
        runs++;
        ok += st == 0;
        unsup += st == 1;
        corrupt += st == 2;
        return st;
      };
      const size_t stride = file.size() / 64 + 1;
      for (size_t n = 0;; n = n + stride < file.size() ? n + stride : file.size()) {
        const int st = run(std::vector<uint8_t>(file.begin(), file.begin() + n));  // an allocation of exactly n bytes
        if (st < 0 || st > 2) return 3;
        if (n == file.size()) break;
      }
      if (!h0.has_alph) continue;
      const size_t astride = h0.alph_len / 64 + 1;
      for (size_t k = 1; k <= h0.alph_len; k++) {
        if (k > 48 && k % astride && k != h0.alph_len) continue;
        // the file with the last k bytes of its ALPH payload gone, the chunk and RIFF sizes made to fit
        const uint32_t len = (uint32_t)(h0.alph_len - k), end = h0.alph_off + h0.alph_len + (h0.alph_len & 1u);
        std::vector<uint8_t> cut(file.begin(), file.begin() + h0.alph_off + len);
        if (len & 1u) cut.push_back(0);
        cut.insert(cut.end(), file.begin() + end, file.end());
        const uint32_t riff = (uint32_t)cut.size() - 8u;
        memcpy(cut.data() + 4, &riff, 4);
        memcpy(cut.data() + h0.alph_off - 4, &len, 4);
        alph_cuts++;
        const int st = run(cut);
        if (st < 0 || st > 2) return 3;
        if (st == 0) printf("okcut %s %zu\n", argv[a], k);
      }
    }
    printf("ok runs %llu decoded %llu unsupported %llu corrupt %llu alph_cuts %llu\n", (unsigned long long)runs,
           (unsigned long long)ok, (unsigned long long)unsup, (unsigned long long)corrupt, (unsigned long long)alph_cuts);
    return 0;
  }
  fprintf(stderr, "usage: alph_emu --decode OUTDIR FILE... | --cuts FILE...\n");
  return 2;
}
