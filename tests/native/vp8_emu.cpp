// vp8_emu.cpp — the lossy WebP path of context option "webp_lossy" on the CPU: the host
// parser (datago_amd/csrc/host/webp_header.cpp) and the walk of datago_amd/csrc/dg_vp8.h
// over an environment with the 64 lanes as a loop, in the kernels' order: k_vp8_parse,
// then k_vp8_recon and k_vp8_filter over the anti-diagonals x + 2y = d with the MBs of a
// diagonal in turn, then k_vp8_rgb.  A stand-alone program for tests/test_vp8_cpu.py,
// which builds it with g++ (once plain, once with -fsanitize=address,undefined):
//
//   vp8_emu --decode OUTDIR FILE...   writes OUTDIR/<n>.out for the n-th file: a line
//                                     "status width height why", then the RGB8 pixels
//   vp8_emu --cuts [--dense|--sampled] FILE...
//                                     every file at its cut lengths, plain and with the RIFF,
//                                     chunk and first-partition sizes made to fit; a cut that
//                                     decodes must give the whole file's pixels; prints a
//                                     summary line and "okcut <file> <length> <fit>" lines
//
// The source is read from an allocation of exactly the file's size and the arena is of
// exactly layout_vp8's size, every access checked, so a load or store outside them aborts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dg_vp8.h"
#include "host/webp_header.h"

using namespace dg;

namespace {

struct Emu {
  Vp8ParseState s;
  const uint8_t *chunk = nullptr;
  uint32_t nbytes = 0;
  std::vector<uint8_t> work;

  uint32_t src8(uint32_t i) {
    if (i >= nbytes) abort();
    return chunk[i];
  }
  uint32_t src_be32(uint32_t i) {
    if ((uint64_t)i + 4u > nbytes) abort();
    return ((uint32_t)chunk[i] << 24) | ((uint32_t)chunk[i + 1] << 16) | ((uint32_t)chunk[i + 2] << 8) | chunk[i + 3];
  }
  template <class F>
  void lanes(F f) {
    for (uint32_t lane = 0; lane < 64u; lane++) f(lane);
  }
  uint8_t &A(uint64_t off) {
    if (off >= work.size()) abort();
    return work[off];
  }
  uint32_t r8(uint64_t off) { return A(off); }
  int32_t r16(uint64_t off) {
    if (off & 1u) abort();
    return (int16_t)(uint16_t)(A(off) | (A(off + 1) << 8));
  }
  void w8(uint64_t off, uint32_t v) { A(off) = (uint8_t)v; }
  void w32(uint64_t off, uint32_t v) {
    if (off & 3u) abort();
    for (uint32_t k = 0; k < 4u; k++) A(off + k) = (uint8_t)(v >> (8u * k));
  }
};

const char *fail_text(uint32_t f) {
  return f == kVp8FailBits ? "WebP: VP8 data ends before the image is complete"
                           : "WebP: VP8 token-partition table reaches past the chunk";
}

// 0 / 1 (unsupported) / 2 (corrupt); px: width x height x 3
int decode(const uint8_t *d, size_t n, std::vector<uint8_t> &px, uint32_t &W, uint32_t &H, const char *&why) {
  Vp8Header h;
  parse_webp_lossy(d, n, h);
  why = h.claim ? h.why : "";
  W = H = 0;
  if (!h.claim) return 2;
  if (h.status != WH_OK) return h.status;
  W = h.width;
  H = h.height;
  if ((uint64_t)W * H * 4ull >= (1ull << 31) || h.chunk_len >= (1u << 28)) {
    why = "WebP: image too large for the GPU path";
    return 1;
  }
  static Emu *ep = nullptr;
  if (!ep) ep = new Emu();
  Emu &e = *ep;
  e.chunk = d + h.chunk_off;
  e.nbytes = h.chunk_len;
  const Vp8Layout L = layout_vp8(W, H);
  e.work.assign(L.bytes, 0xa5);
  Vp8Frame fr;
  const uint32_t f = vp8_parse(e, W, H, h.chunk_len, h.part0, fr);
  if (f) {
    why = fail_text(f);
    return 2;
  }
  static Vp8ReconBuf B;
  const uint32_t nd = vp8_diag_count(L.mbw, L.mbh);
  for (uint32_t pass = 0; pass < 2u; pass++) {
    if (pass == 1u && !fr.filter_type) break;
    for (uint32_t dgl = 0; dgl < nd; dgl++) {
      uint32_t y0, cnt;
      vp8_diag_rows(L.mbw, L.mbh, dgl, y0, cnt);
      for (uint32_t k = 0; k < cnt; k++) {
        const uint32_t my = y0 + k, mx = dgl - 2u * my;
        if (mx >= L.mbw || my >= L.mbh) abort();
        if (pass == 0u)
          vp8_recon_mb(e, B, L, mx, my);
        else
          vp8_filter_mb(e, L, fr.filter_type, mx, my);
      }
    }
  }
  px.resize((size_t)W * H * 3);
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const uint32_t p = vp8_rgb_px(e, L, W, H, x, y);
      uint8_t *o = &px[((size_t)y * W + x) * 3];
      o[0] = (uint8_t)p;
      o[1] = (uint8_t)(p >> 8);
      o[2] = (uint8_t)(p >> 16);
    }
  return 0;
}

bool read_file(const char *path, std::vector<uint8_t> &file) {
  FILE *fp = fopen(path, "rb");
  if (!fp) return false;
  uint8_t buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) file.insert(file.end(), buf, buf + got);
  fclose(fp);
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "--decode")) {
    for (int a = 3; a < argc; a++) {
      std::vector<uint8_t> file, px;
      if (!read_file(argv[a], file)) return 2;
      std::vector<uint8_t> exact(file.begin(), file.end());
      uint32_t W, H;
      const char *why = "";
      const int st = decode(exact.data(), exact.size(), px, W, H, why);
      const std::string out = std::string(argv[2]) + "/" + std::to_string(a - 3) + ".out";
      FILE *fp = fopen(out.c_str(), "wb");
      if (!fp) return 2;
      fprintf(fp, "%d %u %u %s\n", st, W, H, why);
      if (st == 0) fwrite(px.data(), 1, px.size(), fp);
      fclose(fp);
    }
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "--cuts")) {
    uint64_t runs = 0, ok = 0, unsup = 0, corrupt = 0, fitted = 0;
    bool dense = false;
    for (int a = 2; a < argc; a++) {
      if (!strcmp(argv[a], "--dense") || !strcmp(argv[a], "--sampled")) {
        dense = argv[a][2] == 'd';
        continue;
      }
      std::vector<uint8_t> file, full, px;
      if (!read_file(argv[a], file)) return 2;
      Vp8Header h0;
      parse_webp_lossy(file.data(), file.size(), h0);
      uint32_t W, H;
      const char *why = "";
      const int st0 = decode(file.data(), file.size(), full, W, H, why);
      const size_t stride = dense ? 1 : file.size() / 64 + 1;
      for (size_t n = 0; n <= file.size(); n++) {
        if (!dense && n % stride && n != file.size()) continue;
        for (int fit = 0; fit < 2; fit++) {
          // fitted: the sizes say what is there, so the cut is met inside the bool-coded data
          if (fit && (h0.status != WH_OK || n < h0.chunk_off + 10u || n == file.size())) continue;
          std::vector<uint8_t> cut(file.begin(), file.begin() + n);  // an allocation of exactly n bytes
          if (fit) {
            const uint32_t riff = (uint32_t)(n - 8), len = (uint32_t)(n - h0.chunk_off);
            memcpy(cut.data() + 4, &riff, 4);
            memcpy(cut.data() + h0.chunk_off - 4, &len, 4);
            if (h0.part0 > len - 10u) {  // the first partition is what is left
              const uint32_t tag = (uint32_t)cut[h0.chunk_off] | ((uint32_t)cut[h0.chunk_off + 1] << 8) |
                                   ((uint32_t)cut[h0.chunk_off + 2] << 16);
              const uint32_t t2 = (tag & 31u) | ((len - 10u) << 5);
              cut[h0.chunk_off] = (uint8_t)t2;
              cut[h0.chunk_off + 1] = (uint8_t)(t2 >> 8);
              cut[h0.chunk_off + 2] = (uint8_t)(t2 >> 16);
            }
            fitted++;
          }
          const int st = decode(cut.data(), cut.size(), px, W, H, why);
          runs++;
          ok += st == 0;
          unsup += st == 1;
          corrupt += st == 2;
          if (st < 0 || st > 2) return 3;
          if (st == 0 && n != file.size()) {
            if (st0 != 0 || px != full) {
              printf("DIFF %s %zu %d\n", argv[a], n, fit);
              return 4;
            }
            printf("okcut %s %zu %d\n", argv[a], n, fit);
          }
        }
      }
    }
    printf("ok runs %llu decoded %llu unsupported %llu corrupt %llu fitted %llu\n", (unsigned long long)runs,
           (unsigned long long)ok, (unsigned long long)unsup, (unsigned long long)corrupt, (unsigned long long)fitted);
    return 0;
  }
  fprintf(stderr, "usage: vp8_emu --decode OUTDIR FILE... | --cuts [--dense|--sampled] FILE...\n");
  return 2;
}
