// gif_emu.cpp — the GIF path of context option "gif" on the CPU: the host
// parser (datago_amd/csrc/host/gif_header.cpp), k_gif_gather's address rule,
// k_gif_lzw's step with its 64 lanes as arrays over the lane routines of
// datago_amd/csrc/dg_gif.h, and k_gif_expand's placement.  A shared library
// for tests/test_gif_cpu.py (which compares it with tests/ref_gif.py), and with
// -DGIF_MAIN a program of its own that runs every file it is given and each of
// its truncations (built with -fsanitize=address,undefined by the same test).
//
// Every source byte is read from an allocation of exactly the file's size and
// every index from one of exactly fw x fh bytes, with the kernel's own guards,
// so a load or store outside them is a sanitizer error.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dg_gif.h"
#include "host/gif_header.h"

using namespace dg;

namespace {

constexpr uint32_t NL = 64;

uint32_t excl_scan(const uint32_t v[NL], uint32_t out[NL]) {
  uint32_t s = 0;
  for (uint32_t j = 0; j < NL; j++) {
    out[j] = s;
    s += v[j];
  }
  return s;
}

int ctz64(uint64_t m) { return m ? __builtin_ctzll(m) : 64; }

// k_gif_lzw: src / src_end / blocked as GifDesc's, out = fw x fh bytes.  Returns kGifFail* or 0.
uint32_t emu_lzw(const uint8_t *src, const uint8_t *src_end, uint32_t blocked, uint32_t nbytes, uint32_t mcs,
                 uint32_t npix, uint8_t *out, uint64_t *steps_out) {
  std::vector<uint32_t> tpos(kGifMaxCodes, 0xFFFFFFFFu);
  std::vector<uint16_t> tlen(kGifMaxCodes, 0);
  uint8_t win[kGifWinBytes];
  const uint32_t nbits = nbytes * 8u, clear = 1u << mcs, w0 = mcs + 1u;
  GifLzw s = {0u, clear + 2u, 0u, 0u, 0u, 0u};
  uintptr_t win_addr = 0;
  bool win_valid = false;
  uint32_t fail = 0;
  const uint32_t max_steps = nbits / w0 + 2u;
  uint64_t steps = 0;
  for (uint32_t step = 0; step < max_steps && s.o < npix; step++) {
    steps++;
    if (nbytes) {
      const uint32_t k0 = s.bitpos >> 3;
      uint32_t k1 = ((s.bitpos + kGifStepBits) >> 3) + 3u;
      k1 = k1 < nbytes ? k1 : nbytes - 1u;
      if (k0 <= k1) {
        const uintptr_t a0 = (uintptr_t)src + gif_src_index(k0, blocked), a1 = (uintptr_t)src + gif_src_index(k1, blocked);
        if (!win_valid || a0 < win_addr || a1 >= win_addr + kGifWinBytes) {
          win_addr = a0 & ~(uintptr_t)3;
          win_valid = true;
          for (uint32_t i = 0; i < kGifWinBytes / 4u; i++) {
            const uintptr_t ad = win_addr + 4u * i;
            uint32_t v = 0;
            if (ad + 4u <= (uintptr_t)src_end) {
              memcpy(&v, (const void *)ad, 4);
            } else {
              for (uint32_t q = 0; q < 4; q++)
                if (ad + q < (uintptr_t)src_end) v |= (uint32_t) * (const uint8_t *)(ad + q) << (8u * q);
            }
            memcpy(win + 4u * i, &v, 4);
          }
        }
      }
    }
    const uint32_t a = s.pv ? 0u : 1u;
    uint32_t nfj[NL], wj[NL], offj[NL], c[NL];
    bool inb[NL];
    for (uint32_t j = 0; j < NL; j++) {
      nfj[j] = gif_lane_nf(s.nf, a, j);
      wj[j] = gif_width(nfj[j], w0);
    }
    const uint32_t wsum = excl_scan(wj, offj);
    uint64_t stopm = 0;
    for (uint32_t j = 0; j < NL; j++) {
      offj[j] += s.bitpos;
      inb[j] = offj[j] + wj[j] <= nbits;
      c[j] = 0;
      if (inb[j]) {
        const uint32_t kb0 = offj[j] >> 3;
        uint32_t v = 0;
        for (uint32_t q = 0; q < 3; q++) {
          const uint32_t kq = kb0 + q;
          if (kq < nbytes) {
            const uintptr_t wi = (uintptr_t)src + gif_src_index(kq, blocked) - win_addr;
            if (wi >= kGifWinBytes) abort();  // the window rule failed
            v |= (uint32_t)win[wi] << (8u * q);
          }
        }
        c[j] = (v >> (offj[j] & 7u)) & ((1u << wj[j]) - 1u);
      }
      const bool special = inb[j] && (c[j] == clear || c[j] == clear + 1u);
      if (special || !inb[j]) stopm |= 1ull << j;
    }
    const uint32_t k = (uint32_t)ctz64(stopm);
    uint64_t badm = 0;
    for (uint32_t j = 0; j < k; j++)
      if (gif_code_bad(c[j], nfj[j], j, a)) badm |= 1ull << j;
    const uint32_t kb = (uint32_t)ctz64(badm);
    const uint32_t kv = k < kb ? k : kb;
    bool act[NL], lit[NL], old[NL], neu[NL], res[NL], prev_src[NL];
    uint32_t L[NL], S[NL], ci[NL], sl[NL], lev[NL];
    for (uint32_t j = 0; j < NL; j++) {
      act[j] = j < kv;
      lit[j] = act[j] && c[j] < clear;
      old[j] = act[j] && !lit[j] && c[j] < s.nf;
      neu[j] = act[j] && !lit[j] && !old[j];
      if (old[j] && tpos[c[j]] == 0xFFFFFFFFu) abort();  // an entry never written
      L[j] = lit[j] ? 1u : old[j] ? (uint32_t)tlen[c[j]] : 0u;
      S[j] = old[j] ? tpos[c[j]] : 0u;
      ci[j] = neu[j] ? gif_creator(c[j], s.nf, a) : 0u;
      if (ci[j] > j) abort();
      prev_src[j] = ci[j] == 0u;
      sl[j] = prev_src[j] ? 0u : ci[j] - 1u;
      lev[j] = 0;
      res[j] = !neu[j];
    }
    for (uint32_t r = 0; r < 64u; r++) {
      bool any = false;
      for (uint32_t j = 0; j < NL; j++) any |= !res[j];
      if (!any) break;
      uint32_t Lm[NL], levm[NL], levi[NL];
      bool resm[NL], resi[NL];
      for (uint32_t j = 0; j < NL; j++) {  // the shuffles read the round's old values
        Lm[j] = L[sl[j]];
        levm[j] = lev[sl[j]];
        resm[j] = res[sl[j]];
        levi[j] = lev[ci[j]];
        resi[j] = res[ci[j]];
      }
      for (uint32_t j = 0; j < NL; j++) {
        if (res[j]) continue;
        const bool okm = prev_src[j] || resm[j], oki = ci[j] >= j || resi[j];
        if (okm && oki) {
          L[j] = (prev_src[j] ? s.plen : Lm[j]) + 1u;
          const uint32_t l0 = prev_src[j] ? 0u : levm[j] + 1u, l1 = ci[j] < j ? levi[j] + 1u : 0u;
          lev[j] = l0 > l1 ? l0 : l1;
          res[j] = true;
        }
      }
    }
    for (uint32_t j = 0; j < NL; j++) {
      if (!res[j]) abort();  // 64 rounds always settle
      if (!act[j]) L[j] = 0u;
    }
    uint32_t P[NL];
    const uint32_t total = excl_scan(L, P);
    bool kw[NL];
    for (uint32_t j = 0; j < NL; j++) P[j] += s.o;
    for (uint32_t j = 0; j < NL; j++) {
      if (neu[j]) S[j] = prev_src[j] ? s.ppos : P[sl[j]];
      kw[j] = neu[j] && ci[j] == j;
    }
    const bool done_after = s.o + total >= npix;
    if (!done_after) {
      if (kb < k) {
        fail = kGifFailCode;
        break;
      }
      if (k < 64u && (!inb[k] || c[k] == clear + 1u)) {
        fail = kGifFailShort;
        break;
      }
    }
    for (uint32_t j = 0; j < NL; j++) {
      const uint32_t E = s.nf + j - a;
      if (act[j] && j >= a && E < kGifMaxCodes) {
        tpos[E] = j ? P[j - 1] : s.ppos;
        tlen[E] = (uint16_t)((j ? L[j - 1] : s.plen) + 1u);
      }
    }
    uint32_t CL[NL];
    for (uint32_t j = 0; j < NL; j++) {
      const uint32_t room = P[j] < npix ? npix - P[j] : 0u;
      CL[j] = L[j] < room ? L[j] : room;
    }
    // bytes written by this step's levels so far: a level may only read what is older
    std::vector<uint8_t> fresh;
    for (uint32_t lv = 0; lv < 64u; lv++) {
      std::vector<std::pair<uint32_t, uint8_t>> stores;  // the level's stores land after its loads
      for (uint32_t j = 0; j < NL; j++) {
        if (!(CL[j] > 0u && lev[j] == lv)) continue;
        for (uint32_t t = 0; t < CL[j]; t++) {
          uint8_t v;
          if (lit[j]) {
            v = (uint8_t)c[j];
          } else {
            const uint32_t si = S[j] + gif_copy_index(t, L[j], kw[j]);
            if (si >= P[j] || si >= npix) abort();  // a source at or past the string itself
            v = out[si];
          }
          stores.push_back({P[j] + t, v});
        }
      }
      for (auto &st : stores) {
        if (st.first >= npix) abort();
        out[st.first] = st.second;
      }
      bool more = false;
      for (uint32_t j = 0; j < NL; j++) more |= CL[j] > 0u && lev[j] > lv;
      if (!more) break;
    }
    s.o = done_after ? npix : s.o + total;
    if (kv == 64u) {
      s.nf = gif_lane_nf(s.nf, a, 64u);
      s.pv = 1u;
      s.ppos = P[63];
      s.plen = L[63];
      s.bitpos += wsum;
    } else if (!done_after) {
      s.nf = clear + 2u;
      s.pv = 0u;
      s.bitpos = offj[k] + wj[k];
    }
  }
  if (!fail && s.o < npix) fail = kGifFailShort;
  if (steps_out) *steps_out = steps;
  return fail;
}

const char *fail_text(uint32_t f) {
  return f == kGifFailCode    ? "GIF: LZW code above the next free code"
         : f == kGifFailShort ? "GIF: image data ends before the frame is complete"
                              : "GIF: pixel index past the colour table";
}

}  // namespace

extern "C" {

// fields: status, version, width, height, left, top, fw, fh, interlace, has_global, has_local, npal,
// transparent, min_code_size, data_off, nbytes, closed, nruns
int gif_parse(const uint8_t *d, size_t n, int64_t *f, uint8_t *pal, const char **why) {
  GifHeader h;
  parse_gif_header(d, n, h);
  const int64_t v[18] = {h.status, h.version, h.width, h.height, h.left, h.top, h.fw, h.fh, h.interlace,
                         h.has_global, h.has_local, h.npal, h.transparent, h.min_code_size, h.data_off,
                         (int64_t)h.nbytes, h.closed ? 1 : 0, (int64_t)h.runs.size()};
  memcpy(f, v, sizeof(v));
  if (pal) memcpy(pal, h.pal, 1024);
  *why = h.why;
  return h.status;
}

// The whole path.  rgba: width x height x 4 bytes (cap checked).  Returns 0 / 1 (unsupported) / 2 (corrupt).
int gif_decode(const uint8_t *d, size_t n, uint8_t *rgba, size_t cap, const char **why, uint64_t *steps) {
  GifHeader h;
  parse_gif_header(d, n, h);
  *why = h.why;
  if (steps) *steps = 0;
  if (h.status != GH_OK) return h.status;
  const uint32_t npix = h.fw * h.fh;
  std::vector<uint8_t> gathered;
  const uint8_t *src, *src_end;
  if (h.closed) {
    src = d + h.data_off;
    src_end = src + (h.nbytes ? gif_src_index((uint32_t)h.nbytes - 1u, 1u) + 1u : 0u);
  } else {  // k_gif_gather
    gathered.resize(h.nbytes);
    size_t zo = 0;
    for (const GifRun &r : h.runs) {
      const uint32_t total = r.len * r.count;
      for (uint32_t t = 0; t < total; t++) {
        const uint32_t blk = t / r.len, q = t - blk * r.len;
        gathered[zo + t] = d[(size_t)r.off + (size_t)blk * (r.len + 1u) + 1u + q];
      }
      zo += total;
    }
    src = gathered.data();
    src_end = src + h.nbytes;
  }
  std::vector<uint8_t> idx(npix);
  const uint32_t f = emu_lzw(src, src_end, h.closed ? 1u : 0u, (uint32_t)h.nbytes, (uint32_t)h.min_code_size, npix,
                             idx.data(), steps);
  if (f) {
    *why = fail_text(f);
    return 1;
  }
  if ((size_t)h.width * h.height * 4 > cap) return -1;
  bool past = false;
  for (uint32_t y = 0; y < h.height; y++)
    for (uint32_t x = 0; x < h.width; x++) {  // k_gif_expand
      const uint32_t fx = x - h.left, fy = y - h.top;
      uint8_t v[4] = {0, 0, 0, 0};
      if (fx < h.fw && fy < h.fh) {
        const uint32_t i = idx[(size_t)gif_stream_row(fy, h.fh, (uint32_t)h.interlace) * h.fw + fx];
        if (i < (uint32_t)h.npal)
          memcpy(v, h.pal[i], 4);
        else
          past = true;
      }
      memcpy(rgba + ((size_t)y * h.width + x) * 4, v, 4);
    }
  if (past) {
    *why = fail_text(kGifFailPalette);
    return 1;
  }
  return 0;
}

}  // extern "C"

#ifdef GIF_MAIN
// Every file and every one of its truncations through the parser and the emulator.
int main(int argc, char **argv) {
  uint64_t runs = 0, ok = 0, unsup = 0, corrupt = 0;
  for (int a = 1; a < argc; a++) {
    FILE *fp = fopen(argv[a], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(fp);
    std::vector<size_t> cuts;  // every length; of a large file 64 of them and the whole
    const size_t stride = file.size() <= 3000 ? 1 : file.size() / 64 + 1;
    for (size_t n = 0; n < file.size(); n += stride) cuts.push_back(n);
    cuts.push_back(file.size());
    for (size_t n : cuts) {
      std::vector<uint8_t> cut(file.begin(), file.begin() + n);  // an allocation of exactly n bytes
      GifHeader h;
      parse_gif_header(cut.data(), cut.size(), h);
      std::vector<uint8_t> rgba(h.status == GH_OK ? (size_t)h.width * h.height * 4 : 0);
      const char *why = "";
      const int st = gif_decode(cut.data(), cut.size(), rgba.data(), rgba.size(), &why, nullptr);
      runs++;
      ok += st == 0;
      unsup += st == 1;
      corrupt += st == 2;
      if (st < 0 || st > 2) return 3;
    }
  }
  printf("ok runs %llu decoded %llu unsupported %llu corrupt %llu\n", (unsigned long long)runs,
         (unsigned long long)ok, (unsigned long long)unsup, (unsigned long long)corrupt);
  return 0;
}
#endif
