// dg_gif.hip — CDNA4 (gfx950) kernels of the GIF decode stage (option "gif").
//
//   k_gif_gather   data sub-blocks -> one contiguous LZW code stream (only for a
//                  chain that is not 255, 255, .., last: that one is read in place)
//   k_gif_lzw      LZW codes -> the frame's index plane, one wave per image
//   k_gif_expand   indices -> Rgba8 on the logical screen (palette, de-interlace,
//                  frame offset, clipping, transparent black outside the frame)
//
// What they restate: gif 0.13 + weezl as image 0.25's GifDecoder drives them for
// load_from_memory (the first frame composited on the screen); dg_gif.h holds the
// lane routines and the scheme, tests/ref_gif.py the CPU restatement the tests
// compare to.
//
// LZW is a serial code stream, but only through two things: the bit offset of a
// code (its width depends on how many came before) and the strings of entries
// made a moment ago.  k_gif_lzw takes 64 codes per step: widths and offsets are
// closed-form per lane, entries are (position, length) in the output already
// written, and a code whose entry was made inside the step takes its length
// from the lane that made it.  Strings are copied level by level: level 0 reads
// only what earlier steps wrote, level n + 1 what level n wrote.  Between levels
// the wave waits for its stores and reads back with loads that bypass the L1
// (a plain load could hit a line fetched before the store).
//
// Every loop is bounded by the stream's bit count and the frame's pixel count:
// a step consumes at least one code or ends the decode.
#include <hip/hip_runtime.h>

#include "dg_gif.h"
#include "kernels.h"

namespace dg {

// ------------------------------------------------------------ gather

// One piece (kGatherPiece bytes) of a run of `count` sub-blocks of `len` bytes.
__global__ __launch_bounds__(256) void k_gif_gather(const GatherJob *__restrict__ jobs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  const GatherJob j = jobs[it.image];
  const uint32_t total = j.len * j.count;
  const uint32_t b0 = it.item0 * kGatherPiece;
  const uint32_t e = total - b0 < kGatherPiece ? total : b0 + kGatherPiece;
  const DG_GLOBAL uint8_t *s = gp<const uint8_t>(j.src);
  DG_GLOBAL uint8_t *d = gp<uint8_t>(j.dst);
  for (uint32_t t = b0 + threadIdx.x; t < e; t += 256) {
    const uint32_t blk = t / j.len, r = t - blk * j.len;
    d[t] = s[(size_t)blk * (j.len + 1u) + 1u + r];
  }
}

// ------------------------------------------------------------ LZW

__device__ __forceinline__ uint32_t gif_excl_scan(uint32_t v, uint32_t lane, uint32_t *total) {
  uint32_t x = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  *total = __shfl(x, 63);
  return x - v;
}

// A byte the wave itself stored earlier (after gif_drain): past the L1.
__device__ __forceinline__ uint32_t gif_ld(const DG_GLOBAL uint8_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The wave's stores have reached the L2 before any later load is issued.  (Only
// this wave reads them back: nothing has to leave this XCD's L2.)
__device__ __forceinline__ void gif_drain() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(64) void k_gif_lzw(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  __shared__ uint32_t tpos[kGifMaxCodes];
  __shared__ uint16_t tlen[kGifMaxCodes];
  __shared__ __attribute__((aligned(16))) uint8_t win[kGifWinBytes];
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const GifDesc g = im.gif;
  const uint32_t lane = threadIdx.x;
  const uint32_t nbytes = g.nbytes, nbits = nbytes * 8u, npix = g.fw * g.fh;
  const uint32_t clear = 1u << g.mcs, w0 = g.mcs + 1u;
  DG_GLOBAL uint8_t *out = gp<uint8_t>(g.idx);
  GifLzw s = {0u, clear + 2u, 0u, 0u, 0u, 0u};
  uint64_t win_addr = 0;
  bool win_valid = false;
  uint32_t fail = 0;
  const uint32_t max_steps = nbits / w0 + 2u;
  for (uint32_t step = 0; step < max_steps && s.o < npix; step++) {
    // ---- the source window: the bytes this step's codes can touch
    if (nbytes) {
      const uint32_t k0 = s.bitpos >> 3;
      uint32_t k1 = ((s.bitpos + kGifStepBits) >> 3) + 3u;  // a code's three bytes from its last bit offset
      k1 = k1 < nbytes ? k1 : nbytes - 1u;
      if (k0 <= k1) {
        const uint64_t a0 = g.src + gif_src_index(k0, g.blocked), a1 = g.src + gif_src_index(k1, g.blocked);
        if (!win_valid || a0 < win_addr || a1 >= win_addr + kGifWinBytes) {
          __syncthreads();
          win_addr = a0 & ~3ull;
          win_valid = true;
#pragma unroll
          for (uint32_t r = 0; r < kGifWinBytes / 256u; r++) {
            const uint32_t i = lane + 64u * r;
            const uint64_t ad = win_addr + 4ull * i;
            uint32_t v = 0;
            if (ad + 4u <= g.src_end) {
              v = *gp<const uint32_t>(ad);
            } else {
              for (uint32_t q = 0; q < 4; q++)
                if (ad + q < g.src_end) v |= (uint32_t)*gp<const uint8_t>(ad + q) << (8u * q);
            }
            ((uint32_t *)win)[i] = v;
          }
          __syncthreads();
        }
      }
    }
    // ---- widths, bit offsets, codes
    const uint32_t a = s.pv ? 0u : 1u;
    const uint32_t nfj = gif_lane_nf(s.nf, a, lane);
    const uint32_t wj = gif_width(nfj, w0);
    uint32_t wsum;
    const uint32_t offj = s.bitpos + gif_excl_scan(wj, lane, &wsum);
    const bool inb = offj + wj <= nbits;
    uint32_t c = 0;
    if (inb) {
      const uint32_t kb0 = offj >> 3;
      uint32_t v = 0;
#pragma unroll
      for (uint32_t q = 0; q < 3; q++) {
        const uint32_t kq = kb0 + q;
        if (kq < nbytes) v |= (uint32_t)win[(uint32_t)(g.src + gif_src_index(kq, g.blocked) - win_addr)] << (8u * q);
      }
      c = (v >> (offj & 7u)) & ((1u << wj) - 1u);
    }
    const bool special = inb && (c == clear || c == clear + 1u);
    const uint64_t stopm = __ballot(special || !inb);
    const uint32_t k = stopm ? (uint32_t)__builtin_ctzll(stopm) : 64u;
    const uint64_t badm = __ballot(lane < k && gif_code_bad(c, nfj, lane, a));
    const uint32_t kb = badm ? (uint32_t)__builtin_ctzll(badm) : 64u;
    const uint32_t kv = k < kb ? k : kb;  // lanes below kv hold data codes
    const bool act = lane < kv;
    const bool lit = act && c < clear;
    const bool old = act && !lit && c < s.nf;
    const bool neu = act && !lit && !old;  // an entry created inside this step
    // ---- string lengths and copy levels
    uint32_t L = lit ? 1u : old ? (uint32_t)tlen[c] : 0u;
    uint32_t S = old ? tpos[c] : 0u;
    const uint32_t ci = neu ? gif_creator(c, s.nf, a) : 0u;  // <= lane
    const bool prev_src = ci == 0u;                           // the string of the previous step's last code
    const uint32_t sl = prev_src ? 0u : ci - 1u;
    uint32_t lev = 0;
    bool res = !neu;
    for (uint32_t r = 0; r < 64u; r++) {
      if (!__ballot(!res)) break;
      const uint32_t Lm = __shfl(L, sl), levm = __shfl(lev, sl), resm = __shfl((uint32_t)res, sl);
      const uint32_t levi = __shfl(lev, ci), resi = __shfl((uint32_t)res, ci);
      if (!res) {
        const bool okm = prev_src || resm, oki = ci >= lane || resi;
        if (okm && oki) {
          L = (prev_src ? s.plen : Lm) + 1u;
          const uint32_t l0 = prev_src ? 0u : levm + 1u, l1 = ci < lane ? levi + 1u : 0u;
          lev = l0 > l1 ? l0 : l1;
          res = true;
        }
      }
    }
    if (!act) L = 0u;
    uint32_t total;
    const uint32_t P = s.o + gif_excl_scan(L, lane, &total);
    const uint32_t Pm = __shfl(P, sl);
    if (neu) S = prev_src ? s.ppos : Pm;
    const bool kw = neu && ci == lane;
    const bool done_after = s.o + total >= npix;
    // ---- what ends the decode badly: a bad code, the data's end or an end code before the last pixel
    if (!done_after) {
      if (kb < k) {
        fail = kGifFailCode;
        break;
      }
      if (k < 64u) {
        const uint32_t ck = __shfl(c, k), ik = __shfl((uint32_t)inb, k);
        if (!ik || ck == clear + 1u) {
          fail = kGifFailShort;
          break;
        }
      }
    }
    // ---- new entries: code j makes string(code j-1) + first byte of string(code j)
    {
      const uint32_t Pp = __shfl_up(P, 1), Lp = __shfl_up(L, 1);
      const uint32_t E = s.nf + lane - a;
      if (act && lane >= a && E < kGifMaxCodes) {
        tpos[E] = lane ? Pp : s.ppos;
        tlen[E] = (uint16_t)((lane ? Lp : s.plen) + 1u);
      }
    }
    // ---- copies, level by level
    const uint32_t room = P < npix ? npix - P : 0u;
    const uint32_t CL = L < room ? L : room;
    for (uint32_t lv = 0; lv < 64u; lv++) {
      const bool mine = CL > 0u && lev == lv;
      if (mine && lit) {
        out[P] = (uint8_t)c;
      } else if (mine && CL <= kGifShort) {
        uint32_t v[kGifShort];
#pragma unroll
        for (uint32_t t = 0; t < kGifShort; t++)
          if (t < CL) v[t] = gif_ld(out + S + gif_copy_index(t, L, kw));
#pragma unroll
        for (uint32_t t = 0; t < kGifShort; t++)
          if (t < CL) out[P + t] = (uint8_t)v[t];
      }
      uint64_t big = __ballot(mine && !lit && CL > kGifShort);
      while (big) {  // long strings: the whole wave, 64 bytes at a time
        const uint32_t m = (uint32_t)__builtin_ctzll(big);
        big &= big - 1ull;
        const uint32_t Pb = __shfl(P, m), Sb = __shfl(S, m), Lb = __shfl(L, m), Cb = __shfl(CL, m);
        const bool kwb = __shfl((uint32_t)kw, m) != 0u;
        for (uint32_t t = lane; t < Cb; t += 64u) out[Pb + t] = (uint8_t)gif_ld(out + Sb + gif_copy_index(t, Lb, kwb));
      }
      gif_drain();
      if (!__ballot(CL > 0u && lev > lv)) break;
    }
    __syncthreads();  // the table's new entries before the next step's lookups
    // ---- the state after the step
    s.o = done_after ? npix : s.o + total;
    if (kv == 64u) {
      s.nf = gif_lane_nf(s.nf, a, 64u);
      s.pv = 1u;
      s.ppos = __shfl(P, 63);
      s.plen = __shfl(L, 63);
      s.bitpos += wsum;
    } else if (!done_after) {  // a clear code at lane k (everything else ended the decode above)
      s.nf = clear + 2u;
      s.pv = 0u;
      s.bitpos = __shfl(offj, k) + __shfl(wj, k);
    }
  }
  if (!fail && s.o < npix) fail = kGifFailShort;
  if (fail && lane == 0) {
    im.gif.fail = fail;
    im.status = 1;  // DG_ERR_UNSUPPORTED: the caller's CPU decoder decides
  }
}

// ------------------------------------------------------------ expand

// One screen pixel per thread.
__global__ __launch_bounds__(256) void k_gif_expand(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const GifDesc &g = im.gif;
  const uint32_t idx = it.item0 + threadIdx.x;
  const uint32_t W = im.width;
  if (idx >= W * im.height) return;
  const uint32_t y = idx / W, x = idx - y * W;
  const uint32_t fx = x - g.left, fy = y - g.top;  // (wraps above the frame: then >= fw / fh)
  uint32_t v = 0;  // outside the frame: transparent black
  if (fx < g.fw && fy < g.fh) {
    const uint32_t i = gp<const uint8_t>(g.idx)[(size_t)gif_stream_row(fy, g.fh, g.interlace) * g.fw + fx];
    if (i < g.npal) {
      v = gp<const uint32_t>(g.pal)[i];
    } else {
      im.gif.fail = kGifFailPalette;
      im.status = 1;  // DG_ERR_UNSUPPORTED
    }
  }
  *(DG_GLOBAL uint32_t *)(gp<uint8_t>(im.pix) + (size_t)y * im.pix_stride + 4u * (size_t)x) = v;
}

// ------------------------------------------------------------ launchers

void launch_gif_gather(hipStream_t st, const GatherJob *jobs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_gif_gather, dim3(nwg), dim3(256), 0, st, jobs, list);
}
void launch_gif_lzw(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_gif_lzw, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_gif_expand(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_gif_expand, dim3(nwg), dim3(256), 0, st, imgs, list);
}

}  // namespace dg
