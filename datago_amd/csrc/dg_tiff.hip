// dg_tiff.hip — CDNA4 (gfx950) kernels of the TIFF decode stage (option "tiff").
//
//   k_tiff_lzw       one segment's LZW codes -> its bytes in the decoded arena
//   k_tiff_packbits  one segment's PackBits stream -> its bytes in the decoded arena
//   k_tiff_expand    decoded (compression 1: the file's own) segment bytes -> the pixel plane:
//                    predictor 2, WhiteIsZero, strip and tile placement, the edge crop
//   k_tiff_expand16  the same for 16-bit samples (option "tiff16"): the file's byte order undone,
//                    predictor 2 on whole samples, native-endian uint16 in the pixel plane
//   k_tiff_expand1   the same for 1-bit samples (option "tiff_bilevel"): packed rows, MSB first, to
//                    L8 of 0 / 255
//
// What they restate: the tiff crate as image 0.25's TiffDecoder drives it for
// load_from_memory, for the files it and libtiff (Pillow) decode to the same bytes;
// dg_tiff.h holds the lane routines, tests/native/tiff_emu.cpp runs them on the CPU.
//
// A TIFF's coded data comes in independent segments, so the work item of the two
// decode kernels is (image, segment), one wave each: a batch puts images x segments
// waves on the machine and no image waits for its own serial stream.
//
// k_tiff_lzw follows the scheme of k_gif_lzw (64 codes per step, closed-form widths,
// entries as (position, length) in the segment's own output, copies level by level)
// with TIFF's code stream, and differs in where the data lives:
//   * The output of a segment of up to kTiffLdsOut (64 KiB) bytes stays in LDS while
//     it is decoded.  A copy level reads what the level before wrote, and in LDS that
//     is an in-order write and read of one wave: no store drain, no L1-bypassing
//     reload, no byte stores to memory.  The finished segment leaves in 16-byte stores.
//     Positions then fit 16 bits, so the table is 16 KiB.
//   * A larger segment (a whole image in one strip, a 256 x 256 RGB tile) is written
//     to the decoded arena as it goes and read back past the L1, as k_gif_lzw does,
//     with 32-bit positions (24 KiB of table in the same LDS).
//   * The source window is not in LDS: a lane keeps one dword of a 256-byte window
//     in a register and the codes' bytes come by cross-lane reads.
//   LDS per workgroup: 16 KiB table + 64 KiB output = 80 KiB, so two waves per CU
//   (160 KiB), against k_gif_lzw's six.  The choice is not measured: it bets that a
//   step's latency bounds a wave and that LDS copy levels cut it by more than four more
//   waves per CU would hide.  DESIGN.md §3 "TIFF" has the rates and what to try next.
//
// k_tiff_packbits takes 64 header candidates per step: only a header's position is
// serial, found by hopping; output positions come from a prefix sum.
//
// k_tiff_expand gives a wave one row of one segment column at a time, a lane four
// pixels of it from aligned dword loads.  Predictor 2 is a prefix sum with stride spp
// modulo 256: a lane sums its own four pixels per sample, the 64 lane totals are
// scanned with cross-lane shuffles and added back; the carry runs on to the next 256
// pixels of the row.
//
// k_tiff_expand16 keeps that split of the work.  A lane's four pixels are 2 x spp dwords with two
// samples each, funnel-shifted from aligned loads at one of four byte phases; an MM file's
// samples are swapped two at a time by one byte permute; predictor 2 regroups a pixel's samples
// into ceil(spp / 2) dwords so that the sums are packed 16-bit adds (v_pk_add_u16), scanned over
// the wave as above; the stores are 16 bytes wide for spp 2 and 4, 8 bytes for spp 1 and 3.
//
// k_tiff_expand1 keeps the split too.  A lane takes 32 pixels: one dword of the packed row, funnel-shifted
// from two aligned loads at any byte phase, eight nibbles spread to 0 / 255 by two multiplies each
// (tiff1_spread), WhiteIsZero as an exclusive or, two 16-byte stores.  The bits come from the file in
// place (compression 1) or from the arena, where k_tiff_g4 (dg_tiff_g4.hip) and the byte decoders leave
// the same rows.
//
// Every loop is bounded by the segment's bit or byte count and its decoded size: a
// step consumes input or ends the decode.
#include <hip/hip_runtime.h>

#include "dg_tiff.h"
#include "kernels.h"

namespace dg {

__device__ __forceinline__ uint32_t tiff_excl_scan(uint32_t v, uint32_t lane, uint32_t *total) {
  uint32_t x = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  *total = __shfl(x, 63);
  return x - v;
}

// The aligned dword at `ad`; its bytes at or past `end` read as zero.
__device__ __forceinline__ uint32_t tiff_ld32(uint64_t ad, uint64_t end) {
  if (ad + 4u <= end) return *gp<const uint32_t>(ad);
  uint32_t v = 0;
  for (uint32_t q = 0; q < 4; q++)
    if (ad + q < end) v |= (uint32_t)*gp<const uint8_t>(ad + q) << (8u * q);
  return v;
}

// Entry i of a segment table (16 bytes on a 16-byte boundary).
__device__ __forceinline__ TiffSeg tiff_seg(uint64_t segs, uint32_t i) {
  const u32x4 q = *gp<const u32x4>(segs + 16ull * i);
  return TiffSeg{q.x, q.y, q.z, q.w};
}

// A byte the wave itself stored earlier (after tiff_drain): past the L1.
__device__ __forceinline__ uint32_t tiff_ld(const DG_GLOBAL uint8_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The wave's stores have reached the L2 before any later load is issued.
__device__ __forceinline__ void tiff_drain() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------ LZW

constexpr uint32_t kTiffTabBytes = 16384;  // lengths (8 KiB) + 16-bit positions (8 KiB); 32-bit positions reach 24 KiB

__global__ __launch_bounds__(64) void k_tiff_lzw(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kTiffTabBytes + kTiffLdsOut];
  uint16_t *const tlen = (uint16_t *)lds;
  uint16_t *const tpos16 = (uint16_t *)(lds + 8192);
  uint32_t *const tpos32 = (uint32_t *)(lds + 8192);
  uint8_t *const lout = lds + kTiffTabBytes;
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const TiffDesc &g = im.tiff;
  const TiffSeg sg = tiff_seg(g.segs, it.item0);
  const uint32_t lane = threadIdx.x;
  const uint32_t nbytes = sg.nbytes, nbits = nbytes * 8u, npix = sg.dec;
  const uint64_t src = g.file + sg.off, src_end = src + nbytes;
  const bool in_lds = npix <= kTiffLdsOut;
  DG_GLOBAL uint8_t *out = gp<uint8_t>(g.dec + sg.dst);
  auto ldb = [&](uint32_t i) -> uint32_t { return in_lds ? (uint32_t)lout[i] : tiff_ld(out + i); };
  auto stb = [&](uint32_t i, uint32_t v) {
    if (in_lds)
      lout[i] = (uint8_t)v;
    else
      out[i] = (uint8_t)v;
  };
  GifLzw s = {0u, kTiffFirst, 0u, 0u, 0u, 0u};
  uint32_t wdw = 0, fullc = 0, fail = 0;
  uint64_t win_addr = 0;
  bool win_valid = false;
  const uint32_t max_steps = nbits / 9u + 2u;
  for (uint32_t step = 0; step < max_steps && s.o < npix; step++) {
    // ---- the source window: lane i holds the dword at win_addr + 4 i
    if (nbytes) {
      const uint32_t k0 = s.bitpos >> 3;
      uint32_t k1 = k0 + kTiffStepBytes - 1u;
      k1 = k1 < nbytes ? k1 : nbytes - 1u;
      if (k0 <= k1 && (!win_valid || src + k1 >= win_addr + kTiffWinBytes)) {
        win_addr = (src + k0) & ~3ull;
        win_valid = true;
        wdw = tiff_ld32(win_addr + 4ull * lane, src_end);
      }
    }
    // ---- widths, bit offsets, codes
    const uint32_t a = s.pv ? 0u : 1u;
    const uint32_t nfj = gif_lane_nf(s.nf, a, lane);
    const uint32_t wj = tiff_width(nfj);
    uint32_t wsum;
    const uint32_t offj = s.bitpos + tiff_excl_scan(wj, lane, &wsum);
    const bool inb = offj + wj <= nbits;
    const uint32_t wi = (uint32_t)(src + (offj >> 3) - win_addr);  // (meaningless past the data: not used there)
    const uint32_t lo = __shfl(wdw, (wi >> 2) & 63u), hi = __shfl(wdw, ((wi >> 2) + 1u) & 63u);
    const uint32_t x = __funnelshift_r(lo, hi, 8u * (wi & 3u));
    const uint32_t c = inb ? tiff_code(x & 255u, (x >> 8) & 255u, (x >> 16) & 255u, offj, wj) : 0u;
    const bool special = inb && (c == kTiffClear || c == kTiffEnd);
    const uint64_t stopm = __ballot(special || !inb);
    const uint32_t k = stopm ? (uint32_t)__builtin_ctzll(stopm) : 64u;
    const uint64_t badm = __ballot(lane < k && gif_code_bad(c, nfj, lane, a));
    const uint32_t kb = badm ? (uint32_t)__builtin_ctzll(badm) : 64u;
    const uint32_t kv = k < kb ? k : kb;  // lanes below kv hold data codes
    const bool act = lane < kv;
    const bool lit = act && c < kTiffClear;
    const bool old = act && !lit && c < s.nf;
    const bool neu = act && !lit && !old;  // an entry created inside this step
    const uint64_t fullm = __ballot(act && nfj == kGifMaxCodes);  // data codes read with a full table
    // ---- string lengths and copy levels
    uint32_t L = lit ? 1u : old ? (uint32_t)tlen[c] : 0u;
    uint32_t S = old ? (in_lds ? (uint32_t)tpos16[c] : tpos32[c]) : 0u;
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
    const uint32_t P = s.o + tiff_excl_scan(L, lane, &total);
    const uint32_t Pm = __shfl(P, sl);
    if (neu) S = prev_src ? s.ppos : Pm;
    const bool kw = neu && ci == lane;
    const bool done_after = s.o + total >= npix;
    // ---- what ends the decode badly: the code that is one too many for a full table (if a byte is still
    // missing when it is read), a bad code, the data's end or an end code before the last byte
    {
      const uint32_t upto = fullc + (uint32_t)__popcll(fullm & (~0ull >> (63u - lane)));
      const uint64_t overm = __ballot(((fullm >> lane) & 1ull) && upto > kTiffFullCodes);
      if (overm && __shfl(P, (uint32_t)__builtin_ctzll(overm)) < npix) {
        fail = kTiffFailFull;
        break;
      }
      fullc += (uint32_t)__popcll(fullm);
    }
    if (!done_after) {
      if (kb < k) {
        fail = kTiffFailCode;
        break;
      }
      if (k < 64u) {
        const uint32_t ck = __shfl(c, k), ik = __shfl((uint32_t)inb, k);
        if (!ik || ck == kTiffEnd) {
          fail = kTiffFailShort;
          break;
        }
      }
    }
    // ---- new entries: code j makes string(code j-1) + first byte of string(code j)
    {
      const uint32_t Pp = __shfl_up(P, 1), Lp = __shfl_up(L, 1);
      const uint32_t E = s.nf + lane - a;
      if (act && lane >= a && E < kGifMaxCodes) {
        const uint32_t ep = lane ? Pp : s.ppos, el = (lane ? Lp : s.plen) + 1u;
        if (in_lds)
          tpos16[E] = (uint16_t)ep;
        else
          tpos32[E] = ep;
        tlen[E] = (uint16_t)el;  // (an entry is one byte longer than an earlier string: under 4096 + kTiffFullCodes)
      }
    }
    // ---- copies, level by level
    const uint32_t room = P < npix ? npix - P : 0u;
    const uint32_t CL = L < room ? L : room;
    for (uint32_t lv = 0; lv < 64u; lv++) {
      const bool mine = CL > 0u && lev == lv;
      if (mine && lit) {
        stb(P, c);
      } else if (mine && CL <= kTiffShort) {
        uint32_t v[kTiffShort];
#pragma unroll
        for (uint32_t t = 0; t < kTiffShort; t++)
          if (t < CL) v[t] = ldb(S + gif_copy_index(t, L, kw));
#pragma unroll
        for (uint32_t t = 0; t < kTiffShort; t++)
          if (t < CL) stb(P + t, v[t]);
      }
      uint64_t big = __ballot(mine && !lit && CL > kTiffShort);
      while (big) {  // long strings: the whole wave, 64 bytes at a time
        const uint32_t m = (uint32_t)__builtin_ctzll(big);
        big &= big - 1ull;
        const uint32_t Pb = __shfl(P, m), Sb = __shfl(S, m), Lb = __shfl(L, m), Cb = __shfl(CL, m);
        const bool kwb = __shfl((uint32_t)kw, m) != 0u;
        for (uint32_t t = lane; t < Cb; t += 64u) stb(Pb + t, ldb(Sb + gif_copy_index(t, Lb, kwb)));
      }
      if (in_lds)
        __syncthreads();  // one wave: its LDS writes are done before the next level reads
      else
        tiff_drain();
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
      s.nf = kTiffFirst;
      s.pv = 0u;
      s.bitpos = __shfl(offj, k) + __shfl(wj, k);
      fullc = 0u;
    }
  }
  if (!fail && s.o < npix) fail = kTiffFailShort;
  if (fail) {
    if (lane == 0) {
      im.tiff.fail = fail;
      im.status = fail == kTiffFailFull ? 1 : 2;  // DG_ERR_UNSUPPORTED : DG_ERR_CORRUPT
    }
    return;
  }
  if (in_lds) {  // the finished segment: LDS -> the decoded arena (its slot is a multiple of 16 bytes)
    __syncthreads();
    for (uint32_t i = 16u * lane; i < npix; i += 1024u) *(DG_GLOBAL u32x4 *)(out + i) = *(const u32x4 *)(lout + i);
  }
}

// ------------------------------------------------------------ PackBits

__global__ __launch_bounds__(64) void k_tiff_packbits(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const TiffDesc &g = im.tiff;
  const TiffSeg sg = tiff_seg(g.segs, it.item0);
  const uint32_t lane = threadIdx.x;
  const uint32_t nbytes = sg.nbytes, npix = sg.dec;
  const DG_GLOBAL uint8_t *src = gp<const uint8_t>(g.file + sg.off);
  DG_GLOBAL uint8_t *out = gp<uint8_t>(g.dec + sg.dst);
  uint32_t pos = 0, skip = 0, o = 0;  // skip: bytes at the step's head that are data of the run before
  bool fail = false;
  const uint32_t max_steps = nbytes / 64u + 2u;
  for (uint32_t step = 0; step < max_steps && o < npix && pos < nbytes; step++) {
    // ---- every byte as a header
    const uint32_t bp = pos + lane;
    const bool inb = bp < nbytes;
    const uint32_t n = inb ? (uint32_t)src[bp] : 128u, nxt = bp + 1u < nbytes ? (uint32_t)src[bp + 1u] : 0u;
    const uint32_t size = tiff_pb_size(n);
    // ---- which bytes are headers: hop from one to the next
    uint64_t heads = 0;
    uint32_t cur = skip;
    while (cur < 64u) {
      heads |= 1ull << cur;
      cur += __shfl(size, cur);
    }
    skip = cur - 64u;
    const bool head = inb && ((heads >> lane) & 1ull);
    // ---- a header whose data passes the segment's end cuts the step
    const uint64_t cutm = __ballot(head && bp + size > nbytes);
    const uint32_t kc = cutm ? (uint32_t)__builtin_ctzll(cutm) : 64u;
    const uint32_t c = head && lane < kc ? tiff_pb_out(n) : 0u;
    uint32_t total;
    const uint32_t P = o + tiff_excl_scan(c, lane, &total);
    if (kc < 64u && o + total < npix) {
      fail = true;
      break;
    }
    // ---- the bytes: short runs by their own lane, long ones by the wave
    const uint32_t room = P < npix ? npix - P : 0u;
    const uint32_t CL = c < room ? c : room;
    const bool rep = n > 128u;
    if (CL <= kTiffShort) {
#pragma unroll
      for (uint32_t t = 0; t < kTiffShort; t++)
        if (t < CL) out[P + t] = (uint8_t)(rep ? nxt : (uint32_t)src[bp + 1u + t]);
    }
    uint64_t big = __ballot(CL > kTiffShort);
    while (big) {
      const uint32_t m = (uint32_t)__builtin_ctzll(big);
      big &= big - 1ull;
      const uint32_t Pb = __shfl(P, m), Cb = __shfl(CL, m), vb = __shfl(nxt, m), sb = pos + m + 1u;
      const bool rb = __shfl((uint32_t)rep, m) != 0u;
      for (uint32_t t = lane; t < Cb; t += 64u) out[Pb + t] = (uint8_t)(rb ? vb : (uint32_t)src[sb + t]);
    }
    o = o + total < npix ? o + total : npix;
    pos += 64u;
  }
  if ((fail || o < npix) && lane == 0) {
    im.tiff.fail = kTiffFailShort;
    im.status = 2;  // DG_ERR_CORRUPT
  }
}

// ------------------------------------------------------------ expand

// One row of one segment column (npx pixels from `row`) to `dst`: 256 pixels per trip.
template <uint32_t SPP>
__device__ __forceinline__ void tiff_row(uint64_t row, uint64_t end, DG_GLOBAL uint8_t *dst, uint32_t npx, bool pred, uint32_t inv,
                                         uint32_t lane) {
  uint32_t carry = 0;  // predictor 2: the sample sums up to this trip's first pixel
  for (uint32_t q0 = 0; q0 < npx; q0 += 256u) {
    const uint32_t x0 = q0 + 4u * lane;
    const uint32_t n = x0 >= npx ? 0u : npx - x0 < 4u ? npx - x0 : 4u;
    const uint64_t A = row + (uint64_t)x0 * SPP, last = A + n * SPP, A0 = A & ~3ull;
    const uint32_t sh = (uint32_t)(A & 3ull) * 8u;
    uint32_t r[SPP + 1], v[4] = {0u, 0u, 0u, 0u}, p[4];
#pragma unroll
    for (uint32_t k = 0; k <= SPP; k++) r[k] = A0 + 4u * k < last ? tiff_ld32(A0 + 4u * k, end) : 0u;
#pragma unroll
    for (uint32_t k = 0; k < SPP; k++) v[k] = __funnelshift_r(r[k], r[k + 1], sh);
#pragma unroll
    for (uint32_t t = 0; t < 4; t++) p[t] = tiff_px(v, t, SPP);
    if (pred) {
#pragma unroll
      for (uint32_t t = 1; t < 4; t++) p[t] = tiff_badd(p[t], p[t - 1]);
      uint32_t x = p[3];  // the lane's total; inclusive scan over the lanes
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x = tiff_badd(x, y);
      }
      const uint32_t before = __shfl_up(x, 1);
      const uint32_t add = lane ? tiff_badd(carry, before) : carry;
#pragma unroll
      for (uint32_t t = 0; t < 4; t++) p[t] = tiff_badd(p[t], add);
      carry = tiff_badd(carry, __shfl(x, 63));
    }
#pragma unroll
    for (uint32_t t = 0; t < 4; t++) p[t] ^= inv;
    DG_GLOBAL uint8_t *o = dst + (size_t)x0 * SPP;
    if (n == 4u) {  // 4 x SPP bytes on a dword boundary: x0 and the segment column's first pixel are multiples of 4
      if (SPP == 4u) {
        *(DG_GLOBAL u32x4 *)o = u32x4{p[0], p[1], p[2], p[3]};
      } else {
#pragma unroll
        for (uint32_t k = 0; k < SPP; k++) ((DG_GLOBAL uint32_t *)o)[k] = tiff_pack(p, k, SPP);
      }
    } else {
#pragma unroll
      for (uint32_t t = 0; t < 3; t++)
        if (t < n) {
#pragma unroll
          for (uint32_t sidx = 0; sidx < SPP; sidx++) o[t * SPP + sidx] = (uint8_t)(p[t] >> (8u * sidx));
        }
    }
  }
}

__global__ __launch_bounds__(64) void k_tiff_expand(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const TiffDesc &g = im.tiff;
  const uint32_t lane = threadIdx.x, W = im.width;
  const uint32_t pieces = im.height * g.across;
  for (uint32_t pc = it.item0; pc < it.item0 + kTiffExpandPieces && pc < pieces; pc++) {
    const TiffPiece pp = tiff_piece(pc, W, g.spp, g.seg_w, g.seg_h, g.across);
    const TiffSeg sg = tiff_seg(g.segs, pp.seg);
    const uint64_t base = g.comp == 1u ? g.file + sg.off : g.dec + sg.dst;
    const uint64_t end = base + (g.comp == 1u ? sg.nbytes : sg.dec);
    const uint64_t row = base + pp.off;
    const uint32_t npx = pp.npx;
    DG_GLOBAL uint8_t *dst = gp<uint8_t>(im.pix) + (size_t)pp.y * im.pix_stride + (size_t)pp.px0 * g.spp;
    const bool pred = g.pred == 2u;
    const uint32_t inv = g.invert ? 0xFFu : 0u;
    if (g.spp == 1u)
      tiff_row<1>(row, end, dst, npx, pred, inv, lane);
    else if (g.spp == 2u)
      tiff_row<2>(row, end, dst, npx, pred, inv, lane);
    else if (g.spp == 3u)
      tiff_row<3>(row, end, dst, npx, pred, inv, lane);
    else
      tiff_row<4>(row, end, dst, npx, pred, inv, lane);
  }
}

// ------------------------------------------------------------ expand, 16-bit samples

// One row of one segment column (npx pixels of SPP 16-bit samples from `row`, at any byte phase) to `dst` as
// native-endian uint16: 256 pixels per trip, a lane four of them = 2 x SPP dwords, two samples to a dword.
template <uint32_t SPP>
__device__ __forceinline__ void tiff_row16(uint64_t row, uint64_t end, DG_GLOBAL uint8_t *dst, uint32_t npx, bool pred, bool swap,
                                           uint32_t lane) {
  constexpr uint32_t ND = 2u * SPP, PD = (SPP + 1u) / 2u;  // dwords of a lane's row bytes, dwords of one pixel
  uint32_t carry[PD];  // predictor 2: the sample sums up to this trip's first pixel
#pragma unroll
  for (uint32_t k = 0; k < PD; k++) carry[k] = 0u;
  for (uint32_t q0 = 0; q0 < npx; q0 += 256u) {
    const uint32_t x0 = q0 + 4u * lane;
    const uint32_t n = x0 >= npx ? 0u : npx - x0 < 4u ? npx - x0 : 4u;
    const uint64_t A = row + (uint64_t)x0 * ND, last = A + n * ND, A0 = A & ~3ull;
    const uint32_t sh = (uint32_t)(A & 3ull) * 8u;  // four phases: an odd one puts every sample across a dword boundary
    uint32_t r[ND + 1], v[ND];
#pragma unroll
    for (uint32_t k = 0; k <= ND; k++) r[k] = A0 + 4u * k < last ? tiff_ld32(A0 + 4u * k, end) : 0u;
#pragma unroll
    for (uint32_t k = 0; k < ND; k++) v[k] = __funnelshift_r(r[k], r[k + 1], sh);
    if (swap) {
#pragma unroll
      for (uint32_t k = 0; k < ND; k++) v[k] = tiff16_swap(v[k]);
    }
    if (pred) {
      uint32_t p[4][2], x[PD];
#pragma unroll
      for (uint32_t t = 0; t < 4; t++) {
#pragma unroll
        for (uint32_t k = 0; k < 2; k++) p[t][k] = k < PD ? tiff16_px(v, t, k, SPP) : 0u;
      }
#pragma unroll
      for (uint32_t k = 0; k < PD; k++) {
#pragma unroll
        for (uint32_t t = 1; t < 4; t++) p[t][k] = tiff16_hadd(p[t][k], p[t - 1][k]);
        x[k] = p[3][k];  // the lane's total; inclusive scan over the lanes
      }
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (uint32_t k = 0; k < PD; k++) {
          const uint32_t y = __shfl_up(x[k], d);
          if (lane >= d) x[k] = tiff16_hadd(x[k], y);
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < PD; k++) {
        const uint32_t before = __shfl_up(x[k], 1);
        const uint32_t add = lane ? tiff16_hadd(carry[k], before) : carry[k];
#pragma unroll
        for (uint32_t t = 0; t < 4; t++) p[t][k] = tiff16_hadd(p[t][k], add);
        carry[k] = tiff16_hadd(carry[k], __shfl(x[k], 63));
      }
#pragma unroll
      for (uint32_t m = 0; m < ND; m++) v[m] = tiff16_pack(p, m, SPP);
    }
    DG_GLOBAL uint8_t *o = dst + (size_t)x0 * ND;
    if (n == 4u) {  // 8 x SPP bytes on an 8 x SPP / gcd(SPP, 2)-byte boundary: x0 and the segment column's first pixel are multiples of 4
      if (SPP % 2u == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < ND; k += 4) *(DG_GLOBAL u32x4 *)(o + 4u * k) = u32x4{v[k], v[k + 1], v[k + 2], v[k + 3]};
      } else {
#pragma unroll
        for (uint32_t k = 0; k < ND; k += 2) *(DG_GLOBAL u32x2 *)(o + 4u * k) = u32x2{v[k], v[k + 1]};
      }
    } else {  // the row's ragged end, by samples
#pragma unroll
      for (uint32_t j = 0; j < 3u * SPP; j++)
        if (j < n * SPP) ((DG_GLOBAL uint16_t *)o)[j] = (uint16_t)tiff16_at(v, j);
    }
  }
}

__global__ __launch_bounds__(64) void k_tiff_expand16(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const TiffDesc &g = im.tiff;
  const uint32_t lane = threadIdx.x, W = im.width, bpp = 2u * g.spp;
  const uint32_t pieces = im.height * g.across;
  for (uint32_t pc = it.item0; pc < it.item0 + kTiffExpandPieces && pc < pieces; pc++) {
    const TiffPiece pp = tiff_piece(pc, W, bpp, g.seg_w, g.seg_h, g.across);
    const TiffSeg sg = tiff_seg(g.segs, pp.seg);
    const uint64_t base = g.comp == 1u ? g.file + sg.off : g.dec + sg.dst;
    const uint64_t end = base + (g.comp == 1u ? sg.nbytes : sg.dec);
    const uint64_t row = base + pp.off;
    DG_GLOBAL uint8_t *dst = gp<uint8_t>(im.pix) + (size_t)pp.y * im.pix_stride + (size_t)pp.px0 * bpp;
    const bool pred = g.pred == 2u, swap = g.swap != 0u;
    if (g.spp == 1u)
      tiff_row16<1>(row, end, dst, pp.npx, pred, swap, lane);
    else if (g.spp == 2u)
      tiff_row16<2>(row, end, dst, pp.npx, pred, swap, lane);
    else if (g.spp == 3u)
      tiff_row16<3>(row, end, dst, pp.npx, pred, swap, lane);
    else
      tiff_row16<4>(row, end, dst, pp.npx, pred, swap, lane);
  }
}

// ------------------------------------------------------------ expand, 1-bit samples

__global__ __launch_bounds__(64) void k_tiff_expand1(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const TiffDesc &g = im.tiff;
  const uint32_t lane = threadIdx.x, W = im.width, rowb = (g.seg_w + 7u) >> 3;
  const uint32_t pieces = im.height * g.across;
  const uint32_t inv = g.invert ? ~0u : 0u;  // sample 1 is 255 under BlackIsZero, 0 under WhiteIsZero
  for (uint32_t pc = it.item0; pc < it.item0 + kTiffExpandPieces && pc < pieces; pc++) {
    const TiffPiece pp = tiff_piece(pc, W, 1u, g.seg_w, g.seg_h, g.across);
    const TiffSeg sg = tiff_seg(g.segs, pp.seg);
    const uint64_t base = g.comp == 1u ? g.file + sg.off : g.dec + sg.dst;
    const uint64_t end = base + (g.comp == 1u ? sg.nbytes : sg.dec);
    const uint64_t row = base + (uint64_t)(pp.y % g.seg_h) * rowb;  // (tiff_piece's offset counts a byte per pixel)
    DG_GLOBAL uint8_t *dst = gp<uint8_t>(im.pix) + (size_t)pp.y * im.pix_stride + pp.px0;
    for (uint32_t x0 = 32u * lane; x0 < pp.npx; x0 += 2048u) {
      const uint32_t n = pp.npx - x0 < 32u ? pp.npx - x0 : 32u;
      const uint64_t A = row + (x0 >> 3), last = A + ((n + 7u) >> 3), A0 = A & ~3ull;
      const uint32_t r0 = tiff_ld32(A0, end), r1 = A0 + 4u < last ? tiff_ld32(A0 + 4u, end) : 0u;
      const uint32_t v = __funnelshift_r(r0, r1, (uint32_t)(A & 3ull) * 8u);
      uint32_t o[8];
#pragma unroll
      for (uint32_t t = 0; t < 4; t++) {
        const uint32_t b = (v >> (8u * t)) & 255u;
        o[2u * t] = tiff1_spread(b >> 4) ^ inv;
        o[2u * t + 1u] = tiff1_spread(b) ^ inv;
      }
      DG_GLOBAL uint8_t *d = dst + x0;  // on a 32-byte boundary: x0 and the segment column's first pixel are multiples of 16 and 32
      if (n == 32u) {
        *(DG_GLOBAL u32x4 *)d = u32x4{o[0], o[1], o[2], o[3]};
        *(DG_GLOBAL u32x4 *)(d + 16) = u32x4{o[4], o[5], o[6], o[7]};
      } else {  // the row's ragged end
#pragma unroll
        for (uint32_t j = 0; j < 31; j++)
          if (j < n) d[j] = (uint8_t)(o[j >> 2] >> (8u * (j & 3u)));
      }
    }
  }
}

// ------------------------------------------------------------ launchers

void launch_tiff_lzw(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_tiff_lzw, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_tiff_packbits(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_tiff_packbits, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_tiff_expand(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_tiff_expand, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_tiff_expand16(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_tiff_expand16, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_tiff_expand1(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_tiff_expand1, dim3(nwg), dim3(64), 0, st, imgs, list);
}

}  // namespace dg
