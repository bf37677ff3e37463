// dg_tiff_g4.hip — CDNA4 (gfx950) kernel of the CCITT Group 4 decode (option "tiff_bilevel").
//
//   k_tiff_g4   one segment's T.6 stream -> its packed rows (ceil(seg_w / 8) bytes each, MSB
//               first) in the decoded arena, as a raw bilevel segment holds them; k_tiff_expand1
//               (dg_tiff.hip) takes them to the pixel plane.
//
// One wave per (image, segment).  A row's code boundaries depend on where a0 stands, so the
// decode has two layers (dg_tiff_g4.h holds the lane routines, tests/native/tiff_g4_emu.cpp
// runs them on the CPU):
//
//   * Speculative tokens.  Lane j decodes the token that would start at bit bitpos + j from a
//     64-bit window (three cross-lane reads of the source window, one dword per lane in
//     registers): the mode, and for horizontal mode both runs under both colours.
//   * Wave-uniform resolve.  The real tokens are walked in order with cross-lane reads of the
//     lane whose offset is the next token's.  The reference and the current row are bitmaps in
//     LDS (2 KiB each at 16,384 pixels).  b1 and b2 come from the reference row's changing
//     elements, row ^ (row << 1) across words: a lane tests one word right of a0, a ballot
//     picks the first lane with one, ctz the bit.  Runs are filled by the lanes whose words
//     they cover.
//   * A run of k `1` bits is k V0 tokens: behind the first b1 the current row copies the
//     reference row up to its k-th next changing element, found with a popcount prefix over
//     the words right of a0 and copied in one pass.
//
// A finished row goes through a staging buffer in LDS, where rows are joined at byte
// granularity, and leaves in 16-byte stores.  LDS: 2 rows + staging + 2,304 bytes of code
// tables = 8.5 KiB per wave.
//
// Every loop is bounded: a resolve iteration consumes at least one bit or ends the decode, a
// search trip advances 2,048 pixels, and no wave waits on a flag.  What libtiff pads and the
// fax crate fails (an invalid or extension code, a run past the row's end, a pass mode without
// b1, data that ends before the rows do) is kTiffFailG4 / DG_ERR_UNSUPPORTED.
#include <hip/hip_runtime.h>

#include "dg_tiff_g4.h"
#include "host/tiff_header.h"
#include "kernels.h"

namespace dg {

static_assert(kTiffG4MaxWidth == kG4MaxWidth, "the header walk refuses the rows the kernel cannot hold");

// The aligned dword at `ad`; its bytes at or past `end` read as zero.
__device__ __forceinline__ uint32_t g4_ld32(uint64_t ad, uint64_t end) {
  if (ad + 4u <= end) return *gp<const uint32_t>(ad);
  uint32_t v = 0;
  for (uint32_t q = 0; q < 4; q++)
    if (ad + q < end) v |= (uint32_t)*gp<const uint8_t>(ad + q) << (8u * q);
  return v;
}

// The first changing element of `ref` at or right of `from`: any (sel 0), to black (1) or to white (2); W if
// there is none.  ref[-1] is a zero guard word.
__device__ __forceinline__ uint32_t g4_find(const uint32_t *ref, uint32_t nwords, uint32_t W, uint32_t from, uint32_t sel,
                                            uint32_t lane) {
  for (uint32_t base = from >> 5; base < nwords; base += 64u) {
    const uint32_t i = base + lane;
    uint32_t m = 0;
    if (i < nwords) {
      const uint32_t r = ref[i], t = g4_trans(r, ref[(int32_t)i - 1]);
      m = sel == 0u ? t : sel == 1u ? t & r : t & ~r;
      if (i == from >> 5) m &= ~0u << (from & 31u);
    }
    const uint64_t any = __ballot(m != 0u);
    if (any) {
      const uint32_t l = (uint32_t)__builtin_ctzll(any);
      const uint32_t x = (base + l) * 32u + (uint32_t)__builtin_ctz(__shfl(m, l));
      return x < W ? x : W;
    }
  }
  return W;
}

__global__ __launch_bounds__(64) void k_tiff_g4(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  __shared__ __attribute__((aligned(16))) uint32_t rows[2][kG4RowWords + 4];  // [b][1 + i]: word i; [b][0] stays zero
  __shared__ __attribute__((aligned(16))) uint32_t stage[kG4RowWords + 8];    // up to 15 pending bytes and a row
  __shared__ uint16_t tabs[kG4TabSize];
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const TiffDesc &g = im.tiff;
  const u32x4 sq = *gp<const u32x4>(g.segs + 16ull * it.item0);
  const TiffSeg sg = TiffSeg{sq.x, sq.y, sq.z, sq.w};
  const uint32_t lane = threadIdx.x;
  const uint32_t W = g.seg_w, nwords = (W + 31u) >> 5, rowb = (W + 7u) >> 3;
  const uint32_t nbytes = sg.nbytes, nbits = nbytes * 8u;
  const uint64_t src = g.file + sg.off, src_end = src + nbytes;
  DG_GLOBAL uint8_t *out = gp<uint8_t>(g.dec + sg.dst);
  bool fail = W == 0u || W > kG4MaxWidth || nbytes >= (1u << 28);
  const uint32_t nrows = fail ? 0u : sg.dec / rowb;
  // ---- the lookup tables and two white rows
  uint16_t *const twhite = tabs, *const tblack1 = tabs + kG4WhiteSize, *const tblack2 = tblack1 + kG4Black1Size;
  for (uint32_t i = lane; i < kG4TabSize; i += 64u) tabs[i] = 0;
  for (uint32_t i = lane; i < kG4RowWords + 4u; i += 64u) rows[0][i] = rows[1][i] = 0u;
  __syncthreads();
  for (uint32_t i = lane; i < kG4Codes; i += 64u) g4_fill(twhite, tblack1, tblack2, i);
  __syncthreads();
  const G4Tabs T = {twhite, tblack1, tblack2};
  auto peek = [&](uint32_t pos) -> uint64_t {
    const uint64_t a = src + (pos >> 3), a4 = a & ~3ull;
    return g4_window(g4_ld32(a4, src_end), g4_ld32(a4 + 4u, src_end), g4_ld32(a4 + 8u, src_end), (uint32_t)(a & 3ull) * 8u + (pos & 7u));
  };
  uint32_t bitpos = 0, a0 = 0, colour = 0, rdone = 0, cb = 0, pend = 0, obase = 0;
  bool start = true;  // a0 stands before the row's first pixel
  uint32_t wdw = 0;
  uint64_t win_addr = 0;
  bool win_valid = false;
  for (uint32_t step = 0; step <= nbits && rdone < nrows && !fail; step++) {
    // ---- the source window (lane i: the dword at win_addr + 4 i) and every lane's own 64 bits
    const uint32_t k0 = bitpos >> 3;
    if (!win_valid || src + k0 + kG4StepBytes > win_addr + kG4WinBytes) {
      win_addr = (src + k0) & ~3ull;
      win_valid = true;
      wdw = g4_ld32(win_addr + 4ull * lane, src_end);
    }
    const uint32_t off = bitpos + lane;
    const uint32_t wi = (uint32_t)(src + (off >> 3) - win_addr), di = wi >> 2;
    const uint32_t d0 = __shfl(wdw, di & 63u), d1 = __shfl(wdw, (di + 1u) & 63u), d2 = __shfl(wdw, (di + 2u) & 63u);
    const uint64_t w = g4_window(d0, d1, d2, (wi & 3u) * 8u + (off & 7u));
    const G4Tok tok = g4_token(T, w);
    const uint64_t ones = __ballot((w >> 63) != 0ull);  // V0 codes
    // ---- the real tokens, in order
    uint32_t p = 0;
    while (p < 64u && rdone < nrows) {
      uint32_t *const cur = &rows[cb][1];
      const uint32_t *const ref = &rows[cb ^ 1u][1];
      const uint32_t from = start ? 0u : a0 + 1u;
      const uint32_t md = __shfl(tok.mode, p), kind = md & 15u;
      uint32_t used = (md >> 4) & 15u;  // bits the step consumes here
      uint32_t x0 = a0, x1 = a0, c0 = 0, c1 = 0;  // black pixels [x0, x1) and pixels [c0, c1) copied from the reference row
      if (kind == kG4Bad || bitpos + p + used > nbits) {
        fail = true;
        break;
      }
      if (kind == kG4V) {
        const int32_t a1 = (int32_t)g4_find(ref, nwords, W, from, colour ? 2u : 1u, lane) + (int32_t)(md >> 8) - 3;
        if (a1 < (int32_t)a0 || a1 > (int32_t)W) {
          fail = true;
          break;
        }
        x1 = colour ? (uint32_t)a1 : a0;
        a0 = (uint32_t)a1;
        colour ^= 1u;
        // ---- the V0 codes that follow a V0: the current row runs along the reference row
        const uint64_t rest = ~(ones >> p);
        uint32_t left = used == 1u ? (rest ? (uint32_t)__builtin_ctzll(rest) : 64u) - 1u : 0u;
        uint32_t sfrom = a0 + 1u, e = a0;
        c0 = a0;
        while (left && e < W) {
          const uint32_t base = sfrom >> 5, i = base + lane;
          uint32_t t = 0;
          if (i < nwords) {
            t = g4_trans(ref[i], ref[(int32_t)i - 1]);
            if (i == base) t &= ~0u << (sfrom & 31u);
            if (i == W >> 5) t &= (1u << (W & 31u)) - 1u;
          }
          const uint32_t cnt = (uint32_t)__popc(t);
          uint32_t incl = cnt;
#pragma unroll
          for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
          }
          const uint32_t total = __shfl(incl, 63);
          if (left <= total) {  // the left-th changing element from here
            const uint32_t l = (uint32_t)__builtin_ctzll(__ballot(incl >= left));
            e = (base + l) * 32u + g4_nth(__shfl(t, l), left - 1u - (__shfl(incl, l) - __shfl(cnt, l)));
            used += left;
            colour ^= left & 1u;
            left = 0u;
          } else if (base + 64u >= nwords) {  // all of them, then the one behind the last pixel
            e = W;
            used += total + 1u;
            colour ^= (total + 1u) & 1u;
            left = 0u;
          } else {  // more than these 2,048 pixels hold
            used += total;
            colour ^= total & 1u;
            left -= total;
            sfrom = (base + 64u) * 32u;
            e = sfrom - 1u;
          }
        }
        c1 = e;
        a0 = e;
      } else if (kind == kG4P) {
        const uint32_t b1 = g4_find(ref, nwords, W, from, colour ? 2u : 1u, lane);
        if (b1 >= W) {
          fail = true;
          break;
        }
        const uint32_t b2 = g4_find(ref, nwords, W, b1 + 1u, 0u, lane);
        x1 = colour ? b2 : a0;
        a0 = b2;
      } else {  // horizontal
        uint32_t hy = __shfl(colour ? tok.h[1] : tok.h[0], p), r1 = hy & 4095u, r2 = (hy >> 12) & 4095u;
        used = (hy >> 24) & 127u;
        if (hy == kG4Slow) {  // a long make-up chain: every lane reads the two runs from the stream
          uint32_t pos = bitpos + p + 3u;
          if (!g4_run_slow(T, peek, &pos, colour, &r1) || !g4_run_slow(T, peek, &pos, colour ^ 1u, &r2)) hy = 0u;
          used = pos - bitpos - p;
        }
        if (hy == 0u || bitpos + p + used > nbits || a0 + r1 + r2 > W) {
          fail = true;
          break;
        }
        x0 = colour ? a0 : a0 + r1;
        x1 = colour ? a0 + r1 : a0 + r1 + r2;
        a0 += r1 + r2;
      }
      start = false;
      // ---- the pixels
      if (x1 > x0)
        for (uint32_t i = (x0 >> 5) + lane; i <= (x1 - 1u) >> 5; i += 64u) cur[i] |= g4_span(i, x0, x1);
      if (c1 > c0)
        for (uint32_t i = (c0 >> 5) + lane; i <= (c1 - 1u) >> 5; i += 64u) cur[i] |= ref[i] & g4_span(i, c0, c1);
      __syncthreads();
      p += used;
      if (a0 < W) continue;
      // ---- the row's end: its bytes behind the pending ones, whole 16-byte pieces to the arena
      uint8_t *const sb = (uint8_t *)stage;
      for (uint32_t i = lane; i < nwords; i += 64u) {
        const uint32_t v = g4_out(cur[i]);
#pragma unroll
        for (uint32_t q = 0; q < 4; q++)
          if (4u * i + q < rowb) sb[pend + 4u * i + q] = (uint8_t)(v >> (8u * q));
      }
      __syncthreads();
      const uint32_t have = pend + rowb, np = rdone + 1u == nrows ? (have + 15u) >> 4 : have >> 4;
      for (uint32_t q = lane; q < np; q += 64u) *(DG_GLOBAL u32x4 *)(out + obase + 16u * q) = *(const u32x4 *)(stage + 4u * q);
      const uint32_t keep = lane < 4u ? stage[4u * np + lane] : 0u;
      __syncthreads();
      if (lane < 4u) stage[lane] = keep;
      obase += 16u * np;
      pend = have > 16u * np ? have - 16u * np : 0u;
      // ---- the next row: white, against this one
      cb ^= 1u;
      for (uint32_t i = lane; i < nwords; i += 64u) rows[cb][1u + i] = 0u;
      __syncthreads();
      a0 = 0u;
      colour = 0u;
      start = true;
      rdone++;
    }
    bitpos += p;
  }
  if ((fail || rdone < nrows) && lane == 0) {
    im.tiff.fail = kTiffFailG4;
    im.status = 1;  // DG_ERR_UNSUPPORTED
  }
}

void launch_tiff_g4(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_tiff_g4, dim3(nwg), dim3(64), 0, st, imgs, list);
}

}  // namespace dg
