// dg_tiff_inflate.hip — CDNA4 (gfx950) kernel of the TIFF Deflate decode (option "tiff_deflate").
//
//   k_tiff_inflate   one segment's zlib stream -> its bytes in the decoded arena
//
// What it restates: zlib's inflate as libtiff's ZIP codec drives it (the segment's decoded size is the
// output buffer; decoding stops when it is full).  dg_tiff_inflate.h holds the lane routines,
// tests/native/tiff_inflate_emu.cpp runs them on the CPU.  k_tiff_expand (dg_tiff.hip) reads the
// arena as it does after k_tiff_lzw.
//
// A TIFF is many short independent zlib streams, so the work item is (image, segment), one wave
// each, and the kernel is built for a short stream, unlike k_png_inflate's one wave per image:
//   * Output in LDS.  A segment of up to kTiffLdsOut (64 KiB) bytes stays in LDS while it is
//     decoded.  A match is an LDS-to-LDS copy at absolute positions: no ring, no mask, and a
//     distance is too far back when it is larger than the bytes so far.  The finished segment
//     leaves in 16-byte stores.  A larger segment is written to the arena as it goes and read
//     back past the L1, as k_tiff_lzw's large path does.
//   * The token step.  Every lane decodes the whole token that would start at bit bitpos + lane
//     (tinf_token: tables in LDS, 64 bits of the stream from the register window).  The real token
//     starts are found by hopping from start to start with cross-lane reads, as k_tiff_packbits
//     finds its headers; output positions are a prefix sum over the taken tokens.  Literals are
//     stored by their lanes; a match whose source lies before the step's first output byte is
//     copied at once (short ones by their lane, long ones by the wave); matches that reach into
//     the step's own output follow in token order.  An end-of-block code, an invalid token, the
//     data's end or the segment's last byte cuts the step.
//   * The source window is one dword per lane, read across lanes.
//   * Block headers are read wave-uniformly; the code-length tokens of a dynamic header are
//     decoded 64 bit offsets at a time like the data tokens, and the tables are built over the
//     lanes: counts and the sorted symbols by ballots per length, the primary tables one walk
//     per entry.
//   LDS per workgroup: 64 KiB output + 7.5 KiB tables, so two waves per CU as for k_tiff_lzw.
//   Neither that nor the 64 offsets per step is measured against another choice
//   (DESIGN.md §3 "TIFF Deflate").
//
// Every loop is bounded by the segment's bit count and its decoded size: a block header, a
// code-length round and a token step each consume at least one bit or end the decode.
#include <hip/hip_runtime.h>

#include "dg_tiff.h"
#include "dg_tiff_inflate.h"
#include "kernels.h"

namespace dg {

__device__ __forceinline__ uint32_t tinf_excl_scan(uint32_t v, uint32_t lane, uint32_t *total) {
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
__device__ __forceinline__ uint32_t tinf_ld32(uint64_t ad, uint64_t end) {
  if (ad + 4u <= end) return *gp<const uint32_t>(ad);
  uint32_t v = 0;
  for (uint32_t q = 0; q < 4; q++)
    if (ad + q < end) v |= (uint32_t)*gp<const uint8_t>(ad + q) << (8u * q);
  return v;
}

// Canonical form of the n (<= 320) code lengths in lens: cnt[l] (l < 16) and the symbols sorted by (length,
// symbol).  Lane l counts the codes of length l.  Returns what the Kraft sum leaves open (negative: over-
// subscribed); *ncodes the coded symbols.
__device__ __forceinline__ int32_t tinf_build(const uint8_t *lens, uint32_t n, uint16_t *cnt, uint16_t *sym, uint32_t lane,
                                              uint32_t *ncodes) {
  uint32_t c = 0;
  for (uint32_t base = 0; base < n; base += 64u) {
    const uint32_t L = base + lane < n ? (uint32_t)lens[base + lane] : 0u;
#pragma unroll
    for (uint32_t l = 1; l < 16u; l++) {
      const uint64_t m = __ballot(L == l);
      if (lane == l) c += (uint32_t)__popcll(m);
    }
  }
  uint32_t run = tinf_excl_scan(c, lane, ncodes);  // lane l: where the symbols of length l begin
  int32_t left = 1;
  for (uint32_t l = 1; l < 16u && left >= 0; l++) left = (left << 1) - (int32_t)__shfl(c, l);
  if (lane < 16u) cnt[lane] = (uint16_t)c;
  for (uint32_t base = 0; base < n; base += 64u) {
    const uint32_t L = base + lane < n ? (uint32_t)lens[base + lane] : 0u;
#pragma unroll
    for (uint32_t l = 1; l < 16u; l++) {
      const uint64_t m = __ballot(L == l);
      const uint32_t at = __shfl(run, l);
      if (L == l) sym[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(base + lane);
      if (lane == l) run += (uint32_t)__popcll(m);
    }
  }
  __syncthreads();
  return left;
}

// LDS after the output: the tables (bytes)
constexpr uint32_t kTinfLl = 0, kTinfDd = kTinfLl + 4u * kTinfLlSize, kTinfLsym = kTinfDd + 4u * kTinfDdSize;
constexpr uint32_t kTinfDsym = kTinfLsym + 2u * 288u, kTinfLcnt = kTinfDsym + 2u * 32u, kTinfDcnt = kTinfLcnt + 32u;
constexpr uint32_t kTinfLens = kTinfDcnt + 32u, kTinfClTab = kTinfLens + 320u, kTinfClLens = kTinfClTab + kTinfClSize;
constexpr uint32_t kTinfClCnt = kTinfClLens + 32u, kTinfClSym = kTinfClCnt + 32u, kTinfTabBytes = kTinfClSym + 64u;
static_assert(kTinfTabBytes % 16u == 0u && kTinfTabBytes + kTiffLdsOut <= 80u * 1024u, "two waves per CU");

__global__ __launch_bounds__(64) void k_tiff_inflate(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kTiffLdsOut + kTinfTabBytes];
  uint8_t *const lout = lds, *const tb = lds + kTiffLdsOut;
  uint32_t *const ll = (uint32_t *)(tb + kTinfLl), *const dd = (uint32_t *)(tb + kTinfDd);
  uint16_t *const lsym = (uint16_t *)(tb + kTinfLsym), *const dsym = (uint16_t *)(tb + kTinfDsym);
  uint16_t *const lcnt = (uint16_t *)(tb + kTinfLcnt), *const dcnt = (uint16_t *)(tb + kTinfDcnt);
  uint8_t *const lens = tb + kTinfLens, *const cltab = tb + kTinfClTab, *const cllens = tb + kTinfClLens;
  uint16_t *const clcnt = (uint16_t *)(tb + kTinfClCnt), *const clsym = (uint16_t *)(tb + kTinfClSym);
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const TiffDesc &g = im.tiff;
  const u32x4 sq = *gp<const u32x4>(g.segs + 16ull * it.item0);
  const uint32_t lane = threadIdx.x;
  const uint32_t nbytes = sq.y, nbits = nbytes * 8u, dec = sq.z;  // (a file is under 2^28 bytes)
  const uint64_t src = g.file + sq.x, src_end = src + nbytes;
  const bool in_lds = dec <= kTiffLdsOut;
  DG_GLOBAL uint8_t *out = gp<uint8_t>(g.dec + sq.w);
  // a byte the wave itself stored earlier: in LDS, or past the L1 after sync()
  auto ldb = [&](uint32_t i) -> uint32_t {
    return in_lds ? (uint32_t)lout[i] : (uint32_t)__hip_atomic_load(out + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto stb = [&](uint32_t i, uint32_t v) {
    if (in_lds)
      lout[i] = (uint8_t)v;
    else
      out[i] = (uint8_t)v;
  };
  auto sync = [&]() {  // one wave: its writes are done before its next reads
    if (in_lds) {
      __syncthreads();
    } else {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  };
  // ---- the source window: lane i holds the dword at win_addr + 4 i
  uint32_t wdw = 0;
  uint64_t win_addr = 0;
  bool win_valid = false;
  auto need = [&](uint32_t bitpos) {  // the kTinfStepBytes bytes from bitpos on are in the window
    const uint64_t a = src + (bitpos >> 3);
    if (!win_valid || a < win_addr || a + kTinfStepBytes > win_addr + kTinfWinBytes) {
      win_addr = a & ~3ull;
      win_valid = true;
      wdw = tinf_ld32(win_addr + 4ull * lane, src_end);
    }
  };
  auto fetch = [&](uint32_t bp) -> uint64_t {  // 64 bits of the stream from bit bp, at most 70 bits past need()'s position
    const uint32_t wi = (uint32_t)(src + (bp >> 3) - win_addr), q = wi >> 2, sh = 8u * (wi & 3u) + (bp & 7u);
    const uint32_t d0 = __shfl(wdw, q & 63u), d1 = __shfl(wdw, (q + 1u) & 63u), d2 = __shfl(wdw, (q + 2u) & 63u);
    const uint64_t lo = (uint64_t)d0 | ((uint64_t)d1 << 32);
    return sh ? (lo >> sh) | ((uint64_t)d2 << (64u - sh)) : lo;
  };

  uint32_t bitpos = 16, o = 0, fail = 0, bfinal = 0;
  bool in_block = false, exact = false;
  uint32_t trailer = 0xFFFFFFFFu;  // byte offset of the Adler-32, once the stream is known to end at the last byte
  TinfTabs T = {ll, dd, lcnt, lsym, dcnt, dsym, {0u, 0u}, {0u, 0u}};
  if (nbytes < 2u) {
    fail = kTiffFailShort;
  } else {
    need(0);
    const uint32_t h = (uint32_t)fetch(0);
    if (!tinf_zlib_ok(h & 255u, (h >> 8) & 255u)) fail = kTiffFailStream;
  }
  for (uint32_t guard = 0; guard <= nbits && !fail && o < dec; guard++) {
    if (!in_block) {
      // ================= a block header
      if (bfinal) {  // the last block ended and bytes are missing
        fail = kTiffFailShort;
        break;
      }
      if (bitpos + 3u > nbits) {
        fail = kTiffFailShort;
        break;
      }
      need(bitpos);
      const uint32_t hb = (uint32_t)fetch(bitpos);
      bfinal = hb & 1u;
      const uint32_t type = (hb >> 1) & 3u;
      bitpos += 3u;
      if (type == 3u) {
        fail = kTiffFailStream;
        break;
      }
      if (type == 0u) {  // stored: LEN, NLEN, then a wave-wide byte copy
        const uint32_t k = (bitpos + 7u) >> 3;
        if (k + 4u > nbytes) {
          fail = kTiffFailShort;
          break;
        }
        need(8u * k);
        const uint32_t ln = (uint32_t)fetch(8u * k), len = ln & 0xFFFFu;
        if (len != ((ln >> 16) ^ 0xFFFFu)) {
          fail = kTiffFailStream;
          break;
        }
        const uint32_t want = len < dec - o ? len : dec - o;
        if (k + 4u + want > nbytes) {
          fail = kTiffFailShort;
          break;
        }
        const DG_GLOBAL uint8_t *sp = gp<const uint8_t>(src + k + 4u);
        for (uint32_t t = lane; t < want; t += 64u) stb(o + t, sp[t]);
        sync();
        o += want;
        bitpos = 8u * (k + 4u + len);
        if (o == dec && want == len && bfinal) trailer = k + 4u + len;
        continue;
      }
      uint32_t nl = 288u, nd = 32u;
      if (type == 1u) {  // fixed
        for (uint32_t s = lane; s < 320u; s += 64u) lens[s] = (uint8_t)(s < 288u ? tinf_fixed_len(s) : 5u);
        __syncthreads();
      } else {  // dynamic: HLIT, HDIST, HCLEN, the code-length code, then the lengths
        if (bitpos + 14u > nbits) {
          fail = kTiffFailShort;
          break;
        }
        need(bitpos);
        const uint32_t hd = (uint32_t)fetch(bitpos);
        nl = 257u + (hd & 31u);
        nd = 1u + ((hd >> 5) & 31u);
        const uint32_t ncl = 4u + ((hd >> 10) & 15u);
        bitpos += 14u;
        if (nl > kTinfMaxLl || nd > kTinfMaxDd) {
          fail = kTiffFailStream;
          break;
        }
        if (bitpos + 3u * ncl > nbits) {
          fail = kTiffFailShort;
          break;
        }
        need(bitpos);
        if (lane < 19u) cllens[lane] = 0;
        __syncthreads();
        const uint32_t cl3 = (uint32_t)fetch(bitpos + 3u * (lane < 19u ? lane : 0u)) & 7u;  // (every lane: a cross-lane read)
        if (lane < ncl) cllens[tinf_cl_order(lane)] = (uint8_t)cl3;
        bitpos += 3u * ncl;
        __syncthreads();
        uint32_t ncodes;
        const int32_t left = tinf_build(cllens, 19u, clcnt, clsym, lane, &ncodes);
        if (left != 0) {  // zlib takes no incomplete code-length code
          fail = kTiffFailStream;
          break;
        }
        for (uint32_t i = lane; i < kTinfClSize; i += 64u) {
          const uint32_t w = tinf_walk(i, clcnt, clsym, 0u, TinfWalk{0u, 0u}, kTinfClBits);
          cltab[i] = (uint8_t)(w ? ((w >> 16) << 5) | (w & 31u) : 0u);
        }
        __syncthreads();
        // the lengths: 64 bit offsets per round, the tokens found by hopping
        const uint32_t total = nl + nd;
        uint32_t n = 0, prev = 0;
        while (n < total && !fail) {
          need(bitpos);
          const uint32_t tk = tinf_cl_token((uint32_t)fetch(bitpos + lane), cltab);
          uint32_t cur = 0;
          while (cur < 64u && n < total) {
            const uint32_t t = __shfl(tk, cur), nb = t & 255u, rep = (t >> 8) & 255u, s = t >> 16;
            if (bitpos + cur + nb > nbits) {
              fail = kTiffFailShort;
              break;
            }
            if (!t || (s == 16u && n == 0u) || n + rep > total) {  // no such code, nothing to repeat, past the counts
              fail = kTiffFailStream;
              break;
            }
            const uint32_t v = s < 16u ? s : s == 16u ? prev : 0u;
            for (uint32_t q = lane; q < rep; q += 64u) lens[n + q] = (uint8_t)v;
            n += rep;
            prev = v;
            cur += nb;
          }
          bitpos += cur;
        }
        if (fail) break;
        __syncthreads();
        if (lens[256] == 0) {  // no end-of-block code
          fail = kTiffFailStream;
          break;
        }
      }
      // ---- the two codes in canonical form and their primary tables
      uint32_t nc;
      int32_t left = tinf_build(lens, nl, lcnt, lsym, lane, &nc);
      bool ok = tinf_set_ok(left, nc, lcnt[1], true);
      left = tinf_build(lens + nl, nd, dcnt, dsym, lane, &nc);
      ok = ok && tinf_set_ok(left, nc, dcnt[1], true);
      if (!ok) {
        fail = kTiffFailStream;
        break;
      }
      for (uint32_t i = lane; i < kTinfLlSize; i += 64u) ll[i] = tinf_primary(i, lcnt, lsym, kTinfLlBits, false);
      for (uint32_t i = lane; i < kTinfDdSize; i += 64u) dd[i] = tinf_primary(i, dcnt, dsym, kTinfDdBits, true);
      T.lw = tinf_walk_from(lcnt, kTinfLlBits);
      T.dw = tinf_walk_from(dcnt, kTinfDdBits);
      __syncthreads();
      in_block = true;
      continue;
    }
    // ================= a token step: lane j decodes the token that would start at bit bitpos + j
    need(bitpos);
    const uint32_t bp = bitpos + lane;
    TinfTok t = tinf_token(fetch(bp), T);
    if (bp + t.nb > nbits) t.kind = kTinfPast;
    // ---- the real token starts: hop from one to the next
    uint64_t taken = 0;
    uint32_t cur = 0, stopk = kTinfLit;
    while (cur < 64u) {
      taken |= 1ull << cur;
      stopk = __shfl(t.kind, cur);
      if (stopk > kTinfMatch) break;
      cur += __shfl(t.nb, cur);
    }
    const bool tok = (taken >> lane) & 1ull, data = tok && t.kind <= kTinfMatch;
    const uint32_t nout = !data ? 0u : t.kind == kTinfLit ? 1u : t.val;
    uint32_t total;
    const uint32_t P = o + tinf_excl_scan(nout, lane, &total);
    // ---- what ends the decode badly, if it stands before the last byte: an invalid token, the data's end, a
    // distance before the segment's first byte
    const uint64_t badm = __ballot(tok && P < dec && (t.kind > kTinfEob || (t.kind == kTinfMatch && t.dist > P)));
    if (badm) {
      fail = __shfl(t.kind, (uint32_t)__builtin_ctzll(badm)) == kTinfPast ? kTiffFailShort : kTiffFailStream;
      break;
    }
    // ---- the bytes
    const uint32_t CL = data && P < dec ? (nout < dec - P ? nout : dec - P) : 0u;
    const bool match = CL > 0u && t.kind == kTinfMatch;
    const uint32_t S = P - t.dist, span = t.dist < CL ? t.dist : CL;
    const bool early = match && S + span <= o;  // every byte it reads was there before the step
    if (CL > 0u && t.kind == kTinfLit) {
      stb(P, t.val);
    } else if (early && CL <= kTinfShort) {
      uint32_t v[kTinfShort];
#pragma unroll
      for (uint32_t q = 0; q < kTinfShort; q++)
        if (q < CL) v[q] = ldb(S + tinf_src(q, t.dist, CL));
#pragma unroll
      for (uint32_t q = 0; q < kTinfShort; q++)
        if (q < CL) stb(P + q, v[q]);
    }
    uint64_t big = __ballot(early && CL > kTinfShort);
    const uint64_t late = __ballot(match && !early);
    for (uint32_t pass = 0; pass < 2u; pass++) {  // long early matches by the wave; then the late ones in token order
      while (big) {
        const uint32_t m = (uint32_t)__builtin_ctzll(big);
        big &= big - 1ull;
        const uint32_t Pb = __shfl(P, m), Sb = __shfl(S, m), Db = __shfl(t.dist, m), Cb = __shfl(CL, m);
        for (uint32_t q = lane; q < Cb; q += 64u) stb(Pb + q, ldb(Sb + tinf_src(q, Db, Cb)));
        if (pass) sync();
      }
      if (!pass) sync();
      big = pass ? 0ull : late;
    }
    // ---- the state after the step: bitpos is the end of the last token that gave a needed byte
    const uint64_t needm = __ballot(CL > 0u);
    if (needm) {
      const uint32_t last = 63u - (uint32_t)__builtin_clzll(needm);
      bitpos += last + __shfl(t.nb, last);
      exact = __shfl(P + nout, last) == dec;
    }
    o = o + total < dec ? o + total : dec;
    if (stopk == kTinfEob && o < dec) {  // the block ends (its code's lane is cur) and bytes are missing
      bitpos += __shfl(t.nb, cur);
      in_block = false;
    }
  }
  if (!fail && o < dec) fail = kTiffFailShort;
  // ---- the trailer: if the final block's end-of-block code follows the last byte directly
  if (!fail && in_block && bfinal && exact) {
    need(bitpos);
    const TinfTok t = tinf_token(fetch(bitpos), T);
    if (t.kind == kTinfEob && bitpos + t.nb <= nbits) trailer = (bitpos + t.nb + 7u) >> 3;
  }
  if (!fail && trailer != 0xFFFFFFFFu && trailer + 4u <= nbytes) {
    uint32_t a = 0, b = 0, w = (dec % kTinfAdlerMod + kTinfAdlerMod - 4u * lane) % kTinfAdlerMod;  // (dec - i) mod 65521
    for (uint32_t i = 4u * lane; i < dec; i += 256u) {
      const uint32_t v = in_lds ? *(const uint32_t *)(lout + i)
                                : __hip_atomic_load((DG_GLOBAL uint32_t *)(out + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tinf_adler4(v, dec - i, w, a, b);
      w = (w + kTinfAdlerMod - 256u) % kTinfAdlerMod;
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
      a = (a + __shfl_xor(a, d)) % kTinfAdlerMod;
      b = (b + __shfl_xor(b, d)) % kTinfAdlerMod;
    }
    const uint32_t sum = (((dec + b) % kTinfAdlerMod) << 16) | ((1u + a) % kTinfAdlerMod);
    const DG_GLOBAL uint8_t *tp = gp<const uint8_t>(src + trailer);
    const uint32_t want = ((uint32_t)tp[0] << 24) | ((uint32_t)tp[1] << 16) | ((uint32_t)tp[2] << 8) | tp[3];
    if (sum != want) fail = kTiffFailSum;
  }
  if (fail) {
    if (lane == 0) {
      im.tiff.fail = fail;
      im.status = 2;  // DG_ERR_CORRUPT
    }
    return;
  }
  if (in_lds) {  // the finished segment: LDS -> the decoded arena (its slot is a multiple of 16 bytes)
    __syncthreads();
    for (uint32_t i = 16u * lane; i < dec; i += 1024u) *(DG_GLOBAL u32x4 *)(out + i) = *(const u32x4 *)(lout + i);
  }
}

void launch_tiff_inflate(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_tiff_inflate, dim3(nwg), dim3(64), 0, st, imgs, list);
}

}  // namespace dg
