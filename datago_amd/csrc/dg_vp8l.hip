// dg_vp8l.hip — CDNA4 (gfx950) kernels of the lossless WebP decode (option "webp").
//
//   k_vp8l_decode    the VP8L bitstream after its header -> the transform list, the
//                    sub-images and the entropy-decoded ARGB plane, one wave per image
//   k_vp8l_inverse   the inverse transforms in reverse order of reading, one wave per
//                    image: in place, but colour indexing (wider rows) into the other plane
//   k_vp8l_store     ARGB u32 -> pix as RGB8 or RGBA8, 256 pixels per workgroup
//
// What they restate: libwebp's VP8L decoder (tests/ref_webp.py is the CPU form the
// tests compare to); dg_vp8l.h holds the wave-uniform walk and the lane routines.
//
// The symbol walk is serial: the group depends on the pixel position and the cache
// on every pixel before it, so a wave takes one pixel, copy or cache index at a
// time, all lanes in step.  The lanes work where the work is wide: clearing and
// filling code lengths, building the lookup tables (lanes over symbols), copies (64
// pixels per step) and the cache inserts after a copy (the last pixel per slot wins).
// What the wave stored and reads back (pixels under a copy, sub-images, tables of
// another group) is read past the L1 after the stores have drained, as in dg_gif.hip.
#include <hip/hip_runtime.h>

#include "dg_vp8l.h"
#include "kernels.h"

namespace dg {

__device__ __forceinline__ uint32_t vp8l_ld(const DG_GLOBAL uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void vp8l_drain() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

struct Vp8lLds {
  uint32_t first[6][256];
  uint32_t cnt[6][16];
  uint32_t cache[1u << kVp8lMaxCache];
  uint32_t tag[1u << kVp8lMaxCache];
  uint32_t win[kVp8lWinDwords];
  uint32_t cl_sorted[32];
  uint32_t bcnt[16];
  uint8_t lens[kVp8lLensBytes];
};

// The wave's side of the walk of dg_vp8l.h.  Every method is called by all 64 lanes with the same arguments.
struct Vp8lDev {
  Vp8lLds &s;
  DG_GLOBAL uint32_t *work;  // the image's work arena
  DG_GLOBAL uint32_t *tabs;  // its table area
  uint64_t a0, src_end;      // the aligned start of the source window's address space, one past the last byte
  uint32_t lane;
  uint32_t win0;             // first dword the window holds (~0: none)
  uint32_t cur;              // the group whose first[] / cnt[] the LDS holds

  __device__ uint32_t src_dword(uint32_t i) {
    if (win0 == ~0u || i - win0 >= kVp8lWinDwords) {
      __syncthreads();
      win0 = i;
#pragma unroll
      for (uint32_t r = 0; r < kVp8lWinDwords / 64u; r++) {
        const uint32_t j = lane + 64u * r;
        const uint64_t ad = a0 + 4ull * ((uint64_t)i + j);
        uint32_t v = 0;
        if (ad + 4u <= src_end) {
          v = *gp<const uint32_t>(ad);
        } else {
          for (uint32_t q = 0; q < 4; q++)
            if (ad + q < src_end) v |= (uint32_t)*gp<const uint8_t>(ad + q) << (8u * q);
        }
        s.win[j] = v;
      }
      __syncthreads();
    }
    return s.win[i - win0];
  }

  __device__ void lens_fill(uint32_t at, uint32_t n, uint32_t v) {
    if (n == 1u) {
      if (lane == 0 && at < kVp8lLensBytes) s.lens[at] = (uint8_t)v;
      return;
    }
    for (uint32_t i = lane; i < n; i += 64u)
      if (at + i < kVp8lLensBytes) s.lens[at + i] = (uint8_t)v;
  }

  __device__ uint32_t first(uint32_t k, uint32_t i) { return s.first[k][i]; }
  __device__ uint32_t cnt(uint32_t k, uint32_t l) { return s.cnt[k][l]; }
  __device__ uint32_t sorted(uint32_t k, uint32_t i) {
    if (k == 5u) return s.cl_sorted[i & 31u];
    return vp8l_ld(tabs + (size_t)cur * kVp8lGroupWords + 5u * 256u + 5u * 16u + kVp8lSortedOff[k] + i);
  }

  // lens[0..nsym) -> first / cnt in LDS slot k, the sorted symbols in group grp's area (k == 5: in LDS).
  __device__ bool build(uint32_t k, uint32_t nsym, uint32_t grp) {
    __syncthreads();  // the lengths
    if (lane < 16u) s.bcnt[lane] = 0u;
    __syncthreads();
    for (uint32_t i = lane; i < nsym; i += 64u) {
      const uint32_t l = s.lens[i];
      if (l) atomicAdd(&s.bcnt[l], 1u);
    }
    __syncthreads();
    uint32_t cn[16];
#pragma unroll
    for (uint32_t l = 0; l < 16u; l++) cn[l] = l ? s.bcnt[l] : 0u;
    const uint32_t kind = vp8l_code_kind(cn);
    if (!kind) return false;
    if (lane < 16u) s.cnt[k][lane] = cn_at(cn, lane);
    for (uint32_t i = lane; i < 256u; i += 64u) s.first[k][i] = 0u;
    __syncthreads();
    DG_GLOBAL uint32_t *so = tabs + (size_t)grp * kVp8lGroupWords + 5u * 256u + 5u * 16u + (k < 5u ? kVp8lSortedOff[k] : 0u);
    uint32_t code = 0, off = 0;
#pragma unroll
    for (uint32_t l = 1; l < 16u; l++) {
      code = (code + cn[l - 1u]) << 1;
      if (cn[l]) {
        uint32_t run = 0;
        for (uint32_t base = 0; base < nsym; base += 64u) {
          const uint32_t sym = base + lane;
          const bool mine = sym < nsym && s.lens[sym] == l;
          const uint64_t m = __ballot(mine);
          if (mine) {
            const uint32_t r = run + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (k == 5u)
              s.cl_sorted[(off + r) & 31u] = sym;
            else
              so[off + r] = sym;
            if (kind == 1u) {
              for (uint32_t j = 0; j < 256u; j++) s.first[k][j] = kVp8lValid | sym;
            } else if (l <= 8u) {
              const uint32_t ent = kVp8lValid | (l << 16) | sym;
              for (uint32_t j = vp8l_rev(code + r, l); j < 256u; j += 1u << l) s.first[k][j] = ent;
            }
          }
          run += (uint32_t)__popcll(m);
        }
        off += cn[l];
      }
    }
    __syncthreads();
    return true;
  }
  static __device__ __forceinline__ uint32_t cn_at(const uint32_t (&cn)[16], uint32_t i) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t l = 0; l < 16u; l++) v = i == l ? cn[l] : v;
    return v;
  }

  // The group's five first[] / cnt[] from the LDS to its area, and back.
  __device__ void save(uint32_t g) {
    DG_GLOBAL uint32_t *t = tabs + (size_t)g * kVp8lGroupWords;
    for (uint32_t i = lane; i < 5u * 256u; i += 64u) t[i] = (&s.first[0][0])[i];
    for (uint32_t i = lane; i < 5u * 16u; i += 64u) t[5u * 256u + i] = (&s.cnt[0][0])[i];
    cur = g;
    vp8l_drain();
  }
  __device__ void select(uint32_t g) {
    if (g == cur) return;
    __syncthreads();
    const DG_GLOBAL uint32_t *t = tabs + (size_t)g * kVp8lGroupWords;
    for (uint32_t i = lane; i < 5u * 256u; i += 64u) (&s.first[0][0])[i] = vp8l_ld(t + i);
    for (uint32_t i = lane; i < 5u * 16u; i += 64u) (&s.cnt[0][0])[i] = vp8l_ld(t + 5u * 256u + i);
    cur = g;
    __syncthreads();
  }

  __device__ void work_store(uint64_t at, uint32_t v) {
    if (lane == 0) work[at] = v;
  }
  // a pixel of the entropy image: max_group drained its stores, nothing writes it afterwards
  __device__ uint32_t meta_load(uint64_t at) { return vp8l_ld(work + at); }
  __device__ void cache_clear(uint32_t bits) {
    __syncthreads();
    for (uint32_t i = lane; i < (1u << bits); i += 64u) {
      s.cache[i] = 0u;
      s.tag[i] = 0u;
    }
    __syncthreads();
  }
  __device__ uint32_t cache_get(uint32_t i) { return s.cache[i]; }
  __device__ void cache_put(uint32_t i, uint32_t v) {
    if (lane == 0) s.cache[i] = v;
    __syncthreads();
  }

  // len pixels from dist back, 64 per step; then their cache inserts, in pixel order per slot.
  __device__ void copy(uint64_t dst, uint32_t pos, uint32_t dist, uint32_t len, uint32_t cache_bits) {
    vp8l_drain();
    DG_GLOBAL uint32_t *p = work + dst;
    for (uint32_t t0 = 0; t0 < len; t0 += 64u) {
      const uint32_t t = t0 + lane;
      const bool on = t < len;
      uint32_t v = 0;
      if (on) {
        v = vp8l_ld(p + vp8l_copy_src(pos, dist, t));
        p[pos + t] = v;
      }
      if (cache_bits) {
        const uint32_t slot = vp8l_cache_slot(v, cache_bits);
        if (on) atomicMax(&s.tag[slot], lane + 1u);
        __syncthreads();
        if (on && s.tag[slot] == lane + 1u) s.cache[slot] = v;
        __syncthreads();
        if (on) s.tag[slot] = 0u;
        __syncthreads();
      }
    }
  }

  __device__ uint32_t max_group(uint64_t at, uint32_t n) {
    vp8l_drain();
    uint32_t m = 0;
    for (uint32_t i = lane; i < n; i += 64u) {
      const uint32_t g = (vp8l_ld(work + at + i) >> 8) & 0xffffu;
      m = g > m ? g : m;
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
      const uint32_t o = __shfl_xor(m, d);
      m = o > m ? o : m;
    }
    return m;
  }

  // The colour table's entries are deltas to the entry before, per byte: an inclusive scan.
  __device__ void pal_delta(uint64_t at, uint32_t n) {
    vp8l_drain();
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 64u) {
      const uint32_t i = b0 + lane;
      uint32_t v = i < n ? vp8l_ld(work + at + i) : 0u;
#pragma unroll
      for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v = vp8l_add(v, o);
      }
      v = vp8l_add(v, carry);
      if (i < n) work[at + i] = v;
      carry = __shfl(v, 63);
    }
    vp8l_drain();
  }
};

__global__ __launch_bounds__(64) void k_vp8l_decode(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  __shared__ Vp8lLds lds;
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const Vp8lDesc d = im.vp8l;
  Vp8lDev e = {lds, gp<uint32_t>(d.work), gp<uint32_t>(d.tabs), d.src & ~3ull, d.src_end, threadIdx.x, ~0u, ~0u};
  Vp8lBits b;
  vp8l_open(e, b, (uint32_t)(d.src & 3ull), d.nbytes);
  Vp8lWalk o;
  const uint32_t fail = vp8l_walk(e, b, im.width, im.height, d.groups_cap, o, d.alph != 0u);
  if (threadIdx.x == 0) {
    im.vp8l.ntrans = o.ntrans;
    for (uint32_t i = 0; i < 4u; i++) im.vp8l.trans[i] = i < o.ntrans ? o.trans[i] : 0u;
    im.vp8l.xsize = o.xsize;
    im.vp8l.npal = o.npal;
    if (fail) {
      im.vp8l.fail = fail;
      im.status = fail == kVp8lFailGroups ? 1 : 2;  // DG_ERR_UNSUPPORTED / DG_ERR_CORRUPT
    }
  }
}

// ------------------------------------------------------------ inverse transforms

// The predictor, in place, over strips of 64 rows (dg_vp8l.h): lane r owns row y0 + r and stands at
// x = t - 2r in step t.  Its left pixel is its own last value; TR, T, TL are lane r - 1's values of
// the last three steps.  Lane 0 of a strip below the first reads the row above from the plane.
__device__ void vp8l_inv_predictor(DG_GLOBAL uint32_t *px, const DG_GLOBAL uint32_t *sub, uint32_t w, uint32_t h,
                                   uint32_t bits, uint32_t lane) {
  const uint32_t bw = vp8l_div_up(w, bits);
  const uint32_t steps = vp8l_strip_steps(w);
  for (uint32_t y0 = 0; y0 < h; y0 += 64u) {
    vp8l_drain();  // the strip above
    const uint32_t y = y0 + lane;
    const bool row = y < h;
    DG_GLOBAL uint32_t *pr = px + (size_t)y * w;
    const DG_GLOBAL uint32_t *mr = sub + (size_t)(y >> bits) * bw;
    const bool above = lane == 0u && y0 != 0u;  // this lane's T / TL / TR come from the plane
    uint32_t h1 = 0, h2 = 0, h3 = 0;            // this lane's values of the last three steps
    uint32_t a1 = above ? vp8l_ld(pr - w) : 0u, a2 = 0;  // the row above at x and x - 1
    uint32_t firstpx = 0;
    for (uint32_t t0 = 0; t0 < steps; t0 += 8u) {
      uint32_t res[8], mode[8], up[8];
#pragma unroll
      for (uint32_t q = 0; q < 8u; q++) {  // the loads of eight steps in flight
        const uint32_t x = t0 + q - 2u * lane;  // (below zero it wraps: then >= w)
        const bool on = row && x < w;
        res[q] = on ? pr[x] : 0u;
        mode[q] = on ? (mr[x >> bits] >> 8) & 15u : 0u;
        up[q] = (on && above && x + 1u < w) ? vp8l_ld(pr - w + x + 1u) : 0u;
      }
#pragma unroll
      for (uint32_t q = 0; q < 8u; q++) {
        const uint32_t x = t0 + q - 2u * lane;
        const bool on = row && x < w;
        uint32_t TR = __shfl_up(h1, 1), T = __shfl_up(h2, 1), TL = __shfl_up(h3, 1);
        if (above) {
          TR = up[q];
          T = a1;
          TL = a2;
        }
        uint32_t v = 0;
        if (on) {
          if (x + 1u == w) TR = firstpx;  // the format's wrap: the next pixel in memory
          uint32_t p;
          if (y == 0u)
            p = x ? h1 : 0xff000000u;
          else if (x == 0u)
            p = T;
          else
            p = vp8l_predict(mode[q], h1, T, TL, TR);
          v = vp8l_add(res[q], p);
          pr[x] = v;
          if (x == 0u) firstpx = v;
          a2 = a1;
          a1 = up[q];
        }
        h3 = h2;
        h2 = h1;
        h1 = v;
      }
    }
  }
}

__global__ __launch_bounds__(64) void k_vp8l_inverse(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const Vp8lDesc d = im.vp8l;
  const uint32_t lane = threadIdx.x, W = im.width, H = im.height;
  DG_GLOBAL uint32_t *work = gp<uint32_t>(d.work);
  uint32_t cur = 0;
  for (uint32_t ti = d.ntrans; ti-- > 0u;) {
    const uint32_t t = d.trans[ti], type = t & 3u, bits = (t >> 2) & 15u, xs = t >> 8;
    DG_GLOBAL uint32_t *px = work + vp8l_plane_off(W, H, cur);
    const uint32_t n = xs * H;
    if (type == kVp8lPredictor) {
      vp8l_inv_predictor(px, work + vp8l_sub_off(W, H, 0u), xs, H, bits, lane);
    } else if (type == kVp8lColor) {
      const DG_GLOBAL uint32_t *sub = work + vp8l_sub_off(W, H, 1u);
      const uint32_t bw = vp8l_div_up(xs, bits);
      for (uint32_t i = lane; i < n; i += 64u) {
        const uint32_t y = i / xs, x = i - y * xs;
        px[i] = vp8l_color_inv(sub[(y >> bits) * bw + (x >> bits)], px[i]);
      }
    } else if (type == kVp8lGreenT) {
      for (uint32_t i = lane; i < n; i += 64u) px[i] = vp8l_green_inv(px[i]);
    } else {  // colour indexing widens the rows: into the other plane
      DG_GLOBAL uint32_t *dst = work + vp8l_plane_off(W, H, cur ^ 1u);
      const DG_GLOBAL uint32_t *pal = work + vp8l_pal_off(W, H);
      const uint32_t pw = vp8l_div_up(xs, bits);
      for (uint32_t i = lane; i < n; i += 64u) {
        const uint32_t y = i / xs, x = i - y * xs;
        const uint32_t k = vp8l_index_of(px[y * pw + (x >> bits)], x, bits);
        dst[i] = k < d.npal ? pal[k] : 0u;
      }
      cur ^= 1u;
    }
    __threadfence();  // the next transform reads what this one stored
  }
  if (lane == 0) im.vp8l.final_plane = cur;
}

// ARGB -> RGB8 / RGBA8, one pixel per thread.
__global__ __launch_bounds__(256) void k_vp8l_store(const ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  const ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const uint32_t idx = it.item0 + threadIdx.x, W = im.width;
  if (idx >= W * im.height) return;
  const uint32_t y = idx / W, x = idx - y * W;
  const uint32_t p = (gp<const uint32_t>(im.vp8l.work) + vp8l_plane_off(W, im.height, im.vp8l.final_plane))[idx];
  DG_GLOBAL uint8_t *o = gp<uint8_t>(im.pix) + (size_t)y * im.pix_stride + (size_t)x * im.dec_c;
  o[0] = (uint8_t)(p >> 16);
  o[1] = (uint8_t)(p >> 8);
  o[2] = (uint8_t)p;
  if (im.dec_c == 4u) o[3] = (uint8_t)(p >> 24);
}

// ------------------------------------------------------------ launchers

void launch_vp8l_decode(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_vp8l_decode, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_vp8l_inverse(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_vp8l_inverse, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_vp8l_store(hipStream_t st, const ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_vp8l_store, dim3(nwg), dim3(256), 0, st, imgs, list);
}

}  // namespace dg
