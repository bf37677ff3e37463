// dg_vp8.hip — CDNA4 (gfx950) kernels of the lossy WebP decode (option "webp_lossy").
//
//   k_vp8_parse    the VP8 key frame's first partition (header, per-MB modes) and token
//                  partitions -> per-MB records and dequantised coefficients, one wave per image
//   k_vp8_recon    intra prediction + inverse DCT into unfiltered Y / U / V planes, one
//                  workgroup per image over the anti-diagonals x + 2y = d, one wave per MB
//   k_vp8_filter   the loop filter, simple or normal, in place, with the same stepping
//   k_vp8_rgb      fancy chroma upsampling + YUV -> RGB into pix, 256 pixels per workgroup; with an
//                  alpha plane (option "webp_alpha", dg_alph.hip) RGBA, the plane's byte fourth
//
// What they restate: libwebp's VP8 decoder (tests/ref_vp8.py is the CPU form the tests
// compare to); dg_vp8.h holds every statement of the walk, shared with the CPU emulation.
//
// The bool decoder is serial, so k_vp8_parse keeps all lanes in step and lets them work
// where the work is wide (dg_vp8.h says where).  Order between waves comes only from
// __syncthreads inside a workgroup and from kernel boundaries: MB (x, y) needs
// (x-1, y), (x, y-1), (x-1, y-1) and (x+1, y-1), all on earlier diagonals, and the loop
// filter's raster order reduces to the same four.  No wave waits on a flag.
#include <hip/hip_runtime.h>

#include "dg_vp8.h"
#include "kernels.h"

namespace dg {

// What the wave stored (LDS or arena) before, its other lanes may load after.
__device__ __forceinline__ void vp8_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The arena side of an environment of dg_vp8.h: every offset lies inside layout_vp8's bytes.
struct Vp8Arena {
  DG_GLOBAL uint8_t *work;
  uint32_t lane;

  template <class F>
  __device__ __forceinline__ void lanes(F f) {
    vp8_wave_sync();
    f(lane);
    vp8_wave_sync();
  }
  __device__ __forceinline__ uint32_t r8(uint64_t off) { return work[off]; }
  __device__ __forceinline__ int32_t r16(uint64_t off) { return *(const DG_GLOBAL int16_t *)(work + off); }
  __device__ __forceinline__ void w8(uint64_t off, uint32_t v) { work[off] = (uint8_t)v; }
  __device__ __forceinline__ void w32(uint64_t off, uint32_t v) { *(DG_GLOBAL uint32_t *)(work + off) = v; }
};

struct Vp8ParseDev : Vp8Arena {
  Vp8ParseState &s;
  const DG_GLOBAL uint8_t *src;  // the VP8 chunk
  uint32_t nbytes;

  __device__ Vp8ParseDev(Vp8ParseState &st, DG_GLOBAL uint8_t *w, const DG_GLOBAL uint8_t *sr, uint32_t n, uint32_t ln)
      : Vp8Arena{w, ln}, s(st), src(sr), nbytes(n) {}
  __device__ __forceinline__ uint32_t src8(uint32_t i) { return i < nbytes ? src[i] : 0u; }
  __device__ __forceinline__ uint32_t src_be32(uint32_t i) {
    if ((uint64_t)i + 4u > nbytes) return 0u;
    return ((uint32_t)src[i] << 24) | ((uint32_t)src[i + 1u] << 16) | ((uint32_t)src[i + 2u] << 8) | src[i + 3u];
  }
};

__global__ __launch_bounds__(64) void k_vp8_parse(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  __shared__ Vp8ParseState lds;
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const Vp8Desc d = im.vp8;
  Vp8ParseDev e(lds, gp<uint8_t>(d.work), gp<const uint8_t>(d.src), d.nbytes, threadIdx.x);
  Vp8Frame fr;
  const uint32_t fail = vp8_parse(e, im.width, im.height, d.nbytes, d.part0, fr);
  if (threadIdx.x == 0) {
    im.vp8.filter_type = fr.filter_type;
    if (fail) {
      im.vp8.fail = fail;
      im.status = 2;  // DG_ERR_CORRUPT
    }
  }
}

// One workgroup per image, one wave per MB of the current diagonal.
template <bool kFilter>
__device__ __forceinline__ void vp8_diagonals(const ImageDesc &im) {
  __shared__ Vp8ReconBuf bufs[kVp8ReconWaves];
  const Vp8Desc d = im.vp8;
  const Vp8Layout L = layout_vp8(im.width, im.height);
  Vp8Arena e = {gp<uint8_t>(d.work), threadIdx.x & 63u};
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t nd = vp8_diag_count(L.mbw, L.mbh);
  for (uint32_t dg = 0; dg < nd; dg++) {
    uint32_t y0, cnt;
    vp8_diag_rows(L.mbw, L.mbh, dg, y0, cnt);
    for (uint32_t k = wave; k < cnt; k += kVp8ReconWaves) {
      const uint32_t my = y0 + k, mx = dg - 2u * my;
      if (kFilter)
        vp8_filter_mb(e, L, d.filter_type, mx, my);
      else
        vp8_recon_mb(e, bufs[wave], L, mx, my);
    }
    __syncthreads();  // the next diagonal reads what this one stored
  }
}

__global__ __launch_bounds__(64 * kVp8ReconWaves) void k_vp8_recon(const ImageDesc *__restrict__ imgs,
                                                                    const WgItem *__restrict__ list) {
  const ImageDesc &im = imgs[list[blockIdx.x].image];
  if (im.status) return;
  vp8_diagonals<false>(im);
}

__global__ __launch_bounds__(64 * kVp8ReconWaves) void k_vp8_filter(const ImageDesc *__restrict__ imgs,
                                                                     const WgItem *__restrict__ list) {
  const ImageDesc &im = imgs[list[blockIdx.x].image];
  if (im.status || !im.vp8.filter_type) return;
  vp8_diagonals<true>(im);
}

__global__ __launch_bounds__(256) void k_vp8_rgb(const ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  const WgItem it = list[blockIdx.x];
  const ImageDesc &im = imgs[it.image];
  if (im.status) return;
  const uint32_t idx = it.item0 + threadIdx.x, W = im.width, H = im.height;
  if (idx >= W * H) return;
  const uint32_t y = idx / W, x = idx - y * W;
  Vp8Arena e = {gp<uint8_t>(im.vp8.work), threadIdx.x & 63u};
  const uint32_t p = vp8_rgb_px(e, layout_vp8(W, H), W, H, x, y);
  DG_GLOBAL uint8_t *o = gp<uint8_t>(im.pix) + (size_t)y * im.pix_stride + (size_t)x * im.dec_c;
  o[0] = (uint8_t)p;
  o[1] = (uint8_t)(p >> 8);
  o[2] = (uint8_t)(p >> 16);
  if (im.dec_c == 4u) o[3] = gp<const uint8_t>(im.vp8.alph_plane)[idx];
}

// ------------------------------------------------------------ launchers

void launch_vp8_parse(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_vp8_parse, dim3(nwg), dim3(64), 0, st, imgs, list);
}
void launch_vp8_recon(hipStream_t st, const ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_vp8_recon, dim3(nwg), dim3(64 * kVp8ReconWaves), 0, st, imgs, list);
}
void launch_vp8_filter(hipStream_t st, const ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_vp8_filter, dim3(nwg), dim3(64 * kVp8ReconWaves), 0, st, imgs, list);
}
void launch_vp8_rgb(hipStream_t st, const ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_vp8_rgb, dim3(nwg), dim3(256), 0, st, imgs, list);
}

}  // namespace dg
