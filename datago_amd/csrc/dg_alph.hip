// dg_alph.hip — CDNA4 (gfx950) kernel of the alpha plane of a lossy WebP (option "webp_alpha").
//
//   k_alph_plane   the ALPH chunk's filtered plane, raw bytes in the file or the green
//                  channel of the companion descriptor's VP8L plane, -> the unfiltered
//                  plane in the image's arena; one wave per work item (dg_alph.h says
//                  what an item is for each filter)
//
// k_vp8_rgb (dg_vp8.hip) then stores the plane as the fourth channel of pix.  What it
// restates: libwebp's alpha unfilter (tests/ref_alph.py is the CPU form the tests compare
// to); dg_alph.h holds every statement, shared with the CPU emulation.
//
// The companion's stream is decoded by k_vp8l_decode / k_vp8l_inverse before this kernel
// on the same stream.  When it failed, item 0 hands its status to the image, so that no
// later kernel touches the image and the host finds the failure in the image's own
// descriptor.  Order inside the wave comes from the wave barrier of lanes(); the
// gradient walk reads back what the wave stored past the L1, as dg_vp8l.hip does.
#include <hip/hip_runtime.h>

#include "dg_alph.h"
#include "dg_vp8l.h"
#include "kernels.h"

namespace dg {

struct AlphDev {
  uint32_t *shw;                    // kAlphShWords of LDS
  const DG_GLOBAL uint8_t *raw;     // the raw filtered plane, or null
  const DG_GLOBAL uint32_t *argb;   // the VP8L plane otherwise
  DG_GLOBAL uint8_t *out;           // width x height bytes, the allocation a whole number of dwords
  uint32_t lane;

  template <class F>
  __device__ __forceinline__ void lanes(F f) {
    sync();
    f(lane);
    sync();
  }
  // Order through the LDS alone: a wave's LDS operations complete in the order it issues them.
  template <class F>
  __device__ __forceinline__ void lanes_sh(F f) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    f(lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __device__ __forceinline__ uint32_t g(uint32_t i) { return raw ? raw[i] : (argb[i] >> 8) & 255u; }
  __device__ __forceinline__ void put(uint32_t i, uint32_t v) { out[i] = (uint8_t)v; }
  __device__ __forceinline__ uint32_t get(uint32_t i) {
    const uint32_t v = __hip_atomic_load((const DG_GLOBAL uint32_t *)out + (i >> 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (v >> (8u * (i & 3u))) & 255u;
  }
  __device__ __forceinline__ uint32_t &sh(uint32_t k) { return shw[k]; }
};

__global__ __launch_bounds__(64) void k_alph_plane(ImageDesc *__restrict__ imgs, const WgItem *__restrict__ list) {
  __shared__ uint32_t shw[kAlphShWords];
  const WgItem it = list[blockIdx.x];
  ImageDesc &im = imgs[it.image];
  const Vp8Desc d = im.vp8;
  const uint32_t W = im.width, H = im.height;
  const DG_GLOBAL uint32_t *argb = nullptr;
  if (!d.alph_src) {
    const ImageDesc &co = imgs[d.alph_desc];
    const uint32_t cs = co.status;
    if (cs) {  // the alpha stream failed: the image fails with it
      if (it.item0 == 0u && threadIdx.x == 0u) {
        im.vp8.alph_fail = cs;
        if (!im.status) im.status = cs;
      }
      return;
    }
    argb = gp<const uint32_t>(co.vp8l.work) + vp8l_plane_off(W, H, co.vp8l.final_plane);
  }
  if (im.status) return;
  AlphDev e = {shw, d.alph_src ? gp<const uint8_t>(d.alph_src) : nullptr, argb, gp<uint8_t>(d.alph_plane), threadIdx.x};
  alph_unfilter(e, d.alph_filter, W, H, it.item0);
}

void launch_alph_plane(hipStream_t st, ImageDesc *imgs, const WgItem *list, uint32_t nwg) {
  if (nwg) hipLaunchKernelGGL(k_alph_plane, dim3(nwg), dim3(64), 0, st, imgs, list);
}

}  // namespace dg
