// rt_post.h -- internal: what the image-space passes over the rt_aov sums
// (the denoiser in rt_denoise.hip, temporal accumulation in rt_temporal.hip,
// the resolve in rt_resolve.hip, upsampling in rt_upscale.hip) share -- on the
// device the global address space, the unfused dot product, the 16 x 16 pixel
// tile and the guide preparation; on the host the frame size limit and the
// argument rules (overlap, alignment, "0 = default" options).  What only the
// passes that reproject share is in rt_reproject.h, which includes this.
//
// Their arithmetic is written operation by operation, without fmaf, so that
// the numpy restatements (tests/post_ref.py and its users) round the same
// way.  csrc/rt_device.h's dot3 is the fused one: this header does not include
// it, and a pass that includes this one compiles none of the render's device
// helpers and no g_turn_tab.
#ifndef RTOW_RT_POST_H
#define RTOW_RT_POST_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_layout.h"

namespace rtk {

#define RT_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ RT_GLOBAL T *as_global(T *p) {
  return (RT_GLOBAL T *)p;
}

constexpr int kPostTile = 16;  // 16 x 16 pixels per block: a wave is 16 x 4, its rows 256-byte runs of a plane
constexpr int kPostMaxDim = 32768;

inline bool post_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= kPostMaxDim && h <= kPostMaxDim; }
inline dim3 post_grid(int w, int h) {
  return dim3((unsigned)((w + kPostTile - 1) / kPostTile), (unsigned)((h + kPostTile - 1) / kPostTile));
}

// The argument rules the passes' resolve() functions share.
// np bytes at p and nq bytes at q have a byte in common (neither NULL)
inline bool overlap(const void *p, size_t np, const void *q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + nq && b < a + np;
}
// a buffer read and written as float4 (NULL passes)
inline bool post_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// An option of a desc, where 0 asks for the default: v, the effective value.
// false: v lies outside lo .. hi (lo itself only where lo_in), or is NaN
template <typename T>
inline bool post_option(T given, T dflt, T lo, bool lo_in, T hi, T &v) {
  v = given == T(0) ? dflt : given;
  return (lo_in ? v >= lo : v > lo) && v <= hi;
}

// the pixel of this lane in a post_grid launch of 256 threads; false: outside the frame
__device__ __forceinline__ bool post_pixel(int width, int height, int &x, int &y) {
  x = (int)blockIdx.x * kPostTile + (int)(threadIdx.x & (kPostTile - 1));
  y = (int)blockIdx.y * kPostTile + (int)(threadIdx.x / kPostTile);
  return x < width && y < height;
}

// (ax bx + ay by) + az bz, every operation rounded
__device__ __forceinline__ float dot3_unfused(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

// A pixel's guides from its rt_aov sums (h hits, g_p / g_n its three position
// / normal sums): the unit mean normal, 0 where the mean is 0, and the mean
// position; a sky pixel (no hits) has both 0.
struct post_guide {
  float nx, ny, nz, px, py, pz;
  bool sky;
};
__device__ __forceinline__ post_guide post_prepare(uint32_t h, const RT_GLOBAL float *g_p,
                                                   const RT_GLOBAL float *g_n) {
  post_guide g;
  g.sky = h == 0;
  const float hf = (float)h;
  const float ux = g_n[0] / hf, uy = g_n[1] / hf, uz = g_n[2] / hf;
  const float nn = dot3_unfused(ux, uy, uz, ux, uy, uz);
  const float len = __builtin_sqrtf(nn);
  const bool unit = !g.sky && nn > 0.0f;
  g.nx = unit ? ux / len : 0.0f;
  g.ny = unit ? uy / len : 0.0f;
  g.nz = unit ? uz / len : 0.0f;
  g.px = g.sky ? 0.0f : g_p[0] / hf;
  g.py = g.sky ? 0.0f : g_p[1] / hf;
  g.pz = g.sky ? 0.0f : g_p[2] / hf;
  return g;
}

}  // namespace rtk

#endif  // RTOW_RT_POST_H
