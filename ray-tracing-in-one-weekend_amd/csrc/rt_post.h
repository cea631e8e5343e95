// rt_post.h -- internal: what the image-space passes over the rt_aov sums
// (the denoiser in rt_denoise.hip, temporal accumulation in rt_temporal.hip)
// share on the device -- the global address space, the unfused dot product,
// the 16 x 16 pixel tile, the frame size limit and the guide preparation.
//
// Their arithmetic is written operation by operation, without fmaf, so that
// the numpy restatements (tests/post_ref.py and its two users) round the same
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
