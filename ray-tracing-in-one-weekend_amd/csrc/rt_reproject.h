// rt_reproject.h -- internal: what the passes that look a point up in another
// frame share.  temporal accumulation (rt_temporal.hip) and the clamped resolve
// (rt_resolve.hip) share all of it: the projection through a rt_temporal_view,
// the four-tap history gather, the running-length blend and the history write.
// Guided upsampling (rt_upscale.hip) shares the projection and, with the
// resolve, a pixel's centre ray.  On the host: the leading part of the two
// history passes' kernel parameters and the precheck of the two
// *_from_camera builders.
//
// The arithmetic is written operation by operation, as rt_post.h's, so that the
// numpy restatements (tests/temporal_ref.py: project, gather, blend,
// pack_history; tests/resolve_ref.py: centre_rays) round the same way.
#ifndef RTOW_RT_REPROJECT_H
#define RTOW_RT_REPROJECT_H

#include <cmath>

#include "rt_post.h"
#include "rt_temporal.h"
#include "rt_resolve.h"

namespace rtk {

// rt_temporal.h's "View": a vector q relative to the view's eye -> w and the
// pixel coordinates (x, y).  A point P is passed as P - eye, a ray as its
// direction.
__device__ __forceinline__ void rp_project(const rt_temporal_view &v, float qx, float qy, float qz, float &w, float &x,
                                           float &y) {
  w = dot3_unfused(v.pw[0], v.pw[1], v.pw[2], qx, qy, qz);
  x = dot3_unfused(v.px[0], v.px[1], v.px[2], qx, qy, qz) / w - v.x0;
  y = dot3_unfused(v.py[0], v.py[1], v.py[2], qx, qy, qz) / w - v.y0;
}

// rt_resolve.h's "Rays": the unnormalised direction through the centre of pixel (x, y)
__device__ __forceinline__ void rp_centre_ray(const rt_resolve_rays &r, int x, int y, float D[3]) {
  const float xf = (float)x, yf = (float)y;
#pragma unroll
  for (int k = 0; k < 3; ++k) D[k] = (r.d00[k] + xf * r.du[k]) + yf * r.dv[k];
}

// The leading part of temporal_kernel's and resolve_kernel's parameters
struct rp_params {
  int width, height;
  float width_f, height_f;
  float spp_f;
  float max_len_f;
  float pt2;  // plane_tol^2
  float normal_cos;
  int plane_test, normal_test;  // 0: the test is left out
  rt_temporal_view prev;
};
// from the EFFECTIVE options (the desc's "0 = default" rule applied)
inline void rp_fill(rp_params &a, int width, int height, int spp, int max_len, float plane_tol, float normal_cos,
                    const rt_temporal_view &prev) {
  a.width = width;
  a.height = height;
  a.width_f = (float)width;
  a.height_f = (float)height;
  a.spp_f = (float)spp;
  a.max_len_f = (float)max_len;
  a.pt2 = plane_tol * plane_tol;
  a.normal_cos = normal_cos;
  a.plane_test = !std::isinf(plane_tol);
  a.normal_test = normal_cos != -1.0f;
  a.prev = prev;
}

// rt_temporal.h's step 4: the bilinear sums over the up to four history pixels
// around (x, y) that lie on the surface of the pixel (g: its unit normal and P;
// lim = pt2 |P - eye|^2).  A tap outside the frame, on sky or on another
// surface is skipped per lane (its loads are predicated, so no lane reads
// outside the planes); the sums stay 0 where (w, x, y), a
// rp_project result, is off the frame or no tap is left.
struct rp_taps {
  float w, r, g, b, l;
};
__device__ __forceinline__ rp_taps rp_gather(const rp_params &a, float w, float x, float y, const post_guide &g,
                                             float lim, const f4 *hist_in) {
  rp_taps s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (!(w > 0.0f && x > -1.0f && x < a.width_f && y > -1.0f && y < a.height_f)) return s;
  const float xf = __builtin_floorf(x), yf = __builtin_floorf(y);
  const float fx = x - xf, fy = y - yf;
  const int xi = (int)xf, yi = (int)yf;  // -1 .. W-1, -1 .. H-1
  const size_t npx = (size_t)a.width * (size_t)a.height;
  const RT_GLOBAL f4 *__restrict__ h0 = as_global(hist_in);
  const RT_GLOBAL f4 *__restrict__ h1 = h0 + npx;
  const RT_GLOBAL f4 *__restrict__ h2 = h1 + npx;
#pragma unroll
  for (int dy = 0; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = 0; dx <= 1; ++dx) {
      const int tx = xi + dx, ty = yi + dy;
      if (tx < 0 || tx >= a.width || ty < 0 || ty >= a.height) continue;
      const size_t t = (size_t)ty * (size_t)a.width + (size_t)tx;
      const f4 pt = h1[t];
      if (pt.w != 0.0f) continue;
      const f4 nt = h2[t];
      const float e = dot3_unfused(g.nx, g.ny, g.nz, pt.x - g.px, pt.y - g.py, pt.z - g.pz);
      if (a.plane_test && !(e * e <= lim)) continue;
      const float c = dot3_unfused(g.nx, g.ny, g.nz, nt.x, nt.y, nt.z);
      if (a.normal_test && !(c >= a.normal_cos)) continue;
      const f4 ct = h0[t];
      const float b = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy);
      s.w += b;
      s.r += b * ct.x;
      s.g += b * ct.y;
      s.b += b * ct.z;
      s.l += b * ct.w;
    }
  }
  return s;
}

// Step 5: the history's mean colour h (clamped by the caller where it clamps)
// and length hl, blended with the new colour c -> m and the new length
__device__ __forceinline__ void rp_blend(float hr, float hg, float hb, float hl, float cr, float cg, float cb,
                                         float max_len_f, float &mr, float &mg, float &mb, float &len) {
  const float t = hl + 1.0f;
  len = t < max_len_f ? t : max_len_f;
  const float al = 1.0f / len;
  mr = hr + (cr - hr) * al;
  mg = hg + (cg - hg) * al;
  mb = hb + (cb - hb) * al;
}

// Step 6: pixel o's three history planes (m and len; P and the sky flag; n)
// and, where out is not NULL, its sums at o3 = 3 * o.  The helpers take
// scalars and the caller's own 3 * o: with arrays or an offset formed here
// the kernels' instruction streams drift from what they were before the
// steps were shared (profiles/history_share_ab.log).
__device__ __forceinline__ void rp_write(f4 *hist_out, float *out, size_t npx, size_t o, size_t o3, float m0,
                                         float m1, float m2, float len, const post_guide &g, float spp_f) {
  RT_GLOBAL f4 *o0 = as_global(hist_out);
  f4 v;
  v.x = m0;
  v.y = m1;
  v.z = m2;
  v.w = len;
  o0[o] = v;
  v.x = g.px;
  v.y = g.py;
  v.z = g.pz;
  v.w = g.sky ? 1.0f : 0.0f;
  o0[npx + o] = v;
  v.x = g.nx;
  v.y = g.ny;
  v.z = g.nz;
  v.w = 0.0f;
  o0[2 * npx + o] = v;
  if (out) {
    RT_GLOBAL float *q = as_global(out) + o3;
    q[0] = m0 * spp_f;
    q[1] = m1 * spp_f;
    q[2] = m2 * spp_f;
  }
}

// What rt_temporal_view_from_camera and rt_resolve_rays_from_camera ask of
// their camera and frame before they compute
inline bool rp_camera_ok(const rt_camera *cam, int width, int height) {
  if (!cam || !post_size_ok(width, height)) return false;
  if (cam->model != RT_CAMERA_CPU && cam->model != RT_CAMERA_GPU) return false;
  return cam->model != RT_CAMERA_CPU || (width >= 2 && height >= 2);
}

}  // namespace rtk

#endif  // RTOW_RT_REPROJECT_H
