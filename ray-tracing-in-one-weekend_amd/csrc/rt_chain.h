// rt_chain.h -- internal, device only: one sample's specular chain, shared by
// the two passes that follow the render's path through glass and smooth metal
// (guides_kernel in rt_guides.hip, route_kernel in rt_route.hip; each includes
// this once, nothing else does).  It is the single restatement of
// render_kernel's (rt_kernel.hip) segment loop beyond the first hit: both arms
// of the spurious-root rule and the metal and dielectric blocks, line by line,
// on the helpers of rt_device.h and the hit block of rt_trace_pass.h.  The
// render kernel does not include this header; it is inlined into kernels
// compiled with the render kernel's flags.
#ifndef RTOW_RT_CHAIN_H
#define RTOW_RT_CHAIN_H

#include "rt_trace_pass.h"

namespace rtk {

// What a chain-following pass adds to its kparams: how far a chain goes.
struct chain_limits {
  int max_bounces;  // resolved: 0 = follow nothing
  float max_fuzz;
};

// Sample s of pixel px (pix: its index in the whole frame): the camera ray and
// the chain behind it, to the terminal.  Per sample the wave runs one loop over
// segments: closest_hit<> is wave-uniform, so the wave repeats it while any
// lane's chain is alive; a lane whose chain has ended sits the remaining walks
// out under the exec mask (it does not walk again, and it does not leave the
// loop).  Every lane of the wave calls this, lanes on padding rows included
// (they trace nothing).  A hit sample -- its primary ray hit something -- ends
// with
//   terminal(sphere, depth, px, py, pz, nx, ny, nz, thr, thg, thb, bounces, escaped)
// the terminal sphere, the length walked to it, its P and shading N, the
// throughput after it, the bounces followed and whether the chain left the
// scene; a miss calls nothing.  metal_unit: RT_FLAG_METAL_UNIT_VECTOR, read by
// the caller once (wave-uniform).
template <bool OPEN, bool BVH, bool GRID, int GP, class Terminal>
__device__ __forceinline__ void trace_chain(const kparams &p, const trace_pixel &px, uint32_t pix, int s,
                                            bool metal_unit, const chain_limits &lim, work_ctr &wc,
                                            Terminal terminal) {
  float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 1.f, dz = 0.f;
  float tmin = 0.001f;
  if (px.inside)
    tmin = camera_ray(p, pcg4d(pix, (uint32_t)s, 0u, p.seed32), px.col, px.grow, ox, oy, oz, dx, dy, dz);
  float thr = 1.f, thg = 1.f, thb = 1.f;
  int depth = 0;            // counted hits so far: the next hit draws pcg4d(pix, s, depth + 1)
  int origin_sphere = -1;   // the sphere the ray starts on (-1: a camera ray); after the loop, the terminal
  int nb = 0;               // bounces followed
  float walked = 0.0f;      // this segment: distance to the current origin (spurious roots that moved it)
  float total = 0.0f;       // length walked to the last counted hit
  float lpx = 0.f, lpy = 0.f, lpz = 0.f, lnx = 0.f, lny = 0.f, lnz = 0.f;  // the last counted hit's P, N
  bool escaped = false;
  bool alive = px.inside;  // lanes on padding rows trace nothing
  // one wave-level loop over segments: it repeats while any lane is alive
  while (__builtin_amdgcn_ballot_w64(alive)) {
    hit_state hs = no_hit();
    if (alive) hs = walk<OPEN, BVH, GRID, GP>(p, ox, oy, oz, dx, dy, dz, tmin, wc);
    if (alive) {
      const int best = best_of<OPEN>(hs);
      bool skipped = false;
      if (best < 0) {
        // the chain left the scene: the terminal is the last surface it hit
        escaped = origin_sphere >= 0;
        alive = false;
      } else {
        // render_kernel's hit block
        shade_rec sr;
        float tmax, t, b;
        const bool near = hit_root(p, hs, best, ox, oy, oz, dx, dy, dz, sr, tmax, t, b);
        if (b > 0.0f && (t < tmin || (best == origin_sphere && !near))) {
          // a spurious root, either arm: not a segment, not a bounce
          if (t < tmin) {
            ox = fmaf(tmax, dx, ox);
            oy = fmaf(tmax, dy, oy);
            oz = fmaf(tmax, dz, oz);
            walked += tmax;
          } else {
            tmin = __uint_as_float(__float_as_uint(tmax) + 1u);  // nextafter(tmax, +inf), tmax > 0 finite
          }
          skipped = true;
        } else {
          float hx, hy, hz, nx, ny, nz;
          const bool front = hit_surface(sr, near, t, ox, oy, oz, dx, dy, dz, hx, hy, hz, nx, ny, nz);
          const uint32_t kind = sr.kind;
          float sx = 0.f, sy = 0.f, sz = 0.f;
          bool cont = false;
          if (kind != RT_LAMBERTIAN) {  // (a lambertian is a terminal: its scatter is not needed)
            const uint4 r = pcg4d(pix, (uint32_t)s, (uint32_t)(depth + 1), p.seed32);
            const float dn = dot3(dx, dy, dz, nx, ny, nz);
            float rx, ry, rz;
            reflect3(dx, dy, dz, nx, ny, nz, dn, rx, ry, rz);
            sx = rx;
            sy = ry;
            sz = rz;
            if (kind == RT_METAL) {
              // material.h:40-46, with the step's unit vector (z = 1 - 2 u1)
              const float uz = fmaf(-2.0f, unif(r.x), 1.0f);
              float ux, uy;
              polar(fmaf(-uz, uz, 1.0f), unif(r.y), ux, uy);
              float fz = sr.param;
              if (!metal_unit) fz *= ball_radius(r);  // random_in_unit_sphere
              sx = fmaf(fz, ux, rx);
              sy = fmaf(fz, uy, ry);
              sz = fmaf(fz, uz, rz);
              const bool scattered = dot3(sx, sy, sz, nx, ny, nz) > 0.0f;
              cont = scattered && sr.param <= lim.max_fuzz;
            }
            if (kind >= RT_DIELECTRIC) {
              // dielectric, material.h:57-87 (r0 is the same for ior and 1/ior)
              const float ratio = front ? sr.inv_param : sr.param;
              const float cos_t = fminf(-dn, 1.0f);
              const bool cannot = (ratio * ratio) * fmaf(-cos_t, cos_t, 1.0f) > 1.0f;
              if (!(cannot || schlick(cos_t, sr.r0) > unif(r.x))) refract3(dx, dy, dz, nx, ny, nz, cos_t, ratio, sx, sy, sz);
              cont = true;
            }
          }
          // attenuation = albedo (dielectrics store 1,1,1: the product is
          // exact), held finite as the render's wide build holds it
          thr = fminf(thr * sr.ar, 0x1p100f);
          thg = fminf(thg * sr.ag, 0x1p100f);
          thb = fminf(thb * sr.ab, 0x1p100f);
          ++depth;
          total += walked + t;
          walked = 0.0f;
          lpx = hx;
          lpy = hy;
          lpz = hz;
          lnx = nx;
          lny = ny;
          lnz = nz;
          origin_sphere = best;
          if (cont && nb < lim.max_bounces) {
            ++nb;
            ox = hx;
            oy = hy;
            oz = hz;
            dx = sx;  // normalised below
            dy = sy;
            dz = sz;
          } else {
            alive = false;  // the terminal
          }
        }
      }
      // the render's one normalize3 per step: the bounce direction's, and a
      // skipped ray's again (it keeps its own t_min)
      if (alive) {
        const float tmin_new = normalize3(dx, dy, dz);
        tmin = skipped ? tmin : tmin_new;
      }
    }
  }
  if (origin_sphere >= 0) terminal(origin_sphere, total, lpx, lpy, lpz, lnx, lny, lnz, thr, thg, thb, nb, escaped);
}

}  // namespace rtk

#endif  // RTOW_RT_CHAIN_H
