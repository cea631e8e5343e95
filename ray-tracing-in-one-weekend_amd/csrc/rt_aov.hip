// rt_aov.hip -- the first-hit feature pass (include/rt_aov.h, librtow_aov.so):
// a second, small gfx950 kernel that traces the render's primary rays, stops
// at the first hit and writes what it found (coverage, id, depth, position,
// shading normal, albedo), and its host half.
//
// It is the render's first segment, by construction: the primary ray
// (pcg4d(pix, sample, 0, seed32), camera_ray), closest_hit<> with the scan /
// BVH / layer-grid walks and refine_root are the render kernel's own code
// (csrc/rt_device.h), compiled with the same flags.  The grid staging, the
// pixel mapping, the hit block's two halves, the six sums and the host's
// launch sequence are csrc/rt_trace_pass.h's, shared with rt_guides.hip; what
// this file still restates of render_kernel (rt_kernel.hip) is a camera ray's
// arm of the spurious-root rule.
//
// A library of its own: librtow.so's device code stays byte for
// byte what the committed PMC summaries were collected on.  The context stays
// opaque here; rt_api.cpp's rt_internal_frame_begin / _end (csrc/rt_frame.h)
// give the pass the scene's kernel arguments and keep it serialised with the
// context's renders.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_aov.h"
#include "rt_trace_pass.h"

namespace rtk {

struct aov_params {
  kparams k;  // s_lo / s_cnt: this launch's samples of every pixel; out, units, sums: unused
  feature_ptrs f;
};
static_assert(offsetof(aov_params, k) == 0, "kernargs() reads a kparams at offset 0");

// rt_trace_pass.h's mapping and sums; per sample one segment, the camera
// ray's.  Lanes outside the frame's tiles leave before the first walk.  No
// static LDS: every grid placement the context chose for the render
// (kGridLdsMax next to render_kernel's kStaticLds) fits here too.
template <bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void aov_kernel(const aov_params a) {
  const kparams &p = a.k;
  stage_grid<GP>(p);
  trace_pixel px;
  if (!trace_pixel_of(p, px)) return;
  const bool first = p.s_lo == 0;
  feature_sums sums;
  sums.load(a.f, px.o, first);
  if (px.inside) {
    const uint32_t pix = (uint32_t)px.grow * (uint32_t)p.width + (uint32_t)px.col;
    work_ctr wc;
    for (int s = p.s_lo; s < p.s_lo + p.s_cnt; ++s) {
      float ox, oy, oz, dx, dy, dz;
      const float tmin = camera_ray(p, pcg4d(pix, (uint32_t)s, 0u, p.seed32), px.col, px.grow, ox, oy, oz, dx, dy, dz);
      float walked = 0.0f;  // distance to the current origin (0 unless a spurious root moved it)
      while (true) {
        const hit_state hs = walk<OPEN, BVH, GRID, GP>(p, ox, oy, oz, dx, dy, dz, tmin, wc);
        const int best = best_of<OPEN>(hs);
        if (best < 0) break;  // a miss adds nothing
        // render_kernel's hit block for a camera ray (origin_sphere = -1)
        shade_rec sr;
        float tmax, t, b;
        const bool near = hit_root(p, hs, best, ox, oy, oz, dx, dy, dz, sr, tmax, t, b);
        if (b > 0.0f && t < tmin) {
          // a spurious root: the same ray from the scan's root point, same
          // t_min; not a segment
          ox = fmaf(tmax, dx, ox);
          oy = fmaf(tmax, dy, oy);
          oz = fmaf(tmax, dz, oz);
          walked += tmax;
          continue;
        }
        float hx, hy, hz, nx, ny, nz;
        (void)hit_surface(sr, near, t, ox, oy, oz, dx, dy, dz, hx, hy, hz, nx, ny, nz);
        sums.add(best, s, walked + t, hx, hy, hz, nx, ny, nz, sr.ar, sr.ag, sr.ab);
        break;
      }
    }
  }
  sums.store(a.f, px.o, first);
}

}  // namespace rtk

namespace {

template <bool O, bool B, bool G, int P>
struct aov_variant {
  static constexpr auto kernel = &rtk::aov_kernel<O, B, G, P>;
};

int aov_enqueue(const rt_frame_setup &fs, const rt_params *prm, void *const *dev, std::vector<hipEvent_t> *events) {
  rtk::aov_params ap;
  std::memset(&ap, 0, sizeof ap);
  ap.k = fs.kp;
  ap.f = rtk::feature_ptrs_of(dev);
  return trace_launches(fs, prm, events, [&](int s_lo, int s_cnt) {
    ap.k.s_lo = s_lo;
    ap.k.s_cnt = s_cnt;
    launch_frame<aov_variant>(fs, prm, ap);
  });
}

// rt_aov (host arrays) or rt_aov_async (device pointers) after the argument checks
int aov_pass(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_aov_buffers *b, void *stream,
             bool host, double *kernel_ms) {
  void *const bufs[6] = {b->hits, b->id, b->depth, b->position, b->normal, b->albedo};
  static constexpr uint8_t px_bytes[6] = {4, 4, 4, 12, 12, 12};
  return trace_pass(c, cam, prm, bufs, px_bytes, aov_enqueue, stream, host, kernel_ms);
}

}  // namespace

extern "C" {

int rt_aov_version(void) { return RT_AOV_VERSION; }

int rt_aov_async(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_aov_buffers *dev,
                 void *stream) {
  if (!c || !cam || !prm || !dev) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  return aov_pass(c, cam, prm, dev, stream, false, nullptr);
}

int rt_aov(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_aov_buffers *host,
           double *kernel_ms) {
  if (!c || !cam || !prm || !host) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  return aov_pass(c, cam, prm, host, nullptr, true, kernel_ms);
}

}  // extern "C"
