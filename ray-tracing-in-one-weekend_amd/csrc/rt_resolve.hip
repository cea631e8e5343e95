// rt_resolve.hip -- clamped temporal resolve with centre reprojection
// (include/rt_resolve.h, librtow_resolve.so): one small gfx950 kernel, the
// host code that turns an rt_camera into the centre rays the kernel places
// its points on, and the pass's host half.
//
// resolve_kernel is temporal_kernel (rt_temporal.hip) with three changes: the
// point it projects through the previous view lies on the pixel centre's ray
// at the mean first-hit depth; a partly covered pixel restarts; and the
// gathered history colour is clamped to the mean +- gamma standard deviations
// of the 3 x 3 neighbourhood of this frame's colour.  Those three are what
// this file holds; the projection, the gather, the blend and the history
// write are the one copy in csrc/rt_reproject.h.  The nine neighbourhood
// reads come from the vector cache: each is a load from a
// CLAMPED pixel coordinate, so it is unconditional and never leaves the frame,
// and a pixel outside the frame is dropped by a select, not by a branch.
//
// The arithmetic is the header's "Semantics", operation by operation, with
// -ffp-contract=off and the compiler's correctly rounded / and sqrt:
// tests/resolve_ref.py restates it in numpy float32 and gets the same bits.
//
// A library of its own, like the three other passes': the four other code
// objects stay byte for byte what they were.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "rt_resolve.h"
#include "rt_frame.h"
#include "rt_reproject.h"

namespace rtk {

constexpr int kRsDefaultMaxLen = 2, kRsMaxMaxLen = 1024;
constexpr float kRsDefaultPlaneTol = 0.003f, kRsDefaultNormalCos = 0.9f, kRsDefaultGamma = 1.0f;

struct rs_params {
  rp_params h;
  uint32_t spp;
  float gamma;
  int clamp;  // 0: the step is left out
  int keep_partial;
  rt_resolve_rays now;
  // the caller's sums
  const float *cur;
  const uint32_t *hits;
  const float *depth, *normal;
  float *out;         // may be NULL; never cur
  const f4 *hist_in;  // three planes; NULL = no history
  f4 *hist_out;
};

// One lane per pixel, as temporal_kernel.  The neighbourhood is read only by
// the lanes that go on to look a history up.
__global__ __launch_bounds__(256) void resolve_kernel(const rs_params a) {
  int x, y;
  if (!post_pixel(a.h.width, a.h.height, x, y)) return;
  const size_t npx = (size_t)a.h.width * (size_t)a.h.height;
  const size_t o = (size_t)y * (size_t)a.h.width + (size_t)x;
  // 1. prepare
  const RT_GLOBAL float *g_cur = as_global(a.cur);
  const RT_GLOBAL float *g_c = g_cur + 3 * o;
  const RT_GLOBAL float *g_n = as_global(a.normal) + 3 * o;
  const uint32_t h = as_global(a.hits)[o];
  const float cr = g_c[0] / a.h.spp_f, cg = g_c[1] / a.h.spp_f, cb = g_c[2] / a.h.spp_f;
  post_guide g = post_prepare(h, g_n, g_n);  // its normal half: the position half is compiled away, and set below
  const float tm = as_global(a.depth)[o] / (float)h;
  float D[3];
  rp_centre_ray(a.now, x, y, D);
  const float dl = __builtin_sqrtf(dot3_unfused(D[0], D[1], D[2], D[0], D[1], D[2]));
  g.px = g.sky ? 0.0f : a.now.eye[0] + (D[0] / dl) * tm;
  g.py = g.sky ? 0.0f : a.now.eye[1] + (D[1] / dl) * tm;
  g.pz = g.sky ? 0.0f : a.now.eye[2] + (D[2] / dl) * tm;
  // 3. no history
  float mr = cr, mg = cg, mb = cb, len = 1.0f;
  if (a.hist_in && !g.sky && (a.keep_partial || h >= a.spp)) {
    // 2. neighbourhood: unconditional loads from clamped coordinates, selects
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
    if (a.clamp) {
      float m1[3] = {0.0f, 0.0f, 0.0f}, m2[3] = {0.0f, 0.0f, 0.0f}, k = 0.0f;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const int ty = y + dy;
        const bool iny = ty >= 0 && ty < a.h.height;
        const size_t row = (size_t)(iny ? ty : y) * (size_t)a.h.width;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int tx = x + dx;
          const bool in = iny && tx >= 0 && tx < a.h.width;
          const RT_GLOBAL float *q = g_cur + 3 * (row + (size_t)(in ? tx : x));
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float cq = q[ch] / a.h.spp_f;
            m1[ch] = in ? m1[ch] + cq : m1[ch];
            m2[ch] = in ? m2[ch] + cq * cq : m2[ch];
          }
          k = in ? k + 1.0f : k;
        }
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float mu = m1[ch] / k;
        float v = m2[ch] / k - mu * mu;
        v = v > 0.0f ? v : 0.0f;
        const float sd = __builtin_sqrtf(v);
        lo[ch] = mu - a.gamma * sd;
        hi[ch] = mu + a.gamma * sd;
      }
    }
    // 4. reproject and gather (rt_temporal.h, steps 3 and 4)
    const float qx = g.px - a.h.prev.eye[0], qy = g.py - a.h.prev.eye[1], qz = g.pz - a.h.prev.eye[2];
    float w, fxp, fyp;
    rp_project(a.h.prev, qx, qy, qz, w, fxp, fyp);
    const rp_taps s = rp_gather(a.h, w, fxp, fyp, g, a.h.pt2 * dot3_unfused(qx, qy, qz, qx, qy, qz), a.hist_in);
    // 5. clamp and blend
    if (s.w > 0.0f) {
      float hr = s.r / s.w, hg = s.g / s.w, hb = s.b / s.w;
      if (a.clamp) {
        hr = hr < lo[0] ? lo[0] : (hr > hi[0] ? hi[0] : hr);
        hg = hg < lo[1] ? lo[1] : (hg > hi[1] ? hi[1] : hg);
        hb = hb < lo[2] ? lo[2] : (hb > hi[2] ? hi[2] : hb);
      }
      rp_blend(hr, hg, hb, s.l / s.w, cr, cg, cb, a.h.max_len_f, mr, mg, mb, len);
    }
  }
  // 6. write
  rp_write(a.hist_out, a.out, npx, o, 3 * o, mr, mg, mb, len, g, a.h.spp_f);
}

}  // namespace rtk

namespace {

// the desc's options with the defaults filled in
struct rs_options {
  int max_len;
  float plane_tol, normal_cos, gamma;
};

using rtk::overlap;

// false: an argument is NULL, out of range or NaN, or the buffers overlap.
// same_ok: out == cur is allowed (the synchronous wrapper stages out apart)
bool resolve(const rt_resolve_desc *d, rs_options &o, bool same_ok) {
  if (!rtk::post_size_ok(d->width, d->height)) return false;
  if (d->spp < 1 || d->reserved != 0 || (d->flags & ~RT_RESOLVE_KEEP_PARTIAL) != 0) return false;
  if (!d->cur || !d->hits || !d->depth || !d->normal || !d->history_out) return false;
  if (!rtk::post_option(d->max_len, rtk::kRsDefaultMaxLen, 1, true, rtk::kRsMaxMaxLen, o.max_len) ||
      !rtk::post_option(d->plane_tol, rtk::kRsDefaultPlaneTol, 0.0f, false, INFINITY, o.plane_tol) ||
      !rtk::post_option(d->normal_cos, rtk::kRsDefaultNormalCos, -1.0f, true, 1.0f, o.normal_cos) ||
      !rtk::post_option(d->gamma, rtk::kRsDefaultGamma, 0.0f, false, INFINITY, o.gamma))
    return false;
  const size_t npx = (size_t)d->width * (size_t)d->height, hb = 48 * npx;
  if (overlap(d->history_out, hb, d->history_in, hb) || overlap(d->history_out, hb, d->cur, 12 * npx) ||
      overlap(d->history_out, hb, d->out, 12 * npx) || overlap(d->history_out, hb, d->hits, 4 * npx) ||
      overlap(d->history_out, hb, d->depth, 4 * npx) || overlap(d->history_out, hb, d->normal, 12 * npx) ||
      overlap(d->out, 12 * npx, d->history_in, hb))
    return false;
  if (overlap(d->out, 12 * npx, d->cur, 12 * npx) && !(same_ok && d->out == d->cur)) return false;
  return true;
}

// the launch on st; d holds DEVICE pointers
int enqueue(const rt_resolve_desc *d, const rs_options &o, hipStream_t st) {
  rtk::rs_params a;
  std::memset(&a, 0, sizeof a);
  rtk::rp_fill(a.h, d->width, d->height, d->spp, o.max_len, o.plane_tol, o.normal_cos, d->prev);
  a.spp = (uint32_t)d->spp;
  a.gamma = o.gamma;
  a.clamp = !std::isinf(o.gamma);
  a.keep_partial = (d->flags & RT_RESOLVE_KEEP_PARTIAL) != 0;
  a.now = d->now;
  a.cur = d->cur;
  a.hits = d->hits;
  a.depth = d->depth;
  a.normal = d->normal;
  a.out = d->out;
  a.hist_in = static_cast<const rtk::f4 *>(d->history_in);
  a.hist_out = static_cast<rtk::f4 *>(d->history_out);
  rtk::resolve_kernel<<<rtk::post_grid(d->width, d->height), 256, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_resolve_version(void) { return RT_RESOLVE_VERSION; }

int rt_resolve_rays_from_camera(const rt_camera *cam, int width, int height, rt_resolve_rays *out) {
  if (!out || !rtk::rp_camera_ok(cam, width, height)) return RT_ERR_INVALID;
  // D = c + a0 horiz + b0 vert + i (sa horiz) + j (sb vert)
  double a0 = 0.0, b0 = 0.0, sa = 1.0, sb = 1.0;
  if (cam->model == RT_CAMERA_CPU) {
    a0 = 0.5 / (double)(width - 1);
    b0 = ((double)height - 0.5) / (double)(height - 1);
    sa = 1.0 / (double)(width - 1);
    sb = -1.0 / (double)(height - 1);
  }
  rt_resolve_rays r;
  for (int k = 0; k < 3; ++k) {
    const double e = cam->eye[k], hz = cam->horiz[k], vt = cam->vert[k];
    r.eye[k] = cam->eye[k];
    r.d00[k] = (float)(((double)cam->corner[k] - e) + a0 * hz + b0 * vt);
    r.du[k] = (float)(sa * hz);
    r.dv[k] = (float)(sb * vt);
  }
  static_assert(sizeof r == 12 * sizeof(float), "rt_resolve_rays is twelve floats");
  float f[12];
  std::memcpy(f, &r, sizeof r);
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(f[i])) return RT_ERR_INVALID;
  *out = r;
  return RT_OK;
}

int rt_resolve_async(rt_context *c, const rt_resolve_desc *d, void *stream) {
  rs_options o;
  if (!c || !d || !resolve(d, o, false)) return RT_ERR_INVALID;
  if (!rtk::post_aligned16(d->history_in) || !rtk::post_aligned16(d->history_out)) return RT_ERR_INVALID;
  rt_pass_scope ps(c, nullptr, nullptr, stream);
  return ps.end(ps.status == RT_OK ? enqueue(d, o, ps.fs.stream) : ps.status);
}

int rt_resolve(rt_context *c, const rt_resolve_desc *host, double *kernel_ms) {
  rs_options o;
  if (!c || !host || !resolve(host, o, true)) return RT_ERR_INVALID;
  const size_t npx = (size_t)host->width * (size_t)host->height;
  // cur, hits, depth, normal, history in (when there is one), history out, out (apart from cur: "In place")
  const rt_sync_part parts[7] = {{12 * npx, host->cur, nullptr}, {4 * npx, host->hits, nullptr},
                                 {4 * npx, host->depth, nullptr}, {12 * npx, host->normal, nullptr},
                                 {host->history_in ? 48 * npx : 0, host->history_in, nullptr},
                                 {48 * npx, nullptr, host->history_out},
                                 {host->out ? 12 * npx : 0, nullptr, host->out}};
  return rt_sync_pass(c, nullptr, nullptr, parts, kernel_ms, [&](void *const *dev, const rt_frame_setup &fs) {
    rt_resolve_desc d = *host;
    d.cur = static_cast<float *>(dev[0]);
    d.hits = static_cast<uint32_t *>(dev[1]);
    d.depth = static_cast<float *>(dev[2]);
    d.normal = static_cast<float *>(dev[3]);
    d.history_in = dev[4];
    d.history_out = dev[5];
    d.out = static_cast<float *>(dev[6]);
    return enqueue(&d, o, fs.stream);
  });
}

}  // extern "C"
