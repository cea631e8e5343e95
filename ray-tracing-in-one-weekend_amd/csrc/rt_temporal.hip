// rt_temporal.hip -- temporal accumulation with camera reprojection
// (include/rt_temporal.h, librtow_temporal.so): one small gfx950 kernel, the
// host code that turns an rt_camera into the view the kernel projects with,
// and the pass's host half.
//
// temporal_kernel prepares this frame's guides from the rt_aov sums
// (csrc/rt_post.h, shared with the other image-space passes), projects the
// pixel's mean first-hit position through the previous frame's view, gathers
// the up to four history taps around that point that lie on the same surface,
// blends them with the new colour and writes the next frame's history and the
// caller's sums: one launch, no scratch.  A tap is three 16-byte loads (the
// history's planes).  Those four steps are csrc/rt_reproject.h's, shared with
// rt_resolve.hip: what this file keeps is where the point comes from.
//
// The arithmetic is the header's "Semantics", operation by operation, with
// -ffp-contract=off and the compiler's correctly rounded / and sqrt:
// tests/temporal_ref.py restates it in numpy float32 and gets the same bits.
//
// A library of its own, like librtow_aov.so and
// librtow_denoise.so: the three other code objects stay byte for byte what
// they were.  rt_api.cpp's rt_internal_pass_begin / rt_internal_frame_end
// (csrc/rt_frame.h) keep the pass serialised with the context's other passes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "rt_temporal.h"
#include "rt_frame.h"
#include "rt_reproject.h"

namespace rtk {

constexpr int kTpDefaultMaxLen = 2, kTpMaxMaxLen = 1024;
constexpr float kTpDefaultPlaneTol = 0.0003f, kTpDefaultNormalCos = 0.9f;

struct tp_params {
  rp_params h;
  // the caller's sums
  const float *cur;
  const uint32_t *hits;
  const float *position, *normal;
  float *out;         // may be NULL, may be cur
  const f4 *hist_in;  // three planes; NULL = no history
  f4 *hist_out;
};

// One lane per pixel.  The four taps (rp_gather) are unrolled.  Neighbouring
// lanes reproject to neighbouring history pixels wherever the surface is
// continuous, so a wave's taps fall in a few 256-byte runs of each plane and
// overlap in the vector cache.
__global__ __launch_bounds__(256) void temporal_kernel(const tp_params a) {
  int x, y;
  if (!post_pixel(a.h.width, a.h.height, x, y)) return;
  const size_t npx = (size_t)a.h.width * (size_t)a.h.height;
  const size_t o = (size_t)y * (size_t)a.h.width + (size_t)x;
  // 1. prepare
  const RT_GLOBAL float *g_c = as_global(a.cur) + 3 * o;
  const RT_GLOBAL float *g_p = as_global(a.position) + 3 * o;
  const RT_GLOBAL float *g_n = as_global(a.normal) + 3 * o;
  const uint32_t h = as_global(a.hits)[o];
  const float cr = g_c[0] / a.h.spp_f, cg = g_c[1] / a.h.spp_f, cb = g_c[2] / a.h.spp_f;
  const post_guide g = post_prepare(h, g_p, g_n);
  const bool sky = g.sky;
  const float nx = g.nx, ny = g.ny, nz = g.nz, Px = g.px, Py = g.py, Pz = g.pz;
  // 2. no history
  float mr = cr, mg = cg, mb = cb, len = 1.0f;
  if (a.hist_in && !sky) {
    // 3. reproject
    const float qx = Px - a.h.prev.eye[0], qy = Py - a.h.prev.eye[1], qz = Pz - a.h.prev.eye[2];
    float w, fxp, fyp;
    rp_project(a.h.prev, qx, qy, qz, w, fxp, fyp);
    const rp_taps s = rp_gather(a.h, w, fxp, fyp, g, a.h.pt2 * dot3_unfused(qx, qy, qz, qx, qy, qz), a.hist_in);
    // 5. blend
    if (s.w > 0.0f) {
      rp_blend(s.r / s.w, s.g / s.w, s.b / s.w, s.l / s.w, cr, cg, cb, a.h.max_len_f, mr, mg, mb, len);
    }
  }
  // 6. write
  rp_write(a.hist_out, a.out, npx, o, 3 * o, mr, mg, mb, len, g, a.h.spp_f);
}

}  // namespace rtk

namespace {

// the desc's options with the defaults filled in
struct tp_options {
  int max_len;
  float plane_tol, normal_cos;
};

using rtk::overlap;

// false: an argument is NULL, out of range or NaN, or the buffers overlap
bool resolve(const rt_temporal_desc *d, tp_options &o) {
  if (!rtk::post_size_ok(d->width, d->height)) return false;
  if (d->spp < 1 || d->reserved[0] != 0 || d->reserved[1] != 0) return false;
  if (!d->cur || !d->hits || !d->position || !d->normal || !d->history_out) return false;
  if (!rtk::post_option(d->max_len, rtk::kTpDefaultMaxLen, 1, true, rtk::kTpMaxMaxLen, o.max_len) ||
      !rtk::post_option(d->plane_tol, rtk::kTpDefaultPlaneTol, 0.0f, false, INFINITY, o.plane_tol) ||
      !rtk::post_option(d->normal_cos, rtk::kTpDefaultNormalCos, -1.0f, true, 1.0f, o.normal_cos))
    return false;
  const size_t npx = (size_t)d->width * (size_t)d->height, hb = 48 * npx;
  if (overlap(d->history_out, hb, d->history_in, hb) || overlap(d->history_out, hb, d->cur, 12 * npx) ||
      overlap(d->history_out, hb, d->out, 12 * npx) || overlap(d->history_out, hb, d->hits, 4 * npx) ||
      overlap(d->history_out, hb, d->position, 12 * npx) || overlap(d->history_out, hb, d->normal, 12 * npx) ||
      overlap(d->out, 12 * npx, d->history_in, hb))
    return false;
  return true;
}

// the launch on st; d holds DEVICE pointers
int enqueue(const rt_temporal_desc *d, const tp_options &o, hipStream_t st) {
  rtk::tp_params a;
  std::memset(&a, 0, sizeof a);
  rtk::rp_fill(a.h, d->width, d->height, d->spp, o.max_len, o.plane_tol, o.normal_cos, d->prev);
  a.cur = d->cur;
  a.hits = d->hits;
  a.position = d->position;
  a.normal = d->normal;
  a.out = d->out;
  a.hist_in = static_cast<const rtk::f4 *>(d->history_in);
  a.hist_out = static_cast<rtk::f4 *>(d->history_out);
  rtk::temporal_kernel<<<rtk::post_grid(d->width, d->height), 256, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  return RT_OK;
}

struct d3 {
  double x, y, z;
};
d3 of(const float v[3]) { return {(double)v[0], (double)v[1], (double)v[2]}; }
d3 sub(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
d3 scale(d3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
void put(float out[3], d3 a) {
  out[0] = (float)a.x;
  out[1] = (float)a.y;
  out[2] = (float)a.z;
}

}  // namespace

extern "C" {

int rt_temporal_version(void) { return RT_TEMPORAL_VERSION; }

size_t rt_temporal_history_bytes(int width, int height) {
  if (!rtk::post_size_ok(width, height)) return 0;
  return 48 * (size_t)width * (size_t)height;
}

int rt_temporal_view_from_camera(const rt_camera *cam, int width, int height, rt_temporal_view *out) {
  if (!out || !rtk::rp_camera_ok(cam, width, height)) return RT_ERR_INVALID;
  const d3 eye = of(cam->eye), hz = of(cam->horiz), vt = of(cam->vert);
  const d3 c = sub(of(cam->corner), eye);
  const d3 n = cross(hz, vt);
  const d3 bh = cross(vt, n), bv = cross(n, hz);
  const double cn = dot(c, n), dh = dot(hz, bh), dv = dot(vt, bv);
  if (!(cn != 0.0) || !(dh != 0.0) || !(dv != 0.0)) return RT_ERR_INVALID;  // (NaN too)
  const d3 ah = scale(bh, 1.0 / dh), av = scale(bv, 1.0 / dv);
  // x = sx * fs + ox, y = sy * ft + oy, with fs = (A_h.q)/w - A_h.c
  double sx = 1.0, ox = 0.0, sy = 1.0, oy = 0.0;
  if (cam->model == RT_CAMERA_CPU) {
    sx = (double)(width - 1);
    ox = -0.5;
    sy = -(double)(height - 1);
    oy = (double)height - 0.5;
  }
  rt_temporal_view v;
  put(v.eye, eye);
  put(v.pw, scale(n, 1.0 / cn));
  put(v.px, scale(ah, sx));
  put(v.py, scale(av, sy));
  v.x0 = (float)(sx * dot(ah, c) - ox);
  v.y0 = (float)(sy * dot(av, c) - oy);
  static_assert(sizeof v == 14 * sizeof(float), "rt_temporal_view is fourteen floats");
  float f[14];
  std::memcpy(f, &v, sizeof v);
  for (int i = 0; i < 14; ++i)
    if (!std::isfinite(f[i])) return RT_ERR_INVALID;
  *out = v;
  return RT_OK;
}

int rt_temporal_async(rt_context *c, const rt_temporal_desc *d, void *stream) {
  tp_options o;
  if (!c || !d || !resolve(d, o)) return RT_ERR_INVALID;
  if (!rtk::post_aligned16(d->history_in) || !rtk::post_aligned16(d->history_out)) return RT_ERR_INVALID;
  rt_pass_scope ps(c, nullptr, nullptr, stream);
  return ps.end(ps.status == RT_OK ? enqueue(d, o, ps.fs.stream) : ps.status);
}

int rt_temporal(rt_context *c, const rt_temporal_desc *host, double *kernel_ms) {
  tp_options o;
  if (!c || !host || !resolve(host, o)) return RT_ERR_INVALID;
  const size_t npx = (size_t)host->width * (size_t)host->height;
  // cur / out (blended in place), hits, position, normal, history in (when there is one), history out
  const rt_sync_part parts[6] = {{12 * npx, host->cur, host->out}, {4 * npx, host->hits, nullptr},
                                 {12 * npx, host->position, nullptr}, {12 * npx, host->normal, nullptr},
                                 {host->history_in ? 48 * npx : 0, host->history_in, nullptr},
                                 {48 * npx, nullptr, host->history_out}};
  return rt_sync_pass(c, nullptr, nullptr, parts, kernel_ms, [&](void *const *dev, const rt_frame_setup &fs) {
    rt_temporal_desc d = *host;
    d.cur = static_cast<float *>(dev[0]);
    d.out = host->out ? static_cast<float *>(dev[0]) : nullptr;
    d.hits = static_cast<uint32_t *>(dev[1]);
    d.position = static_cast<float *>(dev[2]);
    d.normal = static_cast<float *>(dev[3]);
    d.history_in = dev[4];
    d.history_out = dev[5];
    return enqueue(&d, o, fs.stream);
  });
}

}  // extern "C"
