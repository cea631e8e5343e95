// rt_temporal.hip -- temporal accumulation with camera reprojection
// (include/rt_temporal.h, librtow_temporal.so): one small gfx950 kernel, the
// host code that turns an rt_camera into the view the kernel projects with,
// and the pass's host half.
//
// temporal_kernel prepares this frame's guides from the rt_aov sums
// (csrc/rt_post.h, shared with rt_denoise.hip), projects the pixel's mean first-hit
// position through the previous frame's view, gathers the up to four history
// taps around that point that lie on the same surface, blends them with the
// new colour and writes the next frame's history and the caller's sums: one
// launch, no scratch.  A tap is three 16-byte loads (the history's planes).
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
#include "rt_post.h"

namespace rtk {

constexpr int kTpDefaultMaxLen = 2, kTpMaxMaxLen = 1024;
constexpr float kTpDefaultPlaneTol = 0.0003f, kTpDefaultNormalCos = 0.9f;

struct tp_params {
  int width, height;
  float width_f, height_f;
  float spp_f;
  float max_len_f;
  float pt2;         // plane_tol^2
  float normal_cos;
  int plane_test, normal_test;  // 0: the test is left out
  rt_temporal_view prev;
  // the caller's sums
  const float *cur;
  const uint32_t *hits;
  const float *position, *normal;
  float *out;         // may be NULL, may be cur
  const f4 *hist_in;  // three planes; NULL = no history
  f4 *hist_out;
};

// One lane per pixel.  The four taps are unrolled; a tap outside the frame, on
// sky or on another surface is skipped per lane (its loads are predicated, so
// no lane reads outside the planes).  Neighbouring lanes reproject to
// neighbouring history pixels wherever the surface is continuous, so a wave's
// taps fall in a few 256-byte runs of each plane and overlap in the vector
// cache.
__global__ __launch_bounds__(256) void temporal_kernel(const tp_params a) {
  int x, y;
  if (!post_pixel(a.width, a.height, x, y)) return;
  const size_t npx = (size_t)a.width * (size_t)a.height;
  const size_t o = (size_t)y * (size_t)a.width + (size_t)x;
  // 1. prepare
  const RT_GLOBAL float *g_c = as_global(a.cur) + 3 * o;
  const RT_GLOBAL float *g_p = as_global(a.position) + 3 * o;
  const RT_GLOBAL float *g_n = as_global(a.normal) + 3 * o;
  const uint32_t h = as_global(a.hits)[o];
  const float cr = g_c[0] / a.spp_f, cg = g_c[1] / a.spp_f, cb = g_c[2] / a.spp_f;
  const post_guide g = post_prepare(h, g_p, g_n);
  const bool sky = g.sky;
  const float nx = g.nx, ny = g.ny, nz = g.nz, Px = g.px, Py = g.py, Pz = g.pz;
  // 2. no history
  float mr = cr, mg = cg, mb = cb, len = 1.0f;
  if (a.hist_in && !sky) {
    // 3. reproject
    const float qx = Px - a.prev.eye[0], qy = Py - a.prev.eye[1], qz = Pz - a.prev.eye[2];
    const float w = dot3_unfused(a.prev.pw[0], a.prev.pw[1], a.prev.pw[2], qx, qy, qz);
    const float fxp = dot3_unfused(a.prev.px[0], a.prev.px[1], a.prev.px[2], qx, qy, qz) / w - a.prev.x0;
    const float fyp = dot3_unfused(a.prev.py[0], a.prev.py[1], a.prev.py[2], qx, qy, qz) / w - a.prev.y0;
    const bool ok = w > 0.0f && fxp > -1.0f && fxp < a.width_f && fyp > -1.0f && fyp < a.height_f;
    if (ok) {
      const float xf = __builtin_floorf(fxp), yf = __builtin_floorf(fyp);
      const float fx = fxp - xf, fy = fyp - yf;
      const int xi = (int)xf, yi = (int)yf;  // -1 .. W-1, -1 .. H-1
      const float d2 = dot3_unfused(qx, qy, qz, qx, qy, qz);
      const float lim = a.pt2 * d2;
      const RT_GLOBAL f4 *__restrict__ h0 = as_global(a.hist_in);
      const RT_GLOBAL f4 *__restrict__ h1 = h0 + npx;
      const RT_GLOBAL f4 *__restrict__ h2 = h1 + npx;
      // 4. gather
      float sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f, sw = 0.0f;
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
          const float e = dot3_unfused(nx, ny, nz, pt.x - Px, pt.y - Py, pt.z - Pz);
          if (a.plane_test && !(e * e <= lim)) continue;
          const float g = dot3_unfused(nx, ny, nz, nt.x, nt.y, nt.z);
          if (a.normal_test && !(g >= a.normal_cos)) continue;
          const f4 ct = h0[t];
          const float b = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy);
          sw += b;
          sr += b * ct.x;
          sg += b * ct.y;
          sb += b * ct.z;
          sl += b * ct.w;
        }
      }
      // 5. blend
      if (sw > 0.0f) {
        const float hr = sr / sw, hg = sg / sw, hb = sb / sw, hl = sl / sw;
        const float t = hl + 1.0f;
        len = t < a.max_len_f ? t : a.max_len_f;
        const float al = 1.0f / len;
        mr = hr + (cr - hr) * al;
        mg = hg + (cg - hg) * al;
        mb = hb + (cb - hb) * al;
      }
    }
  }
  // 6. write
  RT_GLOBAL f4 *o0 = as_global(a.hist_out);
  f4 v;
  v.x = mr;
  v.y = mg;
  v.z = mb;
  v.w = len;
  o0[o] = v;
  v.x = Px;
  v.y = Py;
  v.z = Pz;
  v.w = sky ? 1.0f : 0.0f;
  o0[npx + o] = v;
  v.x = nx;
  v.y = ny;
  v.z = nz;
  v.w = 0.0f;
  o0[2 * npx + o] = v;
  if (a.out) {
    RT_GLOBAL float *out = as_global(a.out) + 3 * o;
    out[0] = mr * a.spp_f;
    out[1] = mg * a.spp_f;
    out[2] = mb * a.spp_f;
  }
}

}  // namespace rtk

namespace {

// the desc's options with the defaults filled in
struct tp_options {
  int max_len;
  float plane_tol, normal_cos;
};

bool overlap(const void *p, size_t np, const void *q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + nq && b < a + np;
}

// false: an argument is NULL, out of range or NaN, or the buffers overlap
bool resolve(const rt_temporal_desc *d, tp_options &o) {
  if (!rtk::post_size_ok(d->width, d->height)) return false;
  if (d->spp < 1 || d->reserved[0] != 0 || d->reserved[1] != 0) return false;
  if (!d->cur || !d->hits || !d->position || !d->normal || !d->history_out) return false;
  o.max_len = d->max_len == 0 ? rtk::kTpDefaultMaxLen : d->max_len;
  if (o.max_len < 1 || o.max_len > rtk::kTpMaxMaxLen) return false;
  o.plane_tol = d->plane_tol == 0.0f ? rtk::kTpDefaultPlaneTol : d->plane_tol;
  if (!(o.plane_tol > 0.0f)) return false;  // (NaN too)
  o.normal_cos = d->normal_cos == 0.0f ? rtk::kTpDefaultNormalCos : d->normal_cos;
  if (!(o.normal_cos >= -1.0f && o.normal_cos <= 1.0f)) return false;
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
  a.width = d->width;
  a.height = d->height;
  a.width_f = (float)d->width;
  a.height_f = (float)d->height;
  a.spp_f = (float)d->spp;
  a.max_len_f = (float)o.max_len;
  a.pt2 = o.plane_tol * o.plane_tol;
  a.normal_cos = o.normal_cos;
  a.plane_test = !std::isinf(o.plane_tol);
  a.normal_test = o.normal_cos != -1.0f;
  a.prev = d->prev;
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
  if (!cam || !out || !rtk::post_size_ok(width, height)) return RT_ERR_INVALID;
  if (cam->model != RT_CAMERA_CPU && cam->model != RT_CAMERA_GPU) return RT_ERR_INVALID;
  if (cam->model == RT_CAMERA_CPU && (width < 2 || height < 2)) return RT_ERR_INVALID;
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
  if (((uintptr_t)d->history_in & 15) || ((uintptr_t)d->history_out & 15)) return RT_ERR_INVALID;
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
