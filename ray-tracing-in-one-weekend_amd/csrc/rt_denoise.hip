// rt_denoise.hip -- the guided a-trous denoiser (include/rt_denoise.h,
// librtow_denoise.so): two small gfx950 kernels and their host half.
//
// prepare_kernel turns the five input sums into what the iterations read: two
// float4 of guides per pixel (unit normal + sky flag, mean position + pad) and
// the albedo-demodulated colour, rgb padded to a float4, in colour plane 0: a
// tap is three 16-byte loads.  atrous_kernel runs one iteration of the 5x5
// stencil at step 2^i from one colour plane into the other; the last iteration
// multiplies the albedo back in and writes the caller's buffer instead.
//
// The arithmetic is the header's "Semantics", operation by operation, with
// -ffp-contract=off and the compiler's correctly rounded / and sqrt:
// tests/denoise_ref.py restates it in numpy float32 and gets the same bits.
//
// A library of its own, like librtow_aov.so: librtow.so's
// device code stays byte for byte what the committed PMC summaries were
// collected on.  rt_api.cpp's rt_internal_pass_begin / rt_internal_frame_end
// (csrc/rt_frame.h) keep the filter serialised with the context's renders;
// what it shares with rt_temporal.hip on the device is csrc/rt_post.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "rt_denoise.h"
#include "rt_frame.h"
#include "rt_post.h"

namespace rtk {

constexpr float kDnDefaultSigmaPlane = 0.5f, kDnDefaultSigmaColor = 0.15f;
constexpr int kDnDefaultIterations = 5, kDnDefaultNormalPower = 6;

struct dn_params {
  int width, height;
  int spp;
  float spp_f;
  // the caller's sums
  const float *beauty;
  const uint32_t *hits;
  const float *position, *normal, *albedo;
  float *out;
  // scratch
  f4 *guide_n;  // unit normal, w = 1 for a sky pixel
  f4 *guide_p;  // mean position, w = 0
  const f4 *src;  // the iteration's colour plane (prepare: unused)
  f4 *dst;        // prepare: plane 0; an iteration but the last: the other plane
  // the iteration
  int step;
  int normal_power;
  float sigma_plane;
  float sigma2;  // (sigma_color * 2^-i)^2; 0 = the colour term is off
};

// max(a_c, 1e-3f) of the header: the albedo the colour is divided by before
// the filter and multiplied by after it
__device__ __forceinline__ float demod(float albedo_sum, uint32_t h, int spp, float spp_f) {
  const float a = (albedo_sum + (float)(spp - (int)h)) / spp_f;
  return a > 1e-3f ? a : 1e-3f;
}

__global__ __launch_bounds__(256) void prepare_kernel(const dn_params a) {
  const size_t o = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (o >= (size_t)a.width * (size_t)a.height) return;
  const RT_GLOBAL float *g_b = as_global(a.beauty) + 3 * o;
  const RT_GLOBAL float *g_p = as_global(a.position) + 3 * o;
  const RT_GLOBAL float *g_n = as_global(a.normal) + 3 * o;
  const RT_GLOBAL float *g_a = as_global(a.albedo) + 3 * o;
  const uint32_t h = as_global(a.hits)[o];
  const post_guide g = post_prepare(h, g_p, g_n);
  f4 u, n, p;
  u.x = (g_b[0] / a.spp_f) / demod(g_a[0], h, a.spp, a.spp_f);
  u.y = (g_b[1] / a.spp_f) / demod(g_a[1], h, a.spp, a.spp_f);
  u.z = (g_b[2] / a.spp_f) / demod(g_a[2], h, a.spp, a.spp_f);
  u.w = 0.0f;
  n.x = g.nx;
  n.y = g.ny;
  n.z = g.nz;
  n.w = g.sky ? 1.0f : 0.0f;
  p.x = g.px;
  p.y = g.py;
  p.z = g.pz;
  p.w = 0.0f;
  as_global(a.guide_n)[o] = n;
  as_global(a.guide_p)[o] = p;
  as_global(a.dst)[o] = u;
}

// One lane per pixel; the 25 taps are unrolled, so k[dx] * k[dy] and the
// centre tap's shortcut are compile-time.  Taps outside the frame are skipped
// per lane; the loads of the others go through the vector cache, where the
// taps of a wave's 16 x 4 pixels overlap (steps 1 and 2) or fall in the same
// 256-byte runs (every step).
template <bool LAST>
__global__ __launch_bounds__(256) void atrous_kernel(const dn_params a) {
  int x, y;
  if (!post_pixel(a.width, a.height, x, y)) return;
  const size_t o = (size_t)y * (size_t)a.width + (size_t)x;
  const RT_GLOBAL f4 *__restrict__ gn = as_global(a.guide_n);
  const RT_GLOBAL f4 *__restrict__ gp = as_global(a.guide_p);
  const RT_GLOBAL f4 *__restrict__ src = as_global(a.src);
  const f4 np = gn[o], pp = gp[o], up = src[o];
  const bool sky_p = np.w != 0.0f;
  const bool colour = a.sigma2 != 0.0f;
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + dy * a.step;
    if (qy < 0 || qy >= a.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + dx * a.step;
      if (qx < 0 || qx >= a.width) continue;
      constexpr float k[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};
      const float kk = k[dx + 2] * k[dy + 2];
      if (dx == 0 && dy == 0) {
        sr += kk * up.x;
        sg += kk * up.y;
        sb += kk * up.z;
        sw += kk;
        continue;
      }
      const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
      const f4 nq = gn[q], pq = gp[q], uq = src[q];
      const bool sky_q = nq.w != 0.0f;
      // w_n
      float wn = dot3_unfused(np.x, np.y, np.z, nq.x, nq.y, nq.z);
      wn = wn > 0.0f ? wn : 0.0f;
      for (int i = 0; i < a.normal_power; ++i) wn = wn * wn;
      wn = sky_p != sky_q ? 0.0f : wn;
      wn = sky_p && sky_q ? 1.0f : wn;
      // w_p
      const float ex = pq.x - pp.x, ey = pq.y - pp.y, ez = pq.z - pp.z;
      const float dd = dot3_unfused(ex, ey, ez, ex, ey, ez);
      const float nd = dot3_unfused(np.x, np.y, np.z, ex, ey, ez);
      float wp = 1.0f - (__builtin_fabsf(nd) / __builtin_sqrtf(dd)) / a.sigma_plane;
      wp = wp > 0.0f ? wp : 0.0f;
      wp = dd > 0.0f ? wp : 1.0f;
      wp = sky_p && sky_q ? 1.0f : wp;
      // w_c
      const float cr = up.x - uq.x, cg = up.y - uq.y, cb = up.z - uq.z;
      const float d = (cr * cr + cg * cg) + cb * cb;
      const float wc = colour ? 1.0f / (1.0f + d / a.sigma2) : 1.0f;
      const float w = ((kk * wn) * wp) * wc;
      sr += w * uq.x;
      sg += w * uq.y;
      sb += w * uq.z;
      sw += w;
    }
  }
  const float r = sr / sw, g = sg / sw, b = sb / sw;
  if (LAST) {
    const RT_GLOBAL float *g_a = as_global(a.albedo) + 3 * o;
    const uint32_t h = as_global(a.hits)[o];
    RT_GLOBAL float *out = as_global(a.out) + 3 * o;
    out[0] = (r * demod(g_a[0], h, a.spp, a.spp_f)) * a.spp_f;
    out[1] = (g * demod(g_a[1], h, a.spp, a.spp_f)) * a.spp_f;
    out[2] = (b * demod(g_a[2], h, a.spp, a.spp_f)) * a.spp_f;
  } else {
    f4 v;
    v.x = r;
    v.y = g;
    v.z = b;
    v.w = 0.0f;
    as_global(a.dst)[o] = v;
  }
}

}  // namespace rtk

namespace {

// the desc's options with the defaults filled in; false: out of range
struct dn_options {
  int iterations, normal_power;
  float sigma_plane, sigma_color;  // sigma_color 0 = the term is off
};

bool resolve(const rt_denoise_desc *d, dn_options &o) {
  if (!rtk::post_size_ok(d->width, d->height)) return false;
  if (d->spp < 1 || d->reserved != 0) return false;
  if (!d->beauty || !d->hits || !d->position || !d->normal || !d->albedo || !d->out) return false;
  o.iterations = d->iterations == 0 ? rtk::kDnDefaultIterations : d->iterations;
  if (o.iterations < 1 || o.iterations > 8) return false;
  o.normal_power = d->normal_power == 0 ? rtk::kDnDefaultNormalPower : d->normal_power == -1 ? 0 : d->normal_power;
  if (o.normal_power < 0 || o.normal_power > 10) return false;
  o.sigma_plane = d->sigma_plane == 0.0f ? rtk::kDnDefaultSigmaPlane : d->sigma_plane;
  if (!(o.sigma_plane > 0.0f)) return false;  // (NaN too)
  o.sigma_color = d->sigma_color == 0.0f ? rtk::kDnDefaultSigmaColor : d->sigma_color == -1.0f ? 0.0f : d->sigma_color;
  if (!(o.sigma_color >= 0.0f) || std::isinf(o.sigma_color)) return false;
  return true;
}

// scratch layout: guides n, guides p, colour plane 0, colour plane 1
size_t plane_bytes(int w, int h) { return (size_t)w * (size_t)h * sizeof(rtk::f4); }

// prepare + the iterations on st; d holds DEVICE pointers
int enqueue(const rt_denoise_desc *d, const dn_options &o, void *scratch, hipStream_t st) {
  const size_t pb = plane_bytes(d->width, d->height);
  char *s = static_cast<char *>(scratch);
  rtk::f4 *plane[2] = {reinterpret_cast<rtk::f4 *>(s + 2 * pb), reinterpret_cast<rtk::f4 *>(s + 3 * pb)};
  rtk::dn_params a;
  std::memset(&a, 0, sizeof a);
  a.width = d->width;
  a.height = d->height;
  a.spp = d->spp;
  a.spp_f = (float)d->spp;
  a.beauty = d->beauty;
  a.hits = d->hits;
  a.position = d->position;
  a.normal = d->normal;
  a.albedo = d->albedo;
  a.out = d->out;
  a.guide_n = reinterpret_cast<rtk::f4 *>(s);
  a.guide_p = reinterpret_cast<rtk::f4 *>(s + pb);
  a.dst = plane[0];
  a.normal_power = o.normal_power;
  a.sigma_plane = o.sigma_plane;
  const size_t npx = (size_t)d->width * (size_t)d->height;
  rtk::prepare_kernel<<<(unsigned)((npx + 255) / 256), 256, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  const dim3 grid = rtk::post_grid(d->width, d->height);
  for (int i = 0; i < o.iterations; ++i) {
    a.src = plane[i & 1];
    a.dst = plane[(i + 1) & 1];
    a.step = 1 << i;
    const float sg = o.sigma_color * (1.0f / (float)(1 << i));
    a.sigma2 = sg * sg;
    // (a colour sigma whose square underflows to 0 would read as "off")
    if (o.sigma_color != 0.0f && a.sigma2 == 0.0f) return RT_ERR_INVALID;
    if (i == o.iterations - 1)
      rtk::atrous_kernel<true><<<grid, 256, 0, st>>>(a);
    else
      rtk::atrous_kernel<false><<<grid, 256, 0, st>>>(a);
    RT_HIP(hipGetLastError());
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_denoise_version(void) { return RT_DENOISE_VERSION; }

size_t rt_denoise_scratch_bytes(int width, int height) {
  if (!rtk::post_size_ok(width, height)) return 0;
  return 4 * plane_bytes(width, height);
}

int rt_denoise_async(rt_context *c, const rt_denoise_desc *d, void *scratch, void *stream) {
  dn_options o;
  if (!c || !d || !scratch || ((uintptr_t)scratch & 15) || !resolve(d, o)) return RT_ERR_INVALID;
  rt_pass_scope ps(c, nullptr, nullptr, stream);
  return ps.end(ps.status == RT_OK ? enqueue(d, o, scratch, ps.fs.stream) : ps.status);
}

int rt_denoise(rt_context *c, const rt_denoise_desc *host, double *kernel_ms) {
  dn_options o;
  if (!c || !host || !resolve(host, o)) return RT_ERR_INVALID;
  const size_t npx = (size_t)host->width * (size_t)host->height;
  // beauty / out (filtered in place), hits, position, normal, albedo, the scratch
  const rt_sync_part parts[6] = {{12 * npx, host->beauty, host->out}, {4 * npx, host->hits, nullptr},
                                 {12 * npx, host->position, nullptr}, {12 * npx, host->normal, nullptr},
                                 {12 * npx, host->albedo, nullptr},
                                 {rt_denoise_scratch_bytes(host->width, host->height), nullptr, nullptr}};
  return rt_sync_pass(c, nullptr, nullptr, parts, kernel_ms, [&](void *const *dev, const rt_frame_setup &fs) {
    rt_denoise_desc d = *host;
    d.beauty = d.out = static_cast<float *>(dev[0]);
    d.hits = static_cast<uint32_t *>(dev[1]);
    d.position = static_cast<float *>(dev[2]);
    d.normal = static_cast<float *>(dev[3]);
    d.albedo = static_cast<float *>(dev[4]);
    return enqueue(&d, o, dev[5], fs.stream);
  });
}

}  // extern "C"
