// rt_upscale.hip -- guided upsampling of a low-resolution frame
// (include/rt_upscale.h, librtow_upscale.so): two small gfx950 kernels and the
// pass's host half.
//
// up_prepare_kernel turns the low-resolution sums into three planes of float4
// (demodulated colour + sky flag, mean position, unit normal), so that a tap
// of the second launch is three 16-byte loads.  upscale_kernel runs one lane
// per output pixel on the 16 x 16 tile: it prepares the pixel's own guides,
// maps its centre ray through the low-resolution view (both steps are
// csrc/rt_reproject.h's, shared with rt_resolve.hip) and gathers the taps.
// The taps are read through the vector cache, not staged in LDS (DESIGN.md
// 13): a tile's footprint in the low-resolution frame depends on the two
// cameras, not on a fixed ratio, and at 2 x its 10 x 10 pixels of three planes
// are 4.8 KB that every lane's four taps hit in L1 / L2 after the first miss.
// Every tap is a load from a CLAMPED pixel coordinate, so it is unconditional
// and never leaves the frame; a tap outside the frame is dropped by a select.
// Stage 2 and stage 3 are rare: they sit behind wave-uniform branches, and
// stage 2's sixteen taps are a rolled loop, so neither adds to the common
// path's registers.
//
// The arithmetic is the header's "Semantics", operation by operation, with
// -ffp-contract=off and the compiler's correctly rounded / and sqrt:
// tests/upscale_ref.py restates it in numpy float32 and gets the same bits.
//
// A library of its own, like the four other passes': the five other code
// objects stay byte for byte what they were.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "rt_upscale.h"
#include "rt_frame.h"
#include "rt_reproject.h"

namespace rtk {

constexpr float kUpDefaultPlaneTol = 0.1f, kUpDefaultNormalCos = -0.5f;

struct up_params {
  int lo_width, lo_height, width, height;
  int lo_spp, spp;
  float lo_spp_f, spp_f;
  float xm, ym;  // float(lo_width - 1), float(lo_height - 1)
  float pt2;     // plane_tol^2
  float normal_cos;
  int plane_test, normal_test;  // 0: the test is left out
  int albedo;                   // 0: RT_UPSCALE_NO_ALBEDO
  rt_temporal_view lo_view;
  rt_resolve_rays rays;
  // the caller's sums
  const float *cur;
  const uint32_t *hits_lo;
  const float *position_lo, *normal_lo, *albedo_lo;
  const uint32_t *hits_hi;
  const float *position_hi, *normal_hi, *albedo_hi;
  float *out;
  uint8_t *stage;  // may be NULL
  f4 *planes;      // scratch: three planes of lo_width * lo_height float4
};

// max(a_c, 1e-3f) of the header (rt_denoise.h's Prepare)
__device__ __forceinline__ float up_demod(float albedo_sum, uint32_t h, int spp, float spp_f) {
  const float a = (albedo_sum + (float)(spp - (int)h)) / spp_f;
  return a > 1e-3f ? a : 1e-3f;
}

// Launch 1: one lane per low-resolution pixel.
__global__ __launch_bounds__(256) void up_prepare_kernel(const up_params a) {
  const size_t npx = (size_t)a.lo_width * (size_t)a.lo_height;
  const size_t o = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (o >= npx) return;
  const RT_GLOBAL float *g_c = as_global(a.cur) + 3 * o;
  const uint32_t h = as_global(a.hits_lo)[o];
  const post_guide g = post_prepare(h, as_global(a.position_lo) + 3 * o, as_global(a.normal_lo) + 3 * o);
  float mr = 1.0f, mg = 1.0f, mb = 1.0f;
  if (a.albedo) {
    const RT_GLOBAL float *g_a = as_global(a.albedo_lo) + 3 * o;
    mr = up_demod(g_a[0], h, a.lo_spp, a.lo_spp_f);
    mg = up_demod(g_a[1], h, a.lo_spp, a.lo_spp_f);
    mb = up_demod(g_a[2], h, a.lo_spp, a.lo_spp_f);
  }
  RT_GLOBAL f4 *pl = as_global(a.planes);
  f4 v;
  v.x = (g_c[0] / a.lo_spp_f) / mr;
  v.y = (g_c[1] / a.lo_spp_f) / mg;
  v.z = (g_c[2] / a.lo_spp_f) / mb;
  v.w = g.sky ? 1.0f : 0.0f;
  pl[o] = v;
  v.x = g.px;
  v.y = g.py;
  v.z = g.pz;
  v.w = 0.0f;
  pl[npx + o] = v;
  v.x = g.nx;
  v.y = g.ny;
  v.z = g.nz;
  pl[2 * npx + o] = v;
}

// What launch 2 knows of its output pixel when it looks at a tap.
struct up_pixel {
  float nx, ny, nz, px, py, pz;
  float lim;  // pt2 * d2
  bool sky;
};

// One tap (tx, ty) of the low-resolution frame: its colour, read from the
// clamped coordinate, and whether it is valid for the pixel (header, step 3).
// guided = false: validity is "lies in the frame" (stage 3).
__device__ __forceinline__ bool up_tap(const up_params &a, const up_pixel &p, int tx, int ty, bool guided, f4 &u) {
  const bool in = tx >= 0 && tx < a.lo_width && ty >= 0 && ty < a.lo_height;
  const int cx = tx < 0 ? 0 : (tx < a.lo_width ? tx : a.lo_width - 1);
  const int cy = ty < 0 ? 0 : (ty < a.lo_height ? ty : a.lo_height - 1);
  const size_t npx = (size_t)a.lo_width * (size_t)a.lo_height;
  const size_t t = (size_t)cy * (size_t)a.lo_width + (size_t)cx;
  const RT_GLOBAL f4 *__restrict__ p0 = as_global(a.planes);
  u = p0[t];
  if (!guided) return in;
  const f4 pt = p0[npx + t];
  const f4 nt = p0[2 * npx + t];
  const bool same = (u.w != 0.0f) == p.sky;
  const float e = dot3_unfused(p.nx, p.ny, p.nz, pt.x - p.px, pt.y - p.py, pt.z - p.pz);
  const bool plane = !a.plane_test || e * e <= p.lim;
  const float g = dot3_unfused(p.nx, p.ny, p.nz, nt.x, nt.y, nt.z);
  const bool facing = !a.normal_test || g >= a.normal_cos;
  return in && same && (p.sky || (plane && facing));
}

// Stage 1 (guided) and stage 3 (not): the four bilinear taps.
__device__ __forceinline__ void up_bilinear(const up_params &a, const up_pixel &p, int xi, int yi, float fx, float fy,
                                            bool guided, float &sw, float &sr, float &sg, float &sb) {
  sw = sr = sg = sb = 0.0f;
#pragma unroll
  for (int dy = 0; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = 0; dx <= 1; ++dx) {
      f4 u;
      const bool valid = up_tap(a, p, xi + dx, yi + dy, guided, u);
      const float b = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy);
      sw = valid ? sw + b : sw;
      sr = valid ? sr + b * u.x : sr;
      sg = valid ? sg + b * u.y : sg;
      sb = valid ? sb + b * u.z : sb;
    }
  }
}

// Launch 2: one lane per output pixel.
__global__ __launch_bounds__(256) void upscale_kernel(const up_params a) {
  int x, y;
  if (!post_pixel(a.width, a.height, x, y)) return;
  const size_t o = (size_t)y * (size_t)a.width + (size_t)x;
  // 1. prepare
  const uint32_t h = as_global(a.hits_hi)[o];
  const post_guide g = post_prepare(h, as_global(a.position_hi) + 3 * o, as_global(a.normal_hi) + 3 * o);
  float mr = 1.0f, mg = 1.0f, mb = 1.0f;
  if (a.albedo) {
    const RT_GLOBAL float *g_a = as_global(a.albedo_hi) + 3 * o;
    mr = up_demod(g_a[0], h, a.spp, a.spp_f);
    mg = up_demod(g_a[1], h, a.spp, a.spp_f);
    mb = up_demod(g_a[2], h, a.spp, a.spp_f);
  }
  // 2. map the pixel into the low-resolution frame
  float D[3];
  rp_centre_ray(a.rays, x, y, D);
  float wq, lx, ly;
  rp_project(a.lo_view, D[0], D[1], D[2], wq, lx, ly);
  lx = lx > 0.0f ? lx : 0.0f;  // (NaN too)
  lx = lx < a.xm ? lx : a.xm;
  ly = ly > 0.0f ? ly : 0.0f;
  ly = ly < a.ym ? ly : a.ym;
  const float xf = __builtin_floorf(lx), yf = __builtin_floorf(ly);
  const float fx = lx - xf, fy = ly - yf;
  const int xi = (int)xf, yi = (int)yf;  // 0 .. w-1, 0 .. h-1
  // 3. what a tap is tested against
  up_pixel p;
  p.nx = g.nx, p.ny = g.ny, p.nz = g.nz;
  p.px = g.px, p.py = g.py, p.pz = g.pz;
  p.sky = g.sky;
  const float qx = g.px - a.rays.eye[0], qy = g.py - a.rays.eye[1], qz = g.pz - a.rays.eye[2];
  p.lim = a.pt2 * dot3_unfused(qx, qy, qz, qx, qy, qz);
  // 4. stage 1
  float sw, sr, sg, sb;
  uint8_t stage = 1;
  up_bilinear(a, p, xi, yi, fx, fy, true, sw, sr, sg, sb);
  if (!(sw > 0.0f)) {
    // 5. stage 2: rare, so a rolled loop
    stage = 2;
    sw = sr = sg = sb = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 16; ++k) {
      f4 u;
      const bool valid = up_tap(a, p, xi + (k & 3) - 1, yi + (k >> 2) - 1, true, u);
      sw = valid ? sw + 1.0f : sw;
      sr = valid ? sr + u.x : sr;
      sg = valid ? sg + u.y : sg;
      sb = valid ? sb + u.z : sb;
    }
    if (!(sw > 0.0f)) {
      // 6. stage 3
      stage = 3;
      up_bilinear(a, p, xi, yi, fx, fy, false, sw, sr, sg, sb);
    }
  }
  // 7. write
  RT_GLOBAL float *out = as_global(a.out) + 3 * o;
  out[0] = ((sr / sw) * mr) * a.lo_spp_f;
  out[1] = ((sg / sw) * mg) * a.lo_spp_f;
  out[2] = ((sb / sw) * mb) * a.lo_spp_f;
  if (a.stage) as_global(a.stage)[o] = stage;
}

}  // namespace rtk

namespace {

// the desc's options with the defaults filled in
struct up_options {
  float plane_tol, normal_cos;
};

using rtk::overlap;

// false: an argument is NULL, out of range or NaN, the eyes differ, or the
// buffers overlap.  scratch: the device entry point's (NULL: the synchronous
// one, which allocates its own)
bool resolve(const rt_upscale_desc *d, const void *scratch, up_options &o) {
  if (!rtk::post_size_ok(d->lo_width, d->lo_height) || !rtk::post_size_ok(d->width, d->height)) return false;
  if (d->lo_spp < 1 || d->spp < 1 || d->reserved != 0 || (d->flags & ~RT_UPSCALE_NO_ALBEDO) != 0) return false;
  const bool albedo = !(d->flags & RT_UPSCALE_NO_ALBEDO);
  if (!d->cur || !d->hits_lo || !d->position_lo || !d->normal_lo || !d->hits_hi || !d->position_hi ||
      !d->normal_hi || !d->out)
    return false;
  if (albedo && (!d->albedo_lo || !d->albedo_hi)) return false;
  if (!rtk::post_option(d->plane_tol, rtk::kUpDefaultPlaneTol, 0.0f, false, INFINITY, o.plane_tol) ||
      !rtk::post_option(d->normal_cos, rtk::kUpDefaultNormalCos, -1.0f, true, 1.0f, o.normal_cos))
    return false;
  if (std::memcmp(d->rays.eye, d->lo_view.eye, sizeof d->rays.eye) != 0) return false;
  const size_t nlo = (size_t)d->lo_width * (size_t)d->lo_height, nhi = (size_t)d->width * (size_t)d->height;
  // what the pass reads (the albedos only when it does), then what it writes
  const struct {
    const void *p;
    size_t n;
  } reads[9] = {{d->cur, 12 * nlo},         {d->hits_lo, 4 * nlo},      {d->position_lo, 12 * nlo},
                {d->normal_lo, 12 * nlo},   {albedo ? d->albedo_lo : nullptr, 12 * nlo},
                {d->hits_hi, 4 * nhi},      {d->position_hi, 12 * nhi}, {d->normal_hi, 12 * nhi},
                {albedo ? d->albedo_hi : nullptr, 12 * nhi}},
    writes[3] = {{d->out, 12 * nhi}, {d->stage, nhi}, {scratch, 48 * nlo}};
  for (int i = 0; i < 3; ++i) {
    for (const auto &r : reads)
      if (overlap(writes[i].p, writes[i].n, r.p, r.n)) return false;
    for (int k = i + 1; k < 3; ++k)
      if (overlap(writes[i].p, writes[i].n, writes[k].p, writes[k].n)) return false;
  }
  return true;
}

// the two launches on st; d holds DEVICE pointers
int enqueue(const rt_upscale_desc *d, const up_options &o, void *scratch, hipStream_t st) {
  rtk::up_params a;
  std::memset(&a, 0, sizeof a);
  a.lo_width = d->lo_width;
  a.lo_height = d->lo_height;
  a.width = d->width;
  a.height = d->height;
  a.lo_spp = d->lo_spp;
  a.spp = d->spp;
  a.lo_spp_f = (float)d->lo_spp;
  a.spp_f = (float)d->spp;
  a.xm = (float)(d->lo_width - 1);
  a.ym = (float)(d->lo_height - 1);
  a.pt2 = o.plane_tol * o.plane_tol;
  a.normal_cos = o.normal_cos;
  a.plane_test = !std::isinf(o.plane_tol);
  a.normal_test = o.normal_cos != -1.0f;
  a.albedo = !(d->flags & RT_UPSCALE_NO_ALBEDO);
  a.lo_view = d->lo_view;
  a.rays = d->rays;
  a.cur = d->cur;
  a.hits_lo = d->hits_lo;
  a.position_lo = d->position_lo;
  a.normal_lo = d->normal_lo;
  a.albedo_lo = d->albedo_lo;
  a.hits_hi = d->hits_hi;
  a.position_hi = d->position_hi;
  a.normal_hi = d->normal_hi;
  a.albedo_hi = d->albedo_hi;
  a.out = d->out;
  a.stage = d->stage;
  a.planes = static_cast<rtk::f4 *>(scratch);
  const size_t nlo = (size_t)d->lo_width * (size_t)d->lo_height;
  rtk::up_prepare_kernel<<<dim3((unsigned)((nlo + 255) / 256)), 256, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  rtk::upscale_kernel<<<rtk::post_grid(d->width, d->height), 256, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_upscale_version(void) { return RT_UPSCALE_VERSION; }

size_t rt_upscale_scratch_bytes(int lo_width, int lo_height) {
  if (!rtk::post_size_ok(lo_width, lo_height)) return 0;
  return 48 * (size_t)lo_width * (size_t)lo_height;
}

int rt_upscale_async(rt_context *c, const rt_upscale_desc *d, void *scratch, void *stream) {
  up_options o;
  if (!c || !d || !scratch || !rtk::post_aligned16(scratch) || !resolve(d, scratch, o)) return RT_ERR_INVALID;
  rt_pass_scope ps(c, nullptr, nullptr, stream);
  return ps.end(ps.status == RT_OK ? enqueue(d, o, scratch, ps.fs.stream) : ps.status);
}

int rt_upscale(rt_context *c, const rt_upscale_desc *host, double *kernel_ms) {
  up_options o;
  if (!c || !host || !resolve(host, nullptr, o)) return RT_ERR_INVALID;
  const size_t nlo = (size_t)host->lo_width * (size_t)host->lo_height;
  const size_t nhi = (size_t)host->width * (size_t)host->height;
  const bool albedo = !(host->flags & RT_UPSCALE_NO_ALBEDO);
  // the five low-resolution sums, the four of the output frame, the scratch, out, stage
  const rt_sync_part parts[12] = {{12 * nlo, host->cur, nullptr},
                                  {4 * nlo, host->hits_lo, nullptr},
                                  {12 * nlo, host->position_lo, nullptr},
                                  {12 * nlo, host->normal_lo, nullptr},
                                  {albedo ? 12 * nlo : 0, host->albedo_lo, nullptr},
                                  {4 * nhi, host->hits_hi, nullptr},
                                  {12 * nhi, host->position_hi, nullptr},
                                  {12 * nhi, host->normal_hi, nullptr},
                                  {albedo ? 12 * nhi : 0, host->albedo_hi, nullptr},
                                  {48 * nlo, nullptr, nullptr},
                                  {12 * nhi, nullptr, host->out},
                                  {host->stage ? nhi : 0, nullptr, host->stage}};
  return rt_sync_pass(c, nullptr, nullptr, parts, kernel_ms, [&](void *const *dev, const rt_frame_setup &fs) {
    rt_upscale_desc d = *host;
    d.cur = static_cast<float *>(dev[0]);
    d.hits_lo = static_cast<uint32_t *>(dev[1]);
    d.position_lo = static_cast<float *>(dev[2]);
    d.normal_lo = static_cast<float *>(dev[3]);
    d.albedo_lo = static_cast<float *>(dev[4]);
    d.hits_hi = static_cast<uint32_t *>(dev[5]);
    d.position_hi = static_cast<float *>(dev[6]);
    d.normal_hi = static_cast<float *>(dev[7]);
    d.albedo_hi = static_cast<float *>(dev[8]);
    d.out = static_cast<float *>(dev[10]);
    d.stage = static_cast<uint8_t *>(dev[11]);
    return enqueue(&d, o, dev[9], fs.stream);
  });
}

}  // extern "C"
