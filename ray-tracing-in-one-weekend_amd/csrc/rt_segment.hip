// rt_segment.hip -- closest hits within a per-ray distance limit
// (include/rt_segment.h, librtow_segment.so): rt_trace.hip's kernel with a far
// end per ray, and its host half.
//
// Ray i is rt_trace's ray i, by construction: normalize3, closest_hit<> with
// the scan / BVH / layer-grid walks, refine_root and the hit block are the
// render kernel's own code (csrc/rt_device.h, csrc/rt_trace_pass.h), compiled
// with the same flags.  New is where the walk starts.  All three walks stop at
// hit_state::tmax (the grid DDA's lim, the layer walk's tyl_fc, the BVH's tf),
// so a walk that starts at tmax = the ray's limit instead of +inf is cut short
// by every one of them: closest_hit<>'s trailing `seed`, which no other caller
// passes.
//
// The seed is hit_state{tlim, 0}.  candidate<> takes a root when its key
// (root bits, tie2 | near) is BELOW the current one: against (tlim, 0) that is
// every root strictly below tlim and no root equal to it, whatever the
// interval flag and whichever way ties go (no key with tlim's bits is below
// lo = 0).  A walk that found nothing returns tmax == tlim, and one that found
// something returns tmax < tlim, so the miss is still recognisable; with
// tlim = +inf that is best_of's own test, and the walk is rt_trace's bit for
// bit (no_hit()'s lo = 0xffffffff only lets a root of +inf in, which best_of
// then reports as no hit).
//
// A library of its own: the nine other code objects stay
// byte for byte what they were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_segment.h"
#include "rt_trace_pass.h"

namespace rtk {

struct segment_params {
  kparams k;  // the scene and the grid; the camera and frame fields are zero
  const float *origin, *direction, *t_max;  // t_max NULL: +inf for every ray
  uint8_t *blocked;
  int32_t *id;
  float *t, *position, *normal;
  uint32_t first, end;  // this launch's rays [first, end)
};
static_assert(offsetof(segment_params, k) == 0, "kernargs() reads a kparams at offset 0");

// what ray i found; a NULL output is not wanted
__device__ __forceinline__ void segment_store(const segment_params &a, uint32_t i, int id, float t, float px, float py,
                                              float pz, float nx, float ny, float nz) {
  const size_t o3 = 3 * (size_t)i;
  if (a.blocked) as_global(a.blocked)[i] = id >= 0 ? 1 : 0;
  if (a.id) as_global(a.id)[i] = id;
  if (a.t) as_global(a.t)[i] = t;
  if (a.position) {
    RT_GLOBAL float *g = as_global(a.position) + o3;
    g[0] = px, g[1] = py, g[2] = pz;
  }
  if (a.normal) {
    RT_GLOBAL float *g = as_global(a.normal) + o3;
    g[0] = nx, g[1] = ny, g[2] = nz;
  }
}

// normalize3's l2 r for the direction's l2: the length it multiplies by 0.001f
// for t_min, restated operation by operation (the same bits; inlined next to
// normalize3 the compiler keeps one copy)
__device__ __forceinline__ float length_of(float l2) {
  float r = __uint_as_float(0x5f375a86u - (__float_as_uint(l2) >> 1));
  const float h = 0.5f * l2;
#pragma unroll
  for (int k = 0; k < 3; ++k) r = r * fmaf(-h, r * r, 1.5f);
  return l2 * r;
}

// the walk's result under the seed (lim, 0): nothing below lim, or best_of's sphere
template <bool OPEN>
__device__ __forceinline__ int best_below(const hit_state &hs, float lim) {
  return hs.tmax == lim ? -1 : best_of<OPEN>(hs);
}

// One lane per ray, rt_trace.hip's shape: the block stages the grid first (a
// barrier every lane reaches); then the lanes past the launch's range, the
// invalid rays and the rays whose segment is empty leave, and closest_hit<>
// runs under the remaining lanes' mask.  No static LDS.
template <bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void segment_kernel(const segment_params a) {
  const kparams &p = a.k;
  stage_grid<GP>(p);
  const uint32_t i = (uint32_t)blockIdx.x * (uint32_t)kBlock + (uint32_t)threadIdx.x + a.first;
  if (i >= a.end) return;
  const size_t o3 = 3 * (size_t)i;
  const RT_GLOBAL float *go = as_global(a.origin) + o3;
  const RT_GLOBAL float *gd = as_global(a.direction) + o3;
  float ox = go[0], oy = go[1], oz = go[2];
  float dx = gd[0], dy = gd[1], dz = gd[2];
  const float inf = __builtin_inff();
  const float tm = a.t_max ? as_global(a.t_max)[i] : inf;
  // normalize3's l2: a non-finite direction component makes it non-finite
  const float l2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  if (!(fabsf(ox) < inf && fabsf(oy) < inf && fabsf(oz) < inf && l2 > 0.0f && l2 < inf) || tm != tm) {
    segment_store(a, i, RT_SEGMENT_INVALID, inf, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float len = length_of(l2);
  const float tmin = normalize3(dx, dy, dz);
  // the limit on the normalised ray.  A limit at or below zero must not reach
  // candidate<>: its key compares the float's BITS as an unsigned integer, and
  // a negative float's bits lie above every positive one's -- a seed of -1
  // would let every root in, like +inf.  t_max <= 0 leaves here; tlim > t_min
  // > 0 for every direction normalize3 normalises, and the max with 0 keeps
  // the rule where l2 is too small for it (r overflows, t_min is no number).
  float lim = tm * len;
  int id = RT_SEGMENT_MISS;
  float t = inf, hx = 0.0f, hy = 0.0f, hz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (!(tm > 0.0f) || !(lim > fmaxf(tmin, 0.0f))) {
    segment_store(a, i, id, t, hx, hy, hz, nx, ny, nz);
    return;
  }
  work_ctr wc;
  // rt_trace.hip's loop, each walk seeded with what is left of the limit
  float walked = 0.0f;  // distance to the current origin (0 unless a spurious root moved it)
  while (true) {
    const hit_state hs = walk<OPEN, BVH, GRID, GP>(p, ox, oy, oz, dx, dy, dz, tmin, wc, hit_state{lim, 0u});
    const int best = best_below<OPEN>(hs, lim);
    if (best < 0) break;
    // render_kernel's hit block for a camera ray (origin_sphere = -1)
    shade_rec sr;
    float tmax, tr, b;
    const bool near = hit_root(p, hs, best, ox, oy, oz, dx, dy, dz, sr, tmax, tr, b);
    if (b > 0.0f && tr < tmin) {
      // a spurious root: the same ray from the scan's root point, same
      // t_min, the direction's bits kept, the limit less the distance walked
      ox = fmaf(tmax, dx, ox);
      oy = fmaf(tmax, dy, oy);
      oz = fmaf(tmax, dz, oz);
      walked += tmax;
      lim -= tmax;  // (> 0: the root was below it)
      if (!(lim > tmin)) break;
      continue;
    }
    (void)hit_surface(sr, near, tr, ox, oy, oz, dx, dy, dz, hx, hy, hz, nx, ny, nz);
    id = best;
    t = walked + tr;
    break;
  }
  segment_store(a, i, id, t, hx, hy, hz, nx, ny, nz);
}

}  // namespace rtk

namespace {

template <bool O, bool B, bool G, int P>
struct segment_variant {
  static constexpr auto kernel = &rtk::segment_kernel<O, B, G, P>;
};

constexpr uint64_t kMaxRays = 0x7fffffffu;  // 2^31 - 1
constexpr int kIn = 3, kOut = 5;            // origin, direction, t_max; blocked, id, t, position, normal

// the launches over the batch, ascending ranges of at most RT_OPT_LAUNCH_SAMPLES rays
int segment_enqueue(const rt_frame_setup &fs, uint32_t flags, uint64_t n, const void *const *in, void *const *out,
                    std::vector<hipEvent_t> *events) {
  rtk::segment_params sp;
  std::memset(&sp, 0, sizeof sp);
  sp.k = fs.kp;
  sp.origin = static_cast<const float *>(in[0]);
  sp.direction = static_cast<const float *>(in[1]);
  sp.t_max = static_cast<const float *>(in[2]);
  sp.blocked = static_cast<uint8_t *>(out[0]);
  sp.id = static_cast<int32_t *>(out[1]);
  sp.t = static_cast<float *>(out[2]);
  sp.position = static_cast<float *>(out[3]);
  sp.normal = static_cast<float *>(out[4]);
  const uint64_t per = rt_rays_per_launch(n, fs.launch_samples);
  for (uint64_t first = 0; first < n; first += per) {
    const uint64_t cnt = std::min<uint64_t>(per, n - first);
    sp.first = (uint32_t)first;
    sp.end = (uint32_t)(first + cnt);
    launch_blocks<segment_variant>(fs, flags, (unsigned)((cnt + rtk::kBlock - 1) / rtk::kBlock), sp);
    const int r = trace_launched(fs, events);
    if (r != RT_OK) return r;
  }
  return RT_OK;
}

// [p, p + bytes) and [q, q + qbytes) share a byte
bool overlap(const void *p, uint64_t bytes, const void *q, uint64_t qbytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qbytes && b < a + bytes;
}

// the parts of a pass in one order: the three inputs, then the five outputs
struct segment_parts {
  const void *ptr[kIn + kOut];
  uint64_t bytes[kIn + kOut];
  segment_parts(const rt_segment_rays *r, const rt_segment_hits *h)
      : ptr{r->origin, r->direction, r->t_max, h->blocked, h->id, h->t, h->position, h->normal},
        bytes{12 * r->n, 12 * r->n, 4 * r->n, r->n, 4 * r->n, 4 * r->n, 12 * r->n, 12 * r->n} {}
};

// The argument checks both entry points share, no HIP call and the context
// not read: RT_ERR_INVALID, else RT_OK.
int segment_check(const rt_context *c, const rt_segment_rays *rays, const rt_segment_hits *hits) {
  if (!c || !rays || !hits) return RT_ERR_INVALID;
  const uint64_t n = rays->n;
  if (n > kMaxRays) return RT_ERR_INVALID;
  if (n == 0) return RT_OK;
  if (!rays->origin || !rays->direction) return RT_ERR_INVALID;
  const segment_parts s(rays, hits);
  for (int k = kIn; k < kIn + kOut; ++k)
    for (int j = 0; s.ptr[k] && j < k; ++j)
      if (s.ptr[j] && overlap(s.ptr[k], s.bytes[k], s.ptr[j], s.bytes[j])) return RT_ERR_INVALID;
  return RT_OK;
}

bool wanted(const rt_segment_hits *h) { return h->blocked || h->id || h->t || h->position || h->normal; }

}  // namespace

extern "C" {

int rt_segment_version(void) { return RT_SEGMENT_VERSION; }

int rt_segment_async(rt_context *c, const rt_segment_rays *dev, const rt_segment_hits *out, uint32_t flags,
                     void *stream) {
  int r = segment_check(c, dev, out);
  if (r == RT_OK) r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  if (dev->n == 0 || !wanted(out)) return RT_OK;
  const void *const in[kIn] = {dev->origin, dev->direction, dev->t_max};
  void *const ptrs[kOut] = {out->blocked, out->id, out->t, out->position, out->normal};
  rt_pass_scope ps(c, rt_scene_flags{flags}, stream);
  return ps.end(ps.status != RT_OK ? ps.status : segment_enqueue(ps.fs, flags, dev->n, in, ptrs, nullptr));
}

int rt_segment(rt_context *c, const rt_segment_rays *host, const rt_segment_hits *out, uint32_t flags,
               double *kernel_ms) {
  int r = segment_check(c, host, out);
  if (r == RT_OK) r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  if (host->n == 0 || !wanted(out)) return RT_OK;
  const uint64_t n = host->n;
  const segment_parts s(host, out);
  void *const down[kOut] = {out->blocked, out->id, out->t, out->position, out->normal};
  // t_max is an optional input part and every output an optional output part
  rt_sync_part parts[kIn + kOut];
  for (int k = 0; k < kIn + kOut; ++k)
    parts[k] = {s.ptr[k] ? (size_t)s.bytes[k] : 0, k < kIn ? s.ptr[k] : nullptr, k < kIn ? nullptr : down[k - kIn]};
  rt_pass_scope ps(c, rt_scene_flags{flags}, nullptr);
  return trace_sync_in(
      ps, parts,
      [&](const rt_frame_setup &fs, void *const *dev, std::vector<hipEvent_t> *events) {
        const void *const in[kIn] = {dev[0], dev[1], dev[2]};
        return segment_enqueue(fs, flags, n, in, dev + kIn, events);
      },
      kernel_ms);
}

}  // extern "C"
