// rt_ray_batch.h -- internal: the kernel and the host half of the two passes
// over the caller's own ray batches, rt_trace.hip (closest hits) and
// rt_segment.hip (closest hits within a per-ray distance limit).  Each includes
// this once, nothing else does; LIMIT says which of the two is compiled, and
// with LIMIT false nothing of the limit is.
//
// Ray i is rt_aov's sample of a lens-less primary ray with the same origin and
// unnormalised direction, by construction: normalize3, closest_hit<> with the
// scan / BVH / layer-grid walks, refine_root and the hit block are the render
// kernel's own code (csrc/rt_device.h, csrc/rt_trace_pass.h), compiled with
// the same flags.  The walk / skip / surface loop is restated here from
// rt_aov.hip rather than shared with it: moved into one function, it cost
// aov_kernel ten VGPRs and a wave of occupancy.
//
// The limit is where the walk starts.  All three walks stop at hit_state::tmax
// (the grid DDA's lim, the layer walk's tyl_fc, the BVH's tf), so a walk that
// starts at tmax = the ray's limit instead of +inf is cut short by every one
// of them: closest_hit<>'s trailing `seed`, which no other caller passes.
//
// The seed is hit_state{tlim, 0}.  candidate<> takes a root when its key
// (root bits, tie2 | near) is BELOW the current one: against (tlim, 0) that is
// every root strictly below tlim and no root equal to it, whatever the
// interval flag and whichever way ties go (no key with tlim's bits is below
// lo = 0).  A walk that found nothing returns tmax == tlim, and one that found
// something returns tmax < tlim, so the miss is still recognisable; with
// tlim = +inf that is best_of's own test, and the walk is the unlimited one
// bit for bit (no_hit()'s lo = 0xffffffff only lets a root of +inf in, which
// best_of then reports as no hit).
#ifndef RTOW_RT_RAY_BATCH_H
#define RTOW_RT_RAY_BATCH_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_trace_pass.h"

namespace rtk {

constexpr int kRayMiss = -1, kRayInvalid = -2;  // RT_TRACE_MISS / _INVALID, RT_SEGMENT_MISS / _INVALID

struct batch_params {
  kparams k;  // the scene and the grid; the camera and frame fields are zero
  const float *origin, *direction, *t_max;  // t_max NULL: +inf for every ray
  uint8_t *blocked;
  int32_t *id;
  float *t, *position, *normal;
  uint32_t first, end;  // this launch's rays [first, end)
};
static_assert(offsetof(batch_params, k) == 0, "kernargs() reads a kparams at offset 0");

// what ray i found; a NULL output is not wanted
template <bool LIMIT>
__device__ __forceinline__ void batch_store(const batch_params &a, uint32_t i, int id, float t, float px, float py,
                                            float pz, float nx, float ny, float nz) {
  const size_t o3 = 3 * (size_t)i;
  if (LIMIT && a.blocked) as_global(a.blocked)[i] = id >= 0 ? 1 : 0;
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

// One lane per ray.  The block stages the grid first (a barrier every lane
// reaches); then the lanes past the launch's range, the invalid rays and (LIMIT)
// the rays whose segment is empty leave, and closest_hit<> runs under the
// remaining lanes' mask (it is wave-uniform and does not care which lanes those
// are).  No static LDS: every grid placement the context chose for the render
// fits here too.
template <bool LIMIT, bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void batch_kernel(const batch_params a) {
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
  [[maybe_unused]] float tm = inf;
  if constexpr (LIMIT) tm = a.t_max ? as_global(a.t_max)[i] : inf;
  // normalize3's l2: a non-finite direction component makes it non-finite
  const float l2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  if (!(fabsf(ox) < inf && fabsf(oy) < inf && fabsf(oz) < inf && l2 > 0.0f && l2 < inf) || (LIMIT && tm != tm)) {
    batch_store<LIMIT>(a, i, kRayInvalid, inf, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  [[maybe_unused]] float lim = inf;  // the limit on the normalised ray: t_max times the direction's length
  if constexpr (LIMIT) lim = length_of(l2);
  const float tmin = normalize3(dx, dy, dz);
  if constexpr (LIMIT) lim *= tm;
  int id = kRayMiss;
  float t = inf, hx = 0.0f, hy = 0.0f, hz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
  // A limit at or below zero must not reach candidate<>: its key compares the
  // float's BITS as an unsigned integer, and a negative float's bits lie above
  // every positive one's -- a seed of -1 would let every root in, like +inf.
  // t_max <= 0 leaves here; tlim > t_min > 0 for every direction normalize3
  // normalises, and the max with 0 keeps the rule where l2 is too small for it
  // (r overflows, t_min is no number).
  if constexpr (LIMIT) {
    if (!(tm > 0.0f) || !(lim > fmaxf(tmin, 0.0f))) {
      batch_store<LIMIT>(a, i, id, t, hx, hy, hz, nx, ny, nz);
      return;
    }
  }
  work_ctr wc;
  // rt_aov.hip's sample loop body, each walk seeded with what is left of the limit
  float walked = 0.0f;  // distance to the current origin (0 unless a spurious root moved it)
  while (true) {
    hit_state hs;
    int best;
    if constexpr (LIMIT) {
      hs = walk<OPEN, BVH, GRID, GP>(p, ox, oy, oz, dx, dy, dz, tmin, wc, hit_state{lim, 0u});
      best = best_below<OPEN>(hs, lim);
    } else {
      hs = walk<OPEN, BVH, GRID, GP>(p, ox, oy, oz, dx, dy, dz, tmin, wc);
      best = best_of<OPEN>(hs);
    }
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
      if constexpr (LIMIT) {
        lim -= tmax;  // (> 0: the root was below it)
        if (!(lim > tmin)) break;
      }
      continue;
    }
    (void)hit_surface(sr, near, tr, ox, oy, oz, dx, dy, dz, hx, hy, hz, nx, ny, nz);
    id = best;
    t = walked + tr;
    break;
  }
  batch_store<LIMIT>(a, i, id, t, hx, hy, hz, nx, ny, nz);
}

}  // namespace rtk

// The host half has internal linkage: each of the two libraries keeps its own.
namespace {

constexpr uint64_t kMaxRays = 0x7fffffffu;  // 2^31 - 1
constexpr int kIn = 3, kOut = 5;
constexpr uint8_t kRayBytes[kIn + kOut] = {12, 12, 4, 1, 4, 4, 12, 12};

// A batch as both passes see it, the pointers all host or all device.  An
// absent t_max or blocked (rt_trace has neither) is NULL, as is an output that
// is not wanted.
struct ray_batch {
  uint64_t n;
  const void *in[kIn];  // origin, direction, t_max
  void *out[kOut];      // blocked, id, t, position, normal
  const void *part(int k) const { return k < kIn ? in[k] : out[k - kIn]; }
  uint64_t bytes(int k) const { return kRayBytes[k] * n; }
};

template <bool LIMIT>
struct batch_variant {
  template <bool O, bool B, bool G, int P>
  struct of {
    static constexpr auto kernel = &rtk::batch_kernel<LIMIT, O, B, G, P>;
  };
};

// the launches over the batch, ascending ranges of at most RT_OPT_LAUNCH_SAMPLES rays
template <bool LIMIT>
int batch_enqueue(const rt_frame_setup &fs, uint32_t flags, const ray_batch &b, std::vector<hipEvent_t> *events) {
  rtk::batch_params bp;
  std::memset(&bp, 0, sizeof bp);
  bp.k = fs.kp;
  bp.origin = static_cast<const float *>(b.in[0]);
  bp.direction = static_cast<const float *>(b.in[1]);
  bp.t_max = static_cast<const float *>(b.in[2]);
  bp.blocked = static_cast<uint8_t *>(b.out[0]);
  bp.id = static_cast<int32_t *>(b.out[1]);
  bp.t = static_cast<float *>(b.out[2]);
  bp.position = static_cast<float *>(b.out[3]);
  bp.normal = static_cast<float *>(b.out[4]);
  const uint64_t per = rt_rays_per_launch(b.n, fs.launch_samples);
  for (uint64_t first = 0; first < b.n; first += per) {
    const uint64_t cnt = std::min<uint64_t>(per, b.n - first);
    bp.first = (uint32_t)first;
    bp.end = (uint32_t)(first + cnt);
    launch_blocks<batch_variant<LIMIT>::template of>(fs, flags, (unsigned)((cnt + rtk::kBlock - 1) / rtk::kBlock), bp);
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

// The argument checks both entry points share, no HIP call and the context
// not read: RT_ERR_INVALID, else RT_OK.  b NULL: the caller's rays or hits were.
int batch_check(const rt_context *c, const ray_batch *b) {
  if (!c || !b) return RT_ERR_INVALID;
  if (b->n > kMaxRays) return RT_ERR_INVALID;
  if (b->n == 0) return RT_OK;
  if (!b->in[0] || !b->in[1]) return RT_ERR_INVALID;
  for (int k = kIn; k < kIn + kOut; ++k)
    for (int j = 0; b->part(k) && j < k; ++j)
      if (b->part(j) && overlap(b->part(k), b->bytes(k), b->part(j), b->bytes(j))) return RT_ERR_INVALID;
  return RT_OK;
}

bool wanted(const ray_batch &b) { return std::any_of(b.out, b.out + kOut, [](void *p) { return p != nullptr; }); }

// the asynchronous form: b's pointers are device pointers, nothing waits
template <bool LIMIT>
int batch_async(rt_context *c, const ray_batch *b, uint32_t flags, void *stream) {
  int r = batch_check(c, b);
  if (r == RT_OK) r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  if (b->n == 0 || !wanted(*b)) return RT_OK;
  rt_pass_scope ps(c, rt_scene_flags{flags}, stream);
  return ps.end(ps.status != RT_OK ? ps.status : batch_enqueue<LIMIT>(ps.fs, flags, *b, nullptr));
}

// the synchronous form: b's pointers are host arrays; t_max is an optional
// input part and every output an optional output part
template <bool LIMIT>
int batch_sync(rt_context *c, const ray_batch *b, uint32_t flags, double *kernel_ms) {
  int r = batch_check(c, b);
  if (r == RT_OK) r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  if (b->n == 0 || !wanted(*b)) return RT_OK;
  rt_sync_part parts[kIn + kOut];
  for (int k = 0; k < kIn + kOut; ++k)
    parts[k] = {b->part(k) ? (size_t)b->bytes(k) : 0, k < kIn ? b->in[k] : nullptr, k < kIn ? nullptr : b->out[k - kIn]};
  rt_pass_scope ps(c, rt_scene_flags{flags}, nullptr);
  return trace_sync_in(
      ps, parts,
      [&](const rt_frame_setup &fs, void *const *dev, std::vector<hipEvent_t> *events) {
        const ray_batch d = {b->n, {dev[0], dev[1], dev[2]}, {dev[3], dev[4], dev[5], dev[6], dev[7]}};
        return batch_enqueue<LIMIT>(fs, flags, d, events);
      },
      kernel_ms);
}

}  // namespace

#endif  // RTOW_RT_RAY_BATCH_H
