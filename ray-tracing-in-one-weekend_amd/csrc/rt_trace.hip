// rt_trace.hip -- closest-hit queries for the caller's own ray batches
// (include/rt_trace.h, librtow_trace.so): a gfx950 kernel that traces ray i of
// a batch to its first hit and writes the sphere, the distance, the hit point
// and the shading normal, and its host half.
//
// Ray i is rt_aov's sample of a lens-less primary ray with the same origin and
// unnormalised direction, by construction: normalize3, closest_hit<> with the
// scan / BVH / layer-grid walks, refine_root and the hit block are the render
// kernel's own code (csrc/rt_device.h, csrc/rt_trace_pass.h), compiled with
// the same flags.  The walk / skip / surface loop is restated here from
// rt_aov.hip rather than shared with it: moved into one function, it cost
// aov_kernel ten VGPRs and a wave of occupancy.
//
// A library of its own: librtow.so's device code stays byte for
// byte what the committed PMC summaries were collected on.  The context stays
// opaque here; rt_api.cpp's rt_internal_scene_begin / rt_internal_frame_end
// (csrc/rt_frame.h) give the pass the scene's kernel arguments without a
// camera and keep it serialised with the context's renders.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_trace.h"
#include "rt_trace_pass.h"

namespace rtk {

struct trace_params {
  kparams k;  // the scene and the grid; the camera and frame fields are zero
  const float *origin, *direction;
  int32_t *id;
  float *t, *position, *normal;
  uint32_t first, end;  // this launch's rays [first, end)
};
static_assert(offsetof(trace_params, k) == 0, "kernargs() reads a kparams at offset 0");

// what ray i found; a NULL output is not wanted
__device__ __forceinline__ void trace_store(const trace_params &a, uint32_t i, int id, float t, float px, float py,
                                            float pz, float nx, float ny, float nz) {
  const size_t o3 = 3 * (size_t)i;
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

// One lane per ray.  The block stages the grid first (a barrier every lane
// reaches); then the lanes past the launch's range and the invalid rays leave,
// and closest_hit<> runs under the remaining lanes' mask (it is wave-uniform
// and does not care which lanes those are).  No static LDS: every grid
// placement the context chose for the render fits here too.
template <bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void trace_kernel(const trace_params a) {
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
  // normalize3's l2: a non-finite direction component makes it non-finite
  const float l2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  if (!(fabsf(ox) < inf && fabsf(oy) < inf && fabsf(oz) < inf && l2 > 0.0f && l2 < inf)) {
    trace_store(a, i, RT_TRACE_INVALID, inf, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float tmin = normalize3(dx, dy, dz);
  int id = RT_TRACE_MISS;
  float t = inf, hx = 0.0f, hy = 0.0f, hz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
  work_ctr wc;
  // rt_aov.hip's sample loop body
  float walked = 0.0f;  // distance to the current origin (0 unless a spurious root moved it)
  while (true) {
    const hit_state hs = walk<OPEN, BVH, GRID, GP>(p, ox, oy, oz, dx, dy, dz, tmin, wc);
    const int best = best_of<OPEN>(hs);
    if (best < 0) break;
    // render_kernel's hit block for a camera ray (origin_sphere = -1)
    shade_rec sr;
    float tmax, tr, b;
    const bool near = hit_root(p, hs, best, ox, oy, oz, dx, dy, dz, sr, tmax, tr, b);
    if (b > 0.0f && tr < tmin) {
      // a spurious root: the same ray from the scan's root point, same
      // t_min, the direction's bits kept
      ox = fmaf(tmax, dx, ox);
      oy = fmaf(tmax, dy, oy);
      oz = fmaf(tmax, dz, oz);
      walked += tmax;
      continue;
    }
    (void)hit_surface(sr, near, tr, ox, oy, oz, dx, dy, dz, hx, hy, hz, nx, ny, nz);
    id = best;
    t = walked + tr;
    break;
  }
  trace_store(a, i, id, t, hx, hy, hz, nx, ny, nz);
}

}  // namespace rtk

namespace {

template <bool O, bool B, bool G, int P>
struct trace_variant {
  static constexpr auto kernel = &rtk::trace_kernel<O, B, G, P>;
};

constexpr uint64_t kMaxRays = 0x7fffffffu;  // 2^31 - 1

// the launches over the batch, ascending ranges of at most RT_OPT_LAUNCH_SAMPLES rays
int trace_enqueue(const rt_frame_setup &fs, uint32_t flags, uint64_t n, const float *origin, const float *direction,
                  void *const *out, std::vector<hipEvent_t> *events) {
  rtk::trace_params tp;
  std::memset(&tp, 0, sizeof tp);
  tp.k = fs.kp;
  tp.origin = origin;
  tp.direction = direction;
  tp.id = static_cast<int32_t *>(out[0]);
  tp.t = static_cast<float *>(out[1]);
  tp.position = static_cast<float *>(out[2]);
  tp.normal = static_cast<float *>(out[3]);
  const uint64_t per = rt_rays_per_launch(n, fs.launch_samples);
  for (uint64_t first = 0; first < n; first += per) {
    const uint64_t cnt = std::min<uint64_t>(per, n - first);
    tp.first = (uint32_t)first;
    tp.end = (uint32_t)(first + cnt);
    launch_blocks<trace_variant>(fs, flags, (unsigned)((cnt + rtk::kBlock - 1) / rtk::kBlock), tp);
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
// not read: RT_ERR_INVALID, else RT_OK.
int trace_check(const rt_context *c, const rt_trace_rays *rays, const rt_trace_hits *hits) {
  if (!c || !rays || !hits) return RT_ERR_INVALID;
  const uint64_t n = rays->n;
  if (n > kMaxRays) return RT_ERR_INVALID;
  if (n == 0) return RT_OK;
  if (!rays->origin || !rays->direction) return RT_ERR_INVALID;
  const void *ptr[6] = {rays->origin, rays->direction, hits->id, hits->t, hits->position, hits->normal};
  const uint64_t bytes[6] = {12 * n, 12 * n, 4 * n, 4 * n, 12 * n, 12 * n};
  for (int k = 2; k < 6; ++k)
    for (int j = 0; ptr[k] && j < k; ++j)
      if (ptr[j] && overlap(ptr[k], bytes[k], ptr[j], bytes[j])) return RT_ERR_INVALID;
  return RT_OK;
}

bool wanted(const rt_trace_hits *h) { return h->id || h->t || h->position || h->normal; }

}  // namespace

extern "C" {

int rt_trace_version(void) { return RT_TRACE_VERSION; }

int rt_trace_async(rt_context *c, const rt_trace_rays *dev, const rt_trace_hits *out, uint32_t flags, void *stream) {
  int r = trace_check(c, dev, out);
  if (r == RT_OK) r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  if (dev->n == 0 || !wanted(out)) return RT_OK;
  void *const ptrs[4] = {out->id, out->t, out->position, out->normal};
  rt_pass_scope ps(c, rt_scene_flags{flags}, stream);
  return ps.end(ps.status != RT_OK ? ps.status
                                   : trace_enqueue(ps.fs, flags, dev->n, dev->origin, dev->direction, ptrs, nullptr));
}

int rt_trace(rt_context *c, const rt_trace_rays *host, const rt_trace_hits *out, uint32_t flags, double *kernel_ms) {
  int r = trace_check(c, host, out);
  if (r == RT_OK) r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  if (host->n == 0 || !wanted(out)) return RT_OK;
  const uint64_t n = host->n;
  const rt_sync_part parts[6] = {{(size_t)(12 * n), host->origin, nullptr},
                                 {(size_t)(12 * n), host->direction, nullptr},
                                 {out->id ? (size_t)(4 * n) : 0, nullptr, out->id},
                                 {out->t ? (size_t)(4 * n) : 0, nullptr, out->t},
                                 {out->position ? (size_t)(12 * n) : 0, nullptr, out->position},
                                 {out->normal ? (size_t)(12 * n) : 0, nullptr, out->normal}};
  rt_pass_scope ps(c, rt_scene_flags{flags}, nullptr);
  return trace_sync_in(
      ps, parts,
      [&](const rt_frame_setup &fs, void *const *dev, std::vector<hipEvent_t> *events) {
        return trace_enqueue(fs, flags, n, static_cast<const float *>(dev[0]), static_cast<const float *>(dev[1]),
                             dev + 2, events);
      },
      kernel_ms);
}

}  // extern "C"
