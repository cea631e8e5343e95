// rt_bounce.hip -- the render's path step for the caller's own ray batches
// (include/rt_bounce.h, librtow_bounce.so): ray i traced to its next counted
// hit or the miss, and there the render's material -- scatter direction and
// attenuation -- or the sky's factor; and the render's camera rays written as
// such a batch.  Two gfx950 kernels and their host half.
//
// A ray with key (pix, s, k) and from f is one lane's pass through
// render_kernel's (rt_kernel.hip) segment loop, by construction: normalize3,
// closest_hit<> with the scan / BVH / layer-grid walks, refine_root, the hit
// block (csrc/rt_device.h, csrc/rt_trace_pass.h) and the material helpers are
// the render kernel's own code, compiled with the same flags.  The loop is
// rt_chain.h's restatement of that segment loop for one lane -- both arms of
// the spurious-root rule, the direction normalised again after a skip with
// t_min kept -- with the lambertian block added; it is restated here rather
// than shared, so that guides_kernel and route_kernel stay byte for byte what
// they were.
//
// A library of its own: the ten other code objects stay
// byte for byte what they were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_bounce.h"
#include "rt_trace_pass.h"

namespace rtk {

struct bounce_params {
  kparams k;  // the scene, the grid and seed32; the camera and frame fields are zero
  const float *origin, *direction;
  const int32_t *from;  // NULL: -1 for every ray
  const uint32_t *key;
  uint8_t *status;
  int32_t *id;
  float *t, *position, *normal, *scatter, *attenuation;
  uint32_t first, end;  // this launch's rays [first, end)
  uint32_t n_spheres;
  uint32_t metal_unit;  // RT_FLAG_METAL_UNIT_VECTOR (wave-uniform)
};
static_assert(offsetof(bounce_params, k) == 0, "kernargs() reads a kparams at offset 0");

__device__ __forceinline__ void store3(float *base, size_t o3, float x, float y, float z) {
  if (base) {
    RT_GLOBAL float *g = as_global(base) + o3;
    g[0] = x, g[1] = y, g[2] = z;
  }
}

// what ray i found; a NULL output is not wanted
__device__ __forceinline__ void bounce_store(const bounce_params &a, uint32_t i, uint32_t status, int id, float t,
                                             float px, float py, float pz, float nx, float ny, float nz, float sx,
                                             float sy, float sz, float ar, float ag, float ab) {
  const size_t o3 = 3 * (size_t)i;
  if (a.status) as_global(a.status)[i] = (uint8_t)status;
  if (a.id) as_global(a.id)[i] = id;
  if (a.t) as_global(a.t)[i] = t;
  store3(a.position, o3, px, py, pz);
  store3(a.normal, o3, nx, ny, nz);
  store3(a.scatter, o3, sx, sy, sz);
  store3(a.attenuation, o3, ar, ag, ab);
}

// One lane per ray.  The block stages the grid first (a barrier every lane
// reaches); then the lanes past the launch's range and the invalid rays leave,
// and closest_hit<> runs under the remaining lanes' mask (it is wave-uniform
// and does not care which lanes those are).  No static LDS: every grid
// placement the context chose for the render fits here too.
template <bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void bounce_kernel(const bounce_params a) {
  const kparams &p = a.k;
  stage_grid<GP>(p);
  const uint32_t i = (uint32_t)blockIdx.x * (uint32_t)kBlock + (uint32_t)threadIdx.x + a.first;
  if (i >= a.end) return;
  const size_t o3 = 3 * (size_t)i;
  const RT_GLOBAL float *go = as_global(a.origin) + o3;
  const RT_GLOBAL float *gd = as_global(a.direction) + o3;
  const RT_GLOBAL uint32_t *gk = as_global(a.key) + o3;
  float ox = go[0], oy = go[1], oz = go[2];
  float dx = gd[0], dy = gd[1], dz = gd[2];
  const uint32_t pix = gk[0], sample = gk[1], depth = gk[2];
  const int from = a.from ? as_global(a.from)[i] : -1;
  const float inf = __builtin_inff();
  // normalize3's l2: a non-finite direction component makes it non-finite
  const float l2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  if (!(fabsf(ox) < inf && fabsf(oy) < inf && fabsf(oz) < inf && l2 > 0.0f && l2 < inf) || from < -1 ||
      from >= (int)a.n_spheres || sample >= (1u << 24) || depth >= (1u << 24) - 1u) {
    bounce_store(a, i, RT_BOUNCE_INVALID, -2, inf, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  float tmin = normalize3(dx, dy, dz);
  work_ctr wc;
  float walked = 0.0f;  // distance to the current origin (first-arm skips that moved it)
  // render_kernel's segment loop for this lane, to the next counted hit or the miss
  while (true) {
    const hit_state hs = walk<OPEN, BVH, GRID, GP>(p, ox, oy, oz, dx, dy, dz, tmin, wc);
    const int best = best_of<OPEN>(hs);
    if (best < 0) {
      // miss: the sky gradient's factor, src/cpu/main.cc:27-29, in the render's operations
      const float sa = 0.5f * (dy + 1.0f);
      const float s0 = 1.0f - sa;
      bounce_store(a, i, RT_BOUNCE_MISS, -1, inf, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, fmaf(sa, 0.5f, s0),
                   fmaf(sa, 0.7f, s0), s0 + sa);
      return;
    }
    // render_kernel's hit block
    shade_rec sr;
    float tmax, t, b;
    const bool near = hit_root(p, hs, best, ox, oy, oz, dx, dy, dz, sr, tmax, t, b);
    if (b > 0.0f && (t < tmin || (best == from && !near))) {
      // a spurious root, either arm: not a segment
      if (t < tmin) {
        ox = fmaf(tmax, dx, ox);
        oy = fmaf(tmax, dy, oy);
        oz = fmaf(tmax, dz, oz);
        walked += tmax;
      } else {
        tmin = __uint_as_float(__float_as_uint(tmax) + 1u);  // nextafter(tmax, +inf), tmax > 0 finite
      }
      // the render's one normalize3 per step: a skipped ray's again, and it keeps its own t_min
      (void)normalize3(dx, dy, dz);
      continue;
    }
    float hx, hy, hz, nx, ny, nz;
    const bool front = hit_surface(sr, near, t, ox, oy, oz, dx, dy, dz, hx, hy, hz, nx, ny, nz);
    // the step's one hash and one polar draw: the hit's unit vector (z = 1 - 2 u1)
    const uint4 r = pcg4d(pix, sample, depth + 1u, p.seed32);
    const float uz = fmaf(-2.0f, unif(r.x), 1.0f);
    float ux, uy;
    polar(fmaf(-uz, uz, 1.0f), unif(r.y), ux, uy);
    const float dn = dot3(dx, dy, dz, nx, ny, nz);
    float rx, ry, rz;
    reflect3(dx, dy, dz, nx, ny, nz, dn, rx, ry, rz);
    // render_kernel's three material blocks, each under its own lane mask
    float sx = rx, sy = ry, sz = rz;
    bool scattered = true;
    const uint32_t kind = sr.kind;
    if (kind == RT_LAMBERTIAN) {
      // the opaque-inside rule, keyed on the root
      scattered = near || !sr.sealed;
      // material.h:19-30
      sx = nx + ux;
      sy = ny + uy;
      sz = nz + uz;
      const float e = 1e-8f;
      if (fabsf(sx) < e && fabsf(sy) < e && fabsf(sz) < e) {
        sx = nx;
        sy = ny;
        sz = nz;
      }
    }
    if (kind == RT_METAL) {
      // material.h:40-46
      float fz = sr.param;
      if (!a.metal_unit) fz *= ball_radius(r);  // random_in_unit_sphere
      sx = fmaf(fz, ux, rx);
      sy = fmaf(fz, uy, ry);
      sz = fmaf(fz, uz, rz);
      scattered = dot3(sx, sy, sz, nx, ny, nz) > 0.0f;
    }
    if (kind >= RT_DIELECTRIC) {
      // dielectric, material.h:57-87 (r0 is the same for ior and 1/ior)
      const float ratio = front ? sr.inv_param : sr.param;
      const float cos_t = fminf(-dn, 1.0f);
      const bool cannot = (ratio * ratio) * fmaf(-cos_t, cos_t, 1.0f) > 1.0f;
      if (!(cannot || schlick(cos_t, sr.r0) > unif(r.x))) refract3(dx, dy, dz, nx, ny, nz, cos_t, ratio, sx, sy, sz);
    }
    if (!scattered) sx = sy = sz = 0.0f;
    bounce_store(a, i, scattered ? RT_BOUNCE_SCATTERED : RT_BOUNCE_ABSORBED, best, walked + t, hx, hy, hz, nx, ny, nz,
                 sx, sy, sz, sr.ar, sr.ag, sr.ab);
    return;
  }
}

struct camera_rays_params {
  kparams k;  // the camera and the frame (fill_kparams)
  float *origin, *direction;
  uint32_t *key;
  uint32_t sample0, samples, n;  // n = width * local_rows * samples
};
static_assert(offsetof(camera_rays_params, k) == 0, "the kparams first, like every pass");

// One lane per ray [lrow][col][j]: camera_ray without its normalize3
__global__ __launch_bounds__(kBlock) void camera_rays_kernel(const camera_rays_params a) {
  const kparams &p = a.k;
  const uint32_t i = (uint32_t)blockIdx.x * (uint32_t)kBlock + (uint32_t)threadIdx.x;
  if (i >= a.n) return;
  const uint32_t px = i / a.samples, j = i - px * a.samples;
  const int lrow = (int)(px / (uint32_t)p.width), col = (int)(px - (uint32_t)lrow * (uint32_t)p.width);
  const int band = lrow / p.row_block;
  const int grow = (band * p.band_stride + p.band_offset) * p.row_block + (lrow - band * p.row_block);
  const uint32_t s = a.sample0 + j;
  float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
  uint32_t pix = 0u;
  if (grow < p.height) {  // (a padding row: +0, which rt_bounce reports INVALID)
    pix = (uint32_t)grow * (uint32_t)p.width + (uint32_t)col;
    const uint4 r = pcg4d(pix, s, 0u, p.seed32);
    float ddx = 0.0f, ddy = 0.0f;
    if (p.cam.has_lens) polar(unif(r.z), unif(r.w), ddx, ddy);
    camera_dir(p, r, ddx, ddy, col, grow, ox, oy, oz, dx, dy, dz);
  }
  const size_t o3 = 3 * (size_t)i;
  store3(a.origin, o3, ox, oy, oz);
  store3(a.direction, o3, dx, dy, dz);
  RT_GLOBAL uint32_t *gk = as_global(a.key) + o3;
  gk[0] = pix, gk[1] = s, gk[2] = 0u;
}

}  // namespace rtk

static_assert(RT_BOUNCE_MISS == 0 && RT_BOUNCE_SCATTERED == 1 && RT_BOUNCE_ABSORBED == 2 && RT_BOUNCE_INVALID == 3,
              "the kernel's status values");

namespace {

constexpr uint64_t kMaxRays = 0x7fffffffu;  // 2^31 - 1
constexpr int kIn = 4, kOut = 7;
constexpr uint8_t kRayBytes[kIn + kOut] = {12, 12, 4, 12, 1, 4, 4, 12, 12, 12, 12};

// A batch, the pointers all host or all device.  An absent `from`, and an
// output that is not wanted, is NULL.
struct bounce_batch {
  uint64_t n;
  const void *in[kIn];  // origin, direction, from, key
  void *out[kOut];      // status, id, t, position, normal, scatter, attenuation
  uint64_t seed;
  const void *part(int k) const { return k < kIn ? in[k] : out[k - kIn]; }
  uint64_t bytes(int k) const { return kRayBytes[k] * n; }
};

// the public structs as a batch; NULL where one of them is
const bounce_batch *batch_of(const rt_bounce_rays *r, const rt_bounce_out *o, bounce_batch &b) {
  if (!r || !o) return nullptr;
  b = {r->n,
       {r->origin, r->direction, r->from, r->key},
       {o->status, o->id, o->t, o->position, o->normal, o->scatter, o->attenuation},
       r->seed};
  return &b;
}

template <bool O, bool B, bool G, int P>
struct bounce_variant {
  static constexpr auto kernel = &rtk::bounce_kernel<O, B, G, P>;
};

// the launches over the batch, ascending ranges of at most RT_OPT_LAUNCH_SAMPLES rays
int bounce_enqueue(const rt_frame_setup &fs, uint32_t flags, const bounce_batch &b, std::vector<hipEvent_t> *events) {
  RT_HIP(ensure_turn_table());
  rtk::bounce_params bp;
  std::memset(&bp, 0, sizeof bp);
  bp.k = fs.kp;
  bp.k.seed32 = rt_seed32(b.seed);
  bp.origin = static_cast<const float *>(b.in[0]);
  bp.direction = static_cast<const float *>(b.in[1]);
  bp.from = static_cast<const int32_t *>(b.in[2]);
  bp.key = static_cast<const uint32_t *>(b.in[3]);
  bp.status = static_cast<uint8_t *>(b.out[0]);
  bp.id = static_cast<int32_t *>(b.out[1]);
  bp.t = static_cast<float *>(b.out[2]);
  bp.position = static_cast<float *>(b.out[3]);
  bp.normal = static_cast<float *>(b.out[4]);
  bp.scatter = static_cast<float *>(b.out[5]);
  bp.attenuation = static_cast<float *>(b.out[6]);
  bp.n_spheres = fs.n_spheres;
  bp.metal_unit = (flags & RT_FLAG_METAL_UNIT_VECTOR) ? 1u : 0u;
  const uint64_t per = rt_rays_per_launch(b.n, fs.launch_samples);
  for (uint64_t first = 0; first < b.n; first += per) {
    const uint64_t cnt = std::min<uint64_t>(per, b.n - first);
    bp.first = (uint32_t)first;
    bp.end = (uint32_t)(first + cnt);
    launch_blocks<bounce_variant>(fs, flags, (unsigned)((cnt + rtk::kBlock - 1) / rtk::kBlock), bp);
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
// not read: RT_ERR_INVALID, else RT_OK.  b NULL: the caller's rays or out were.
int bounce_check(const rt_context *c, const bounce_batch *b) {
  if (!c || !b) return RT_ERR_INVALID;
  if (b->n > kMaxRays) return RT_ERR_INVALID;
  if (b->n == 0) return RT_OK;
  if (!b->in[0] || !b->in[1] || !b->in[3]) return RT_ERR_INVALID;
  for (int k = kIn; k < kIn + kOut; ++k)
    for (int j = 0; b->part(k) && j < k; ++j)
      if (b->part(j) && overlap(b->part(k), b->bytes(k), b->part(j), b->bytes(j))) return RT_ERR_INVALID;
  return RT_OK;
}

bool wanted(const bounce_batch &b) { return std::any_of(b.out, b.out + kOut, [](void *p) { return p != nullptr; }); }

// ---- camera rays ----
struct camera_batch {
  int32_t sample0, samples;
  uint64_t n;  // rays
};

// the checks of both camera-ray entry points, no HIP call: the status, and the ray count
int camera_check(const rt_context *c, const rt_camera *cam, const rt_params *prm, int32_t sample0, int32_t samples,
                 const void *origin, const void *direction, const void *key, camera_batch &cb) {
  if (!c || !cam || !prm) return RT_ERR_INVALID;
  if (sample0 < 0 || samples < 0 || (int64_t)sample0 + samples > (1 << 24)) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r == RT_ERR_INVALID) return r;
  // (width * local_rows < 2^63: both are int32)
  const uint64_t px = (uint64_t)prm->width * (uint64_t)prm->local_rows;
  if (samples > 0 && px > kMaxRays / (uint64_t)samples) return RT_ERR_INVALID;
  cb = {sample0, samples, px * (uint64_t)samples};
  if (cb.n > 0 && (!origin || !direction || !key)) return RT_ERR_INVALID;
  return r;
}

int camera_enqueue(const rt_frame_setup &fs, const camera_batch &cb, void *const *dev,
                   std::vector<hipEvent_t> *events) {
  RT_HIP(ensure_turn_table());
  rtk::camera_rays_params cp;
  std::memset(&cp, 0, sizeof cp);
  cp.k = fs.kp;
  cp.origin = static_cast<float *>(dev[0]);
  cp.direction = static_cast<float *>(dev[1]);
  cp.key = static_cast<uint32_t *>(dev[2]);
  cp.sample0 = (uint32_t)cb.sample0;
  cp.samples = (uint32_t)cb.samples;
  cp.n = (uint32_t)cb.n;
  rtk::camera_rays_kernel<<<(unsigned)((cb.n + rtk::kBlock - 1) / rtk::kBlock), rtk::kBlock, 0, fs.stream>>>(cp);
  return trace_launched(fs, events);
}

}  // namespace

extern "C" {

int rt_bounce_version(void) { return RT_BOUNCE_VERSION; }

int rt_bounce_async(rt_context *c, const rt_bounce_rays *dev, const rt_bounce_out *out, uint32_t flags,
                    void *stream) {
  bounce_batch bb;
  const bounce_batch *b = batch_of(dev, out, bb);
  int r = bounce_check(c, b);
  if (r == RT_OK) r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  if (b->n == 0 || !wanted(*b)) return RT_OK;
  rt_pass_scope ps(c, rt_scene_flags{flags}, stream);
  return ps.end(ps.status != RT_OK ? ps.status : bounce_enqueue(ps.fs, flags, *b, nullptr));
}

int rt_bounce(rt_context *c, const rt_bounce_rays *host, const rt_bounce_out *out, uint32_t flags,
              double *kernel_ms) {
  bounce_batch bb;
  const bounce_batch *b = batch_of(host, out, bb);
  int r = bounce_check(c, b);
  if (r == RT_OK) r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  if (b->n == 0 || !wanted(*b)) return RT_OK;
  // `from` is an optional input part and every output an optional output part
  rt_sync_part parts[kIn + kOut];
  for (int k = 0; k < kIn + kOut; ++k)
    parts[k] = {b->part(k) ? (size_t)b->bytes(k) : 0, k < kIn ? b->in[k] : nullptr, k < kIn ? nullptr : b->out[k - kIn]};
  rt_pass_scope ps(c, rt_scene_flags{flags}, nullptr);
  return trace_sync_in(
      ps, parts,
      [&](const rt_frame_setup &fs, void *const *dev, std::vector<hipEvent_t> *events) {
        const bounce_batch d = {b->n,
                                {dev[0], dev[1], dev[2], dev[3]},
                                {dev[4], dev[5], dev[6], dev[7], dev[8], dev[9], dev[10]},
                                b->seed};
        return bounce_enqueue(fs, flags, d, events);
      },
      kernel_ms);
}

int rt_bounce_camera_rays_async(rt_context *c, const rt_camera *cam, const rt_params *prm, int32_t sample0,
                                int32_t samples, float *origin, float *direction, uint32_t *key, void *stream) {
  camera_batch cb;
  const int r = camera_check(c, cam, prm, sample0, samples, origin, direction, key, cb);
  if (r != RT_OK) return r;
  if (cb.n == 0) return RT_OK;
  void *const dev[3] = {origin, direction, key};
  rt_pass_scope ps(c, cam, prm, stream);
  return ps.end(ps.status != RT_OK ? ps.status : camera_enqueue(ps.fs, cb, dev, nullptr));
}

int rt_bounce_camera_rays(rt_context *c, const rt_camera *cam, const rt_params *prm, int32_t sample0,
                          int32_t samples, float *origin, float *direction, uint32_t *key, double *kernel_ms) {
  camera_batch cb;
  const int r = camera_check(c, cam, prm, sample0, samples, origin, direction, key, cb);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  if (cb.n == 0) return RT_OK;
  const size_t b3 = 12 * (size_t)cb.n;
  const rt_sync_part parts[3] = {{b3, nullptr, origin}, {b3, nullptr, direction}, {b3, nullptr, key}};
  return trace_sync(
      c, cam, prm, parts,
      [&](const rt_frame_setup &fs, const rt_params *, void *const *dev, std::vector<hipEvent_t> *events) {
        return camera_enqueue(fs, cb, dev, events);
      },
      kernel_ms);
}

}  // extern "C"
