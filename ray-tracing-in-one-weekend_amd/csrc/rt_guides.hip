// rt_guides.hip -- feature buffers that follow mirror and glass paths
// (include/rt_guides.h, librtow_guides.so): a gfx950 kernel that traces each
// sample's render path through specular surfaces and writes what the first
// rough surface on it looks like (coverage, id, virtual depth, position,
// shading normal, throughput, bounce and escape counts), and its host half.
//
// It is the render's path, by construction: the primary ray, closest_hit<>
// with the scan / BVH / layer-grid walks, refine_root and the helpers of the
// material step are the render kernel's own code (csrc/rt_device.h), and the
// file is compiled with the render kernel's flags.  The grid staging, the
// pixel mapping, the hit block's two halves, the six sums rt_aov also writes
// and the host's launch sequence are csrc/rt_trace_pass.h's, shared with
// rt_aov.hip: max_bounces = -1 gives rt_aov's bytes through the same code.
// What this file still restates of render_kernel (rt_kernel.hip), line by
// line, is both arms of the spurious-root rule and the metal and dielectric
// blocks.
//
// A library of its own: librtow.so's device code stays byte
// for byte what it was.  The context stays opaque here; rt_frame.h gives the
// pass the scene's kernel arguments and keeps it serialised with the context's
// renders.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_guides.h"
#include "rt_trace_pass.h"

namespace rtk {

struct guides_params {
  kparams k;  // s_lo / s_cnt: this launch's samples of every pixel; out, units, sums, max_depth: unused
  feature_ptrs f;
  uint32_t *bounces, *escaped;
  int max_bounces;  // resolved: 0 = follow nothing
  float max_fuzz;
};
static_assert(offsetof(guides_params, k) == 0, "kernargs() reads a kparams at offset 0");

// rt_trace_pass.h's mapping and sums, and two counters next to them.  Per
// sample the wave runs one loop over segments: closest_hit<> is wave-uniform,
// so the wave repeats it while any lane's chain is alive; a lane whose chain
// has ended sits the remaining walks out under the exec mask (it does not walk
// again, and it does not leave the loop).  RT_FLAG_METAL_UNIT_VECTOR is read at
// run time (wave-uniform).  No static LDS: every grid placement the context
// chose for the render fits here too.
template <bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void guides_kernel(const guides_params a) {
  const kparams &p = a.k;
  stage_grid<GP>(p);
  trace_pixel px;
  if (!trace_pixel_of(p, px)) return;
  RT_GLOBAL uint32_t *g_bnc = as_global(a.bounces);
  RT_GLOBAL uint32_t *g_esc = as_global(a.escaped);
  const bool first = p.s_lo == 0;
  feature_sums sums;
  uint32_t bnc = 0, esc = 0;
  sums.load(a.f, px.o, first);
  if (!first) {
    if (a.bounces) bnc = g_bnc[px.o];
    if (a.escaped) esc = g_esc[px.o];
  }
  const uint32_t pix = (uint32_t)px.grow * (uint32_t)p.width + (uint32_t)px.col;
  const bool metal_unit = (p.flags & RT_FLAG_METAL_UNIT_VECTOR) != 0;
  work_ctr wc;
  for (int s = p.s_lo; s < p.s_lo + p.s_cnt; ++s) {
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 1.f, dz = 0.f;
    float tmin = 0.001f;
    if (px.inside)
      tmin = camera_ray(p, pcg4d(pix, (uint32_t)s, 0u, p.seed32), px.col, px.grow, ox, oy, oz, dx, dy, dz);
    float thr = 1.f, thg = 1.f, thb = 1.f;
    int depth = 0;            // counted hits so far: the next hit draws pcg4d(pix, s, depth + 1)
    int origin_sphere = -1;   // the sphere the ray starts on (-1: a camera ray); after the loop, the terminal
    int nb = 0;               // bounces followed
    float walked = 0.0f;      // this segment: distance to the current origin (spurious roots that moved it)
    float total = 0.0f;       // length walked to the last counted hit
    float lpx = 0.f, lpy = 0.f, lpz = 0.f, lnx = 0.f, lny = 0.f, lnz = 0.f;  // the last counted hit's P, N
    bool escaped = false;
    bool alive = px.inside;  // lanes on padding rows trace nothing
    // one wave-level loop over segments: it repeats while any lane is alive
    while (__builtin_amdgcn_ballot_w64(alive)) {
      hit_state hs = no_hit();
      if (alive) hs = walk<OPEN, BVH, GRID, GP>(p, ox, oy, oz, dx, dy, dz, tmin, wc);
      if (alive) {
        const int best = best_of<OPEN>(hs);
        bool skipped = false;
        if (best < 0) {
          // the chain left the scene: the terminal is the last surface it hit
          escaped = origin_sphere >= 0;
          alive = false;
        } else {
          // render_kernel's hit block
          shade_rec sr;
          float tmax, t, b;
          const bool near = hit_root(p, hs, best, ox, oy, oz, dx, dy, dz, sr, tmax, t, b);
          if (b > 0.0f && (t < tmin || (best == origin_sphere && !near))) {
            // a spurious root, either arm: not a segment, not a bounce
            if (t < tmin) {
              ox = fmaf(tmax, dx, ox);
              oy = fmaf(tmax, dy, oy);
              oz = fmaf(tmax, dz, oz);
              walked += tmax;
            } else {
              tmin = __uint_as_float(__float_as_uint(tmax) + 1u);  // nextafter(tmax, +inf), tmax > 0 finite
            }
            skipped = true;
          } else {
            float hx, hy, hz, nx, ny, nz;
            const bool front = hit_surface(sr, near, t, ox, oy, oz, dx, dy, dz, hx, hy, hz, nx, ny, nz);
            const uint32_t kind = sr.kind;
            float sx = 0.f, sy = 0.f, sz = 0.f;
            bool cont = false;
            if (kind != RT_LAMBERTIAN) {  // (a lambertian is a terminal: its scatter is not needed)
              const uint4 r = pcg4d(pix, (uint32_t)s, (uint32_t)(depth + 1), p.seed32);
              const float dn = dot3(dx, dy, dz, nx, ny, nz);
              float rx, ry, rz;
              reflect3(dx, dy, dz, nx, ny, nz, dn, rx, ry, rz);
              sx = rx;
              sy = ry;
              sz = rz;
              if (kind == RT_METAL) {
                // material.h:40-46, with the step's unit vector (z = 1 - 2 u1)
                const float uz = fmaf(-2.0f, unif(r.x), 1.0f);
                float ux, uy;
                polar(fmaf(-uz, uz, 1.0f), unif(r.y), ux, uy);
                float fz = sr.param;
                if (!metal_unit) fz *= ball_radius(r);  // random_in_unit_sphere
                sx = fmaf(fz, ux, rx);
                sy = fmaf(fz, uy, ry);
                sz = fmaf(fz, uz, rz);
                const bool scattered = dot3(sx, sy, sz, nx, ny, nz) > 0.0f;
                cont = scattered && sr.param <= a.max_fuzz;
              }
              if (kind >= RT_DIELECTRIC) {
                // dielectric, material.h:57-87 (r0 is the same for ior and 1/ior)
                const float ratio = front ? sr.inv_param : sr.param;
                const float cos_t = fminf(-dn, 1.0f);
                const bool cannot = (ratio * ratio) * fmaf(-cos_t, cos_t, 1.0f) > 1.0f;
                if (!(cannot || schlick(cos_t, sr.r0) > unif(r.x))) refract3(dx, dy, dz, nx, ny, nz, cos_t, ratio, sx, sy, sz);
                cont = true;
              }
            }
            // attenuation = albedo (dielectrics store 1,1,1: the product is
            // exact), held finite as the render's wide build holds it
            thr = fminf(thr * sr.ar, 0x1p100f);
            thg = fminf(thg * sr.ag, 0x1p100f);
            thb = fminf(thb * sr.ab, 0x1p100f);
            ++depth;
            total += walked + t;
            walked = 0.0f;
            lpx = hx;
            lpy = hy;
            lpz = hz;
            lnx = nx;
            lny = ny;
            lnz = nz;
            origin_sphere = best;
            if (cont && nb < a.max_bounces) {
              ++nb;
              ox = hx;
              oy = hy;
              oz = hz;
              dx = sx;  // normalised below
              dy = sy;
              dz = sz;
            } else {
              alive = false;  // the terminal
            }
          }
        }
        // the render's one normalize3 per step: the bounce direction's, and a
        // skipped ray's again (it keeps its own t_min)
        if (alive) {
          const float tmin_new = normalize3(dx, dy, dz);
          tmin = skipped ? tmin : tmin_new;
        }
      }
    }
    if (origin_sphere >= 0) {
      sums.add(origin_sphere, s, total, lpx, lpy, lpz, lnx, lny, lnz, thr, thg, thb);
      bnc += (uint32_t)nb;
      esc += escaped ? 1u : 0u;
    }
  }
  sums.store(a.f, px.o, first);
  if (a.bounces) g_bnc[px.o] = bnc;
  if (a.escaped) g_esc[px.o] = esc;
}

}  // namespace rtk

namespace {

template <bool O, bool B, bool G, int P>
struct guides_variant {
  static constexpr auto kernel = &rtk::guides_kernel<O, B, G, P>;
};

constexpr int kDefaultBounces = 8;
constexpr int kMaxBounces = 64;

// the options with their defaults filled in; false: out of range
bool resolve_options(const rt_guides_options *o, int *max_bounces, float *max_fuzz) {
  *max_bounces = kDefaultBounces;
  *max_fuzz = 0.0f;
  if (!o) return true;
  if (o->reserved != 0 || o->max_bounces < -1 || o->max_bounces > kMaxBounces) return false;
  if (!(o->max_fuzz >= 0.0f)) return false;  // NaN or negative
  *max_bounces = o->max_bounces == 0 ? kDefaultBounces : std::max(o->max_bounces, 0);
  *max_fuzz = o->max_fuzz;
  return true;
}

// rt_guides (host arrays) or rt_guides_async (device pointers) after the argument checks
int guides_pass(rt_context *c, const rt_camera *cam, const rt_params *prm, int max_bounces, float max_fuzz,
                const rt_guides_buffers *b, void *stream, bool host, double *kernel_ms) {
  void *const bufs[8] = {b->hits, b->id, b->depth, b->position, b->normal, b->albedo, b->bounces, b->escaped};
  static constexpr uint8_t px_bytes[8] = {4, 4, 4, 12, 12, 12, 4, 4};
  return trace_pass(
      c, cam, prm, bufs, px_bytes,
      [&](const rt_frame_setup &fs, const rt_params *, void *const *dev, std::vector<hipEvent_t> *events) {
        rtk::guides_params gp;
        std::memset(&gp, 0, sizeof gp);
        gp.k = fs.kp;
        gp.f = rtk::feature_ptrs_of(dev);
        gp.bounces = static_cast<uint32_t *>(dev[6]);
        gp.escaped = static_cast<uint32_t *>(dev[7]);
        gp.max_bounces = max_bounces;
        gp.max_fuzz = max_fuzz;
        return trace_launches(fs, prm, events, [&](int s_lo, int s_cnt) {
          gp.k.s_lo = s_lo;
          gp.k.s_cnt = s_cnt;
          launch_frame<guides_variant>(fs, prm, gp);
        });
      },
      stream, host, kernel_ms);
}

}  // namespace

extern "C" {

int rt_guides_version(void) { return RT_GUIDES_VERSION; }

int rt_guides_async(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_guides_options *opts,
                    const rt_guides_buffers *dev, void *stream) {
  int mb;
  float mf;
  if (!c || !cam || !prm || !dev || !resolve_options(opts, &mb, &mf)) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  return guides_pass(c, cam, prm, mb, mf, dev, stream, false, nullptr);
}

int rt_guides(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_guides_options *opts,
              const rt_guides_buffers *host, double *kernel_ms) {
  int mb;
  float mf;
  if (!c || !cam || !prm || !host || !resolve_options(opts, &mb, &mf)) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  return guides_pass(c, cam, prm, mb, mf, host, nullptr, true, kernel_ms);
}

}  // extern "C"
