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
// One sample's chain -- the segment loop, both arms of the spurious-root rule
// and the metal and dielectric blocks, restated from render_kernel
// (rt_kernel.hip) line by line -- is csrc/rt_chain.h's, shared with
// rt_route.hip; this file says what happens at the terminal.
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

#include "rt_chain.h"
#include "rt_guides.h"
#include "rt_trace_pass.h"

namespace rtk {

struct guides_params {
  kparams k;  // s_lo / s_cnt: this launch's samples of every pixel; out, units, sums, max_depth: unused
  feature_ptrs f;
  uint32_t *bounces, *escaped;
  chain_limits lim;
};
static_assert(offsetof(guides_params, k) == 0, "kernargs() reads a kparams at offset 0");

// rt_trace_pass.h's mapping and sums, and two counters next to them.  Per
// sample rt_chain.h's trace_chain: one wave-level loop over segments, at whose
// end a hit sample's terminal is added to the sums.
// RT_FLAG_METAL_UNIT_VECTOR is read at run time (wave-uniform).  No static LDS:
// every grid placement the context chose for the render fits here too.
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
  for (int s = p.s_lo; s < p.s_lo + p.s_cnt; ++s)
    trace_chain<OPEN, BVH, GRID, GP>(p, px, pix, s, metal_unit, a.lim, wc,
                                     [&](int sphere, float depth, float hx, float hy, float hz, float nx, float ny,
                                         float nz, float thr, float thg, float thb, int nb, bool escaped) {
                                       sums.add(sphere, s, depth, hx, hy, hz, nx, ny, nz, thr, thg, thb);
                                       bnc += (uint32_t)nb;
                                       esc += escaped ? 1u : 0u;
                                     });
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
        gp.lim = {max_bounces, max_fuzz};
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
