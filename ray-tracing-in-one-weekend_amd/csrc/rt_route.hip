// rt_route.hip -- guide buffers of each pixel's dominant specular route
// (include/rt_route.h, librtow_route.so): a gfx950 kernel that traces each
// sample's chain through specular surfaces, votes per pixel for the route most
// samples took and sums that route's terminals into a per-pixel state; a small
// finalize kernel that turns the state into rt_aov's buffers; and the host
// half.
//
// One sample's chain is csrc/rt_chain.h's trace_chain, the code guides_kernel
// (rt_guides.hip) runs: the same sample, the same terminal.  The grid staging,
// the pixel mapping, the launch table and the launch sequence are
// csrc/rt_trace_pass.h's.  What this file adds is what happens at the
// terminal: the one-sweep majority vote of rt_route.h.
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
#include "rt_route.h"
#include "rt_trace_pass.h"

namespace rtk {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
static_assert(RT_ROUTE_STATE_BYTES_PER_PIXEL == 4 * sizeof(u4), "four planes of 16-byte entries");

// A pixel's state (rt_route.h): one 16-byte entry in each of the four planes,
// moved as one vector load / store each.
struct route_state {
  u4 vote = {0u, 0u, 0u, 0u};            // key, votes, n, hits
  f4 pd = {0.0f, 0.0f, 0.0f, 0.0f};      // P.xyz, depth
  f4 nrm = {0.0f, 0.0f, 0.0f, 0.0f};     // N.xyz; w: id's bits, kept in `id`
  f4 alb = {0.0f, 0.0f, 0.0f, 0.0f};     // albedo.rgb, 0
  int id = -1;

  __device__ __forceinline__ void load(const void *state, size_t npx, size_t o) {
    const RT_GLOBAL u4 *g = as_global(static_cast<const u4 *>(state));
    vote = g[o];
    pd = __builtin_bit_cast(f4, g[npx + o]);
    const u4 nw = g[2 * npx + o];
    nrm = __builtin_bit_cast(f4, nw);
    id = (int)nw.w;
    alb = __builtin_bit_cast(f4, g[3 * npx + o]);
  }
  __device__ __forceinline__ void store(void *state, size_t npx, size_t o) const {
    RT_GLOBAL u4 *g = as_global(static_cast<u4 *>(state));
    u4 nw = __builtin_bit_cast(u4, nrm);
    nw.w = (uint32_t)id;
    u4 aw = __builtin_bit_cast(u4, alb);
    aw.w = 0u;
    g[o] = vote;
    g[npx + o] = __builtin_bit_cast(u4, pd);
    g[2 * npx + o] = nw;
    g[3 * npx + o] = aw;
  }
  // hit sample s: terminal sphere, route key k and the ten features
  __device__ __forceinline__ void add(int sphere, int s, uint32_t k, float depth, float px, float py, float pz,
                                      float nx, float ny, float nz, float ar, float ag, float ab) {
    vote.w += 1u;
    if (s == 0) id = sphere;
    const bool adopt = vote.y == 0u;
    if (adopt || k == vote.x) {
      // adopt: key = k, votes = n = 1, each sum (+0) + x; the key again: one more of each
      vote.x = k;
      vote.y = adopt ? 1u : vote.y + 1u;
      vote.z = adopt ? 1u : vote.z + 1u;
      pd.x = (adopt ? 0.0f : pd.x) + px;
      pd.y = (adopt ? 0.0f : pd.y) + py;
      pd.z = (adopt ? 0.0f : pd.z) + pz;
      pd.w = (adopt ? 0.0f : pd.w) + depth;
      nrm.x = (adopt ? 0.0f : nrm.x) + nx;
      nrm.y = (adopt ? 0.0f : nrm.y) + ny;
      nrm.z = (adopt ? 0.0f : nrm.z) + nz;
      alb.x = (adopt ? 0.0f : alb.x) + ar;
      alb.y = (adopt ? 0.0f : alb.y) + ag;
      alb.z = (adopt ? 0.0f : alb.z) + ab;
    } else {
      vote.y -= 1u;
    }
  }
};

struct route_params {
  kparams k;  // s_lo / s_cnt: this launch's samples of every pixel; out, units, sums, max_depth: unused
  void *state;
  chain_limits lim;
};
static_assert(offsetof(route_params, k) == 0, "kernargs() reads a kparams at offset 0");

// rt_trace_pass.h's mapping (one wave per 8x8 tile, one lane per pixel, samples
// in ascending order) and rt_chain.h's chain per sample; at the terminal, the
// vote.  The first launch of a call (s_lo == 0) starts from the initial state,
// a later one from the stored one; every lane of the frame's tiles inside the
// local buffers stores its state, lanes on padding rows the initial one.  No
// static LDS, as in the other traced passes.
template <bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void route_kernel(const route_params a) {
  const kparams &p = a.k;
  stage_grid<GP>(p);
  trace_pixel px;
  if (!trace_pixel_of(p, px)) return;
  const size_t npx = (size_t)p.width * (size_t)p.local_rows;
  route_state st;
  if (p.s_lo != 0) st.load(a.state, npx, px.o);
  const uint32_t pix = (uint32_t)px.grow * (uint32_t)p.width + (uint32_t)px.col;
  const bool metal_unit = (p.flags & RT_FLAG_METAL_UNIT_VECTOR) != 0;
  work_ctr wc;
  for (int s = p.s_lo; s < p.s_lo + p.s_cnt; ++s)
    trace_chain<OPEN, BVH, GRID, GP>(p, px, pix, s, metal_unit, a.lim, wc,
                                     [&](int sphere, float depth, float hx, float hy, float hz, float nx, float ny,
                                         float nz, float thr, float thg, float thb, int nb, bool escaped) {
                                       const uint32_t k = (((uint32_t)nb << 1) | (escaped ? 1u : 0u)) + 1u;
                                       st.add(sphere, s, k, depth, hx, hy, hz, nx, ny, nz, thr, thg, thb);
                                     });
  st.store(a.state, npx, px.o);
}

struct finalize_params {
  const void *state;
  size_t npx;  // W * local_rows
  uint32_t *hits;
  int32_t *id;
  float *depth, *position, *normal, *albedo;
  uint32_t *route, *matched;
};

// One lane per pixel of the local buffers: the state's four entries in, the
// wanted outputs out (rt_route.h, "Finalize").  n == hits copies the sums;
// otherwise (sum / n) * hits, each correctly rounded (the file is compiled
// without contraction, and hipcc's fp32 division is the correctly rounded
// one).  hits == 0 is n == hits == 0: the zeros are copied.
__global__ __launch_bounds__(kBlock) void route_finalize_kernel(const finalize_params a) {
  const size_t o = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (o >= a.npx) return;
  route_state st;
  st.load(a.state, a.npx, o);
  const uint32_t n = st.vote.z, hits = st.vote.w;
  const bool whole = n == hits;
  const float fn = (float)n, fh = (float)hits;
  const auto fin = [&](float sum) { return whole ? sum : (sum / fn) * fh; };
  if (a.hits) as_global(a.hits)[o] = hits;
  if (a.id) as_global(a.id)[o] = st.id;
  if (a.depth) as_global(a.depth)[o] = fin(st.pd.w);
  if (a.position) {
    as_global(a.position)[3 * o + 0] = fin(st.pd.x);
    as_global(a.position)[3 * o + 1] = fin(st.pd.y);
    as_global(a.position)[3 * o + 2] = fin(st.pd.z);
  }
  if (a.normal) {
    as_global(a.normal)[3 * o + 0] = fin(st.nrm.x);
    as_global(a.normal)[3 * o + 1] = fin(st.nrm.y);
    as_global(a.normal)[3 * o + 2] = fin(st.nrm.z);
  }
  if (a.albedo) {
    as_global(a.albedo)[3 * o + 0] = fin(st.alb.x);
    as_global(a.albedo)[3 * o + 1] = fin(st.alb.y);
    as_global(a.albedo)[3 * o + 2] = fin(st.alb.z);
  }
  if (a.route) as_global(a.route)[o] = st.vote.x - 1u;
  if (a.matched) as_global(a.matched)[o] = n;
}

}  // namespace rtk

namespace {

template <bool O, bool B, bool G, int P>
struct route_variant {
  static constexpr auto kernel = &rtk::route_kernel<O, B, G, P>;
};

constexpr int kDefaultBounces = 8;
constexpr int kMaxBounces = 64;
constexpr size_t kOutputs = 8;
constexpr uint8_t kPxBytes[kOutputs] = {4, 4, 4, 12, 12, 12, 4, 4};

// the options with their defaults filled in; false: out of range
bool resolve_options(const rt_route_options *o, rtk::chain_limits *lim) {
  *lim = {kDefaultBounces, 0.0f};
  if (!o) return true;
  if (o->reserved != 0 || o->max_bounces < -1 || o->max_bounces > kMaxBounces) return false;
  if (!(o->max_fuzz >= 0.0f)) return false;  // NaN or negative
  *lim = {o->max_bounces == 0 ? kDefaultBounces : std::max(o->max_bounces, 0), o->max_fuzz};
  return true;
}

size_t frame_px(const rt_params *prm) {
  return prm->width < 1 || prm->local_rows < 1 ? 0 : (size_t)prm->width * (size_t)prm->local_rows;
}

// does the state (64 bytes per pixel) share a byte with a wanted output?
bool state_overlaps(const void *state, void *const (&out)[kOutputs], size_t npx) {
  const uintptr_t s0 = (uintptr_t)state, s1 = s0 + RT_ROUTE_STATE_BYTES_PER_PIXEL * npx;
  for (size_t k = 0; k < kOutputs; ++k) {
    const uintptr_t b0 = (uintptr_t)out[k], b1 = b0 + kPxBytes[k] * npx;
    if (out[k] && b0 < s1 && s0 < b1) return true;
  }
  return false;
}

// the launches over the sample ranges into the state dev[8], then the finalize
// kernel into the outputs dev[0 .. 8)
int route_enqueue(const rt_frame_setup &fs, const rt_params *prm, void *const *dev, std::vector<hipEvent_t> *events,
                  const rtk::chain_limits &lim) {
  rtk::route_params rp;
  std::memset(&rp, 0, sizeof rp);
  rp.k = fs.kp;
  rp.state = dev[kOutputs];
  rp.lim = lim;
  const int r = trace_launches(fs, prm, events, [&](int s_lo, int s_cnt) {
    rp.k.s_lo = s_lo;
    rp.k.s_cnt = s_cnt;
    launch_frame<route_variant>(fs, prm, rp);
  });
  if (r != RT_OK) return r;
  const size_t npx = frame_px(prm);
  const rtk::finalize_params fp = {dev[kOutputs],
                                   npx,
                                   static_cast<uint32_t *>(dev[0]),
                                   static_cast<int32_t *>(dev[1]),
                                   static_cast<float *>(dev[2]),
                                   static_cast<float *>(dev[3]),
                                   static_cast<float *>(dev[4]),
                                   static_cast<float *>(dev[5]),
                                   static_cast<uint32_t *>(dev[6]),
                                   static_cast<uint32_t *>(dev[7])};
  rtk::route_finalize_kernel<<<(unsigned)((npx + rtk::kBlock - 1) / rtk::kBlock), rtk::kBlock, 0, fs.stream>>>(fp);
  RT_HIP(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_route_version(void) { return RT_ROUTE_VERSION; }

size_t rt_route_state_bytes(int width, int local_rows) {
  return width < 1 || local_rows < 1 ? 0 : (size_t)RT_ROUTE_STATE_BYTES_PER_PIXEL * (size_t)width * (size_t)local_rows;
}

int rt_route_async(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_route_options *opts,
                   const rt_route_buffers *dev, void *state, void *stream) {
  rtk::chain_limits lim;
  if (!c || !cam || !prm || !dev || !resolve_options(opts, &lim)) return RT_ERR_INVALID;
  if (!state || ((uintptr_t)state & 15u) != 0 || dev->state) return RT_ERR_INVALID;
  void *const out[kOutputs] = {dev->hits,   dev->id,     dev->depth, dev->position,
                               dev->normal, dev->albedo, dev->route, dev->matched};
  if (state_overlaps(state, out, frame_px(prm))) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  if (std::all_of(out, out + kOutputs, [](void *b) { return !b; }) || frame_px(prm) == 0) return RT_OK;
  void *const ptrs[kOutputs + 1] = {out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], state};
  rt_pass_scope ps(c, cam, prm, stream);
  return ps.end(ps.status != RT_OK ? ps.status : route_enqueue(ps.fs, prm, ptrs, nullptr, lim));
}

int rt_route(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_route_options *opts,
             const rt_route_buffers *host, double *kernel_ms) {
  rtk::chain_limits lim;
  if (!c || !cam || !prm || !host || !resolve_options(opts, &lim)) return RT_ERR_INVALID;
  void *const out[kOutputs] = {host->hits,   host->id,     host->depth, host->position,
                               host->normal, host->albedo, host->route, host->matched};
  const size_t npx = frame_px(prm);
  if (host->state && state_overlaps(host->state, out, npx)) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  if ((std::all_of(out, out + kOutputs, [](void *b) { return !b; }) && !host->state) || npx == 0) return RT_OK;
  // the eight outputs, and the pass's own state (always there; copied out on request)
  rt_sync_part parts[kOutputs + 1];
  for (size_t k = 0; k < kOutputs; ++k) parts[k] = {out[k] ? kPxBytes[k] * npx : 0, nullptr, out[k]};
  parts[kOutputs] = {RT_ROUTE_STATE_BYTES_PER_PIXEL * npx, nullptr, host->state};
  return trace_sync(
      c, cam, prm, parts,
      [&](const rt_frame_setup &fs, const rt_params *p, void *const *dev, std::vector<hipEvent_t> *events) {
        return route_enqueue(fs, p, dev, events, lim);
      },
      kernel_ms);
}

}  // extern "C"
