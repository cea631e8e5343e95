// rt_guides.hip -- feature buffers that follow mirror and glass paths
// (include/rt_guides.h, librtow_guides.so): a gfx950 kernel that traces each
// sample's render path through specular surfaces and writes what the first
// rough surface on it looks like (coverage, id, virtual depth, position,
// shading normal, throughput, bounce and escape counts), and its host half.
//
// It is the render's path, by construction: the primary ray, closest_hit<>
// with the scan / BVH / layer-grid walks, refine_root and the helpers of the
// material step are the render kernel's own code (csrc/rt_device.h); the hit
// block -- both arms of the spurious-root rule, the face rule, the metal and
// dielectric blocks -- restates render_kernel's (rt_kernel.hip) line by line,
// and the file is compiled with the render kernel's flags.
//
// A library of its own: librtow.so's and librtow_aov.so's
// device code stay byte for byte what they were.  The context stays opaque
// here; rt_frame.h gives the pass the scene's kernel arguments and keeps it
// serialised with the context's renders.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "rt_device.h"
#include "rt_frame.h"
#include "rt_guides.h"

namespace rtk {

// closest_hit<> re-reads its parameters with kernargs(), a kparams at offset 0
// of the kernarg segment: the kernel's one argument begins with a
// complete kparams, and the pass's own values follow it.
struct guides_params {
  kparams k;  // s_lo / s_cnt: this launch's samples of every pixel; out, units, sums, max_depth: unused
  uint32_t *hits;
  int32_t *id;
  float *depth, *position, *normal, *albedo;
  uint32_t *bounces, *escaped;
  int max_bounces;  // resolved: 0 = follow nothing
  float max_fuzz;
};
static_assert(offsetof(guides_params, k) == 0, "kernargs() reads a kparams at offset 0");

// rt_aov's mapping: one wave64 per 8x8 tile, 4 waves per block, one lane per
// pixel, the launch's samples in ascending order, so a pixel's fp32 sums are
// added in sample order by one lane and do not depend on the walk, the launch
// split or the bands.  Per sample the wave runs one loop over segments:
// closest_hit<> is wave-uniform, so the wave repeats it while any lane's chain
// is alive; a lane whose chain has ended sits the remaining walks out under
// the exec mask (it does not walk again, and it does not leave the loop).
// RT_FLAG_METAL_UNIT_VECTOR is read at run time (wave-uniform).  No static
// LDS: every grid placement the context chose for the render fits here too.
template <bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void guides_kernel(const guides_params a) {
  const kparams &p = a.k;
  // the block's copy of the layer grid, as render_kernel stages it
  if (GP == kGridLds) {
    const RT_GLOBAL f4 *gi = as_global(p.grid_items);
    for (int i = (int)threadIdx.x; i < p.grid_n_items; i += kBlock) s_grid_dyn[i] = gi[i];
    uint16_t *sc = reinterpret_cast<uint16_t *>(s_grid_dyn + p.grid_n_items);
    const RT_GLOBAL uint32_t *gc = as_global(p.grid_cells);
    const uint32_t base = (uint32_t)(uintptr_t)(lds_f4 *)s_grid_dyn;
    for (int i = (int)threadIdx.x; i <= p.grid_n_cells; i += kBlock)
      sc[i] = (uint16_t)(base + ((i < p.grid_n_cells ? gc[i] >> 4 : (uint32_t)p.grid_n_items) << 4));
    __syncthreads();
  } else if (GP == kGridCells) {
    uint16_t *sc = reinterpret_cast<uint16_t *>(s_grid_dyn);
    const RT_GLOBAL uint32_t *gc = as_global(p.grid_cells);
    for (int i = (int)threadIdx.x; i <= p.grid_n_cells; i += kBlock)
      sc[i] = (uint16_t)(i < p.grid_n_cells ? gc[i] >> 4 : (uint32_t)p.grid_n_items);
    __syncthreads();
  }
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
  const int tile = (int)blockIdx.x * kWavesPerBlock + wave;
  const int lane = lane_now();
  const int col = (tile % p.tiles_x) * kTile + (lane & (kTile - 1));
  const int lrow = (tile / p.tiles_x) * kTile + (lane >> 3);
  if (col >= p.width || lrow >= p.local_rows) return;
  const int band = lrow / p.row_block;
  const int grow = (band * p.band_stride + p.band_offset) * p.row_block + (lrow - band * p.row_block);
  const size_t o = (size_t)lrow * (size_t)p.width + (size_t)col;
  RT_GLOBAL uint32_t *g_hits = as_global(a.hits);
  RT_GLOBAL int32_t *g_id = as_global(a.id);
  RT_GLOBAL float *g_depth = as_global(a.depth);
  RT_GLOBAL float *g_pos = as_global(a.position);
  RT_GLOBAL float *g_nrm = as_global(a.normal);
  RT_GLOBAL float *g_alb = as_global(a.albedo);
  RT_GLOBAL uint32_t *g_bnc = as_global(a.bounces);
  RT_GLOBAL uint32_t *g_esc = as_global(a.escaped);
  const bool first = p.s_lo == 0;
  uint32_t hits = 0, bnc = 0, esc = 0;
  int id = -1;
  float dep = 0.0f, sp[3] = {0.0f, 0.0f, 0.0f}, sn[3] = {0.0f, 0.0f, 0.0f}, sa[3] = {0.0f, 0.0f, 0.0f};
  if (!first) {
    if (a.hits) hits = g_hits[o];
    if (a.depth) dep = g_depth[o];
    if (a.bounces) bnc = g_bnc[o];
    if (a.escaped) esc = g_esc[o];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.position) sp[k] = g_pos[3 * o + k];
      if (a.normal) sn[k] = g_nrm[3 * o + k];
      if (a.albedo) sa[k] = g_alb[3 * o + k];
    }
  }
  const bool inside = grow < p.height;  // lanes on padding rows trace nothing
  const uint32_t pix = (uint32_t)grow * (uint32_t)p.width + (uint32_t)col;
  const bool metal_unit = (p.flags & RT_FLAG_METAL_UNIT_VECTOR) != 0;
  work_ctr wc;
  for (int s = p.s_lo; s < p.s_lo + p.s_cnt; ++s) {
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 1.f, dz = 0.f;
    float tmin = 0.001f;
    if (inside) tmin = camera_ray(p, pcg4d(pix, (uint32_t)s, 0u, p.seed32), col, grow, ox, oy, oz, dx, dy, dz);
    float thr = 1.f, thg = 1.f, thb = 1.f;
    int depth = 0;            // counted hits so far: the next hit draws pcg4d(pix, s, depth + 1)
    int origin_sphere = -1;   // the sphere the ray starts on (-1: a camera ray); after the loop, the terminal
    int nb = 0;               // bounces followed
    float walked = 0.0f;      // this segment: distance to the current origin (spurious roots that moved it)
    float total = 0.0f;       // length walked to the last counted hit
    float lpx = 0.f, lpy = 0.f, lpz = 0.f, lnx = 0.f, lny = 0.f, lnz = 0.f;  // the last counted hit's P, N
    bool escaped = false;
    bool alive = inside;
    // one wave-level loop over segments: it repeats while any lane is alive
    while (__builtin_amdgcn_ballot_w64(alive)) {
      hit_state hs = no_hit();
      if (alive) {
        // the render's choice of the first extras group's form (kparams
        // extras_fold), taken at run time as in rt_aov: the class is a
        // wave-uniform branch
        const int fold = GRID ? p.extras_fold : 0;
        if (fold == (kFoldLead | kFoldRest))
          hs = closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldLead | kFoldRest : 0>(ox, oy, oz, dx, dy, dz, tmin, wc);
        else if (fold == kFoldLead)
          hs = closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldLead : 0>(ox, oy, oz, dx, dy, dz, tmin, wc);
        else if (fold == kFoldRest)
          hs = closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldRest : 0>(ox, oy, oz, dx, dy, dz, tmin, wc);
        else
          hs = closest_hit<OPEN, BVH, false, GRID, GP, 0>(ox, oy, oz, dx, dy, dz, tmin, wc);
      }
      if (alive) {
        const int best = best_of<OPEN>(hs);
        bool skipped = false;
        if (best < 0) {
          // the chain left the scene: the terminal is the last surface it hit
          escaped = origin_sphere >= 0;
          alive = false;
        } else {
          // render_kernel's hit block
          const float o2 = dot3(ox, oy, oz, ox, oy, oz);
          const float ox2 = -2.0f * ox, oy2 = -2.0f * oy, oz2 = -2.0f * oz;
          const float tmax = hs.tmax;
          const bool near = near_of(hs) != 0;
          static_assert(sizeof(shade_rec) == 64, "best << 6");
          const shade_rec sr = cload_g((const RT_GLOBAL shade_rec *)((const RT_GLOBAL char *)as_global(p.shade) +
                                                                     ((uint32_t)best << 6)));
          float b;
          const float t = refine_root(sr, tmax, near, ox, oy, oz, dx, dy, dz, o2, ox2, oy2, oz2, b);
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
            const float px = fmaf(t, dx, ox), py = fmaf(t, dy, oy), pz = fmaf(t, dz, oz);
            const bool front = near != (sr.inv_r < 0.0f);
            const float fir = front ? sr.inv_r : -sr.inv_r;
            const float nx = (px - sr.cx) * fir, ny = (py - sr.cy) * fir, nz = (pz - sr.cz) * fir;
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
            lpx = px;
            lpy = py;
            lpz = pz;
            lnx = nx;
            lny = ny;
            lnz = nz;
            origin_sphere = best;
            if (cont && nb < a.max_bounces) {
              ++nb;
              ox = px;
              oy = py;
              oz = pz;
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
      ++hits;
      if (s == 0) id = origin_sphere;
      dep += total;
      sp[0] += lpx;
      sp[1] += lpy;
      sp[2] += lpz;
      sn[0] += lnx;
      sn[1] += lny;
      sn[2] += lnz;
      sa[0] += thr;
      sa[1] += thg;
      sa[2] += thb;
      bnc += (uint32_t)nb;
      esc += escaped ? 1u : 0u;
    }
  }
  if (a.hits) g_hits[o] = hits;
  if (a.id && first) g_id[o] = id;
  if (a.depth) g_depth[o] = dep;
  if (a.bounces) g_bnc[o] = bnc;
  if (a.escaped) g_esc[o] = esc;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (a.position) g_pos[3 * o + k] = sp[k];
    if (a.normal) g_nrm[3 * o + k] = sn[k];
    if (a.albedo) g_alb[3 * o + k] = sa[k];
  }
}

// guides_kernel variant V: bit 0 the open interval, bits 1.. the walk (0 scan,
// 1 BVH, 2 + placement the layer grid), as rt_aov's
template <int V>
void launch_guides_variant(unsigned blocks, size_t lds, hipStream_t st, const guides_params &gp) {
  constexpr bool O = V & 1;
  constexpr int W = V >> 1;
  constexpr bool B = W >= 1, G = W >= 2;
  constexpr int P = G ? W - 2 : kGridGlobal;
  guides_kernel<O, B, G, P><<<blocks, kBlock, G ? lds : 0, st>>>(gp);
}
using guides_launch_fn = void (*)(unsigned, size_t, hipStream_t, const guides_params &);
template <int... V>
constexpr auto guides_launch_table(std::integer_sequence<int, V...>) {
  return std::array<guides_launch_fn, sizeof...(V)>{&launch_guides_variant<V>...};
}
constexpr auto kGuidesLaunch = guides_launch_table(std::make_integer_sequence<int, 10>{});
static_assert(kGridGlobal == 0 && kGridLds == 1 && kGridCells == 2, "variant = 2 + placement");

// this code object's copy of the lens sample's table, once per device
hipError_t ensure_turn_table() {
  static std::mutex mu;
  static std::vector<char> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  if ((size_t)dev < done.size() && done[(size_t)dev]) return hipSuccess;
  float tab[2 * RT_TURN_TABLE];
  rt_turn_table(tab);
  e = hipMemcpyToSymbol(HIP_SYMBOL(g_turn_tab), tab, sizeof tab);
  if (e != hipSuccess) return e;
  if ((size_t)dev >= done.size()) done.resize((size_t)dev + 1, 0);
  done[(size_t)dev] = 1;
  return hipSuccess;
}

}  // namespace rtk

namespace {

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

bool any_wanted(const rt_guides_buffers *b) {
  return b->hits || b->id || b->depth || b->position || b->normal || b->albedo || b->bounces || b->escaped;
}

// The launches of one pass on fs.stream.  events (may be null): one event is
// appended after each launch, for the synchronous caller to wait on in turn.
int guides_launches(const rt_frame_setup &fs, const rt_params *prm, int max_bounces, float max_fuzz,
                    const rt_guides_buffers *dev, std::vector<hipEvent_t> *events) {
  RT_HIP(rtk::ensure_turn_table());
  rtk::guides_params gp;
  std::memset(&gp, 0, sizeof gp);
  gp.k = fs.kp;
  gp.hits = dev->hits;
  gp.id = dev->id;
  gp.depth = dev->depth;
  gp.position = dev->position;
  gp.normal = dev->normal;
  gp.albedo = dev->albedo;
  gp.bounces = dev->bounces;
  gp.escaped = dev->escaped;
  gp.max_bounces = max_bounces;
  gp.max_fuzz = max_fuzz;
  const unsigned blocks = (unsigned)rt_frame_blocks(prm);
  const bool bvh = (prm->flags & RT_FLAG_ACCEL_BVH) != 0;
  const int walk = !bvh ? 0 : (fs.grid ? 2 + fs.placement : 1);
  const int v = ((prm->flags & RT_FLAG_OPEN_INTERVAL) ? 1 : 0) | (walk << 1);
  // rt_aov's cut: ascending sample ranges over all pixels, `per` samples per
  // pixel and launch, about RT_OPT_LAUNCH_SAMPLES samples at most, at least
  // one; at most kMaxLaunches launches.  spp = 0: one launch that only initialises.
  const double frame_px = (double)prm->width * (double)prm->local_rows;
  long long per = (long long)std::min((double)std::max(prm->spp, 1), std::floor(fs.launch_samples / frame_px));
  per = std::max({per, 1LL, ((long long)prm->spp + rtk::kMaxLaunches - 1) / rtk::kMaxLaunches});
  for (long long s0 = 0; s0 == 0 || s0 < prm->spp; s0 += per) {
    gp.k.s_lo = (int)s0;
    gp.k.s_cnt = (int)std::min<long long>(per, prm->spp - s0);
    rtk::kGuidesLaunch[(size_t)v](blocks, fs.lds_bytes, fs.stream, gp);
    RT_HIP(hipGetLastError());  // a launch that cannot start stops the pass here
    if (events) {
      hipEvent_t ev = nullptr;
      RT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      events->push_back(ev);
      RT_HIP(hipEventRecord(ev, fs.stream));
    }
  }
  return RT_OK;
}

// One pass.  host false: rt_guides_async (bufs are device pointers, nothing
// waits).  Else rt_guides: bufs are host pointers; the pass runs through
// rt_sync_pass and is waited for launch by launch.  Whatever was enqueued, the
// pass ends with the context's ev_done recorded on its stream (rt_pass_scope).
int guides_pass(rt_context *c, const rt_camera *cam, const rt_params *prm, int max_bounces, float max_fuzz,
                const rt_guides_buffers *bufs, void *stream, bool host, double *kernel_ms) {
  const size_t npx = (size_t)prm->width * (size_t)prm->local_rows;
  if (!host || npx == 0) {
    rt_pass_scope ps(c, cam, prm, host ? nullptr : stream);
    return ps.end(ps.status != RT_OK || npx == 0 ? ps.status
                                                 : guides_launches(ps.fs, prm, max_bounces, max_fuzz, bufs, nullptr));
  }
  // the wanted buffers
  const rt_sync_part parts[8] = {{bufs->hits ? 4 * npx : 0, nullptr, bufs->hits},
                                 {bufs->id ? 4 * npx : 0, nullptr, bufs->id},
                                 {bufs->depth ? 4 * npx : 0, nullptr, bufs->depth},
                                 {bufs->position ? 12 * npx : 0, nullptr, bufs->position},
                                 {bufs->normal ? 12 * npx : 0, nullptr, bufs->normal},
                                 {bufs->albedo ? 12 * npx : 0, nullptr, bufs->albedo},
                                 {bufs->bounces ? 4 * npx : 0, nullptr, bufs->bounces},
                                 {bufs->escaped ? 4 * npx : 0, nullptr, bufs->escaped}};
  std::vector<hipEvent_t> events;
  const int r = rt_sync_pass(
      c, cam, prm, parts, kernel_ms,
      [&](void *const *dev, const rt_frame_setup &fs) {
        const rt_guides_buffers d = {static_cast<uint32_t *>(dev[0]), static_cast<int32_t *>(dev[1]),
                                     static_cast<float *>(dev[2]),    static_cast<float *>(dev[3]),
                                     static_cast<float *>(dev[4]),    static_cast<float *>(dev[5]),
                                     static_cast<uint32_t *>(dev[6]), static_cast<uint32_t *>(dev[7])};
        return guides_launches(fs, prm, max_bounces, max_fuzz, &d, &events);
      },
      [&]() -> int {
        // wait launch by launch: a fault surfaces after the launch it happened in
        for (hipEvent_t ev : events) RT_HIP(hipEventSynchronize(ev));
        return RT_OK;
      });
  for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
  return r;
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
  if (!any_wanted(dev)) return RT_OK;
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
  if (!any_wanted(host)) return RT_OK;
  return guides_pass(c, cam, prm, mb, mf, host, nullptr, true, kernel_ms);
}

}  // extern "C"
