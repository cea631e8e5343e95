// rt_aov.hip -- the first-hit feature pass (include/rt_aov.h, librtow_aov.so):
// a second, small gfx950 kernel that traces the render's primary rays, stops
// at the first hit and writes what it found (coverage, id, depth, position,
// shading normal, albedo), and its host half.
//
// It is the render's first segment, by construction: the primary ray
// (pcg4d(pix, sample, 0, seed32), camera_ray), closest_hit<> with the scan /
// BVH / layer-grid walks, refine_root, the spurious-root rule and the
// face-normal rule are the render kernel's own code (csrc/rt_device.h, and
// render_kernel's hit block in rt_kernel.hip, which this kernel restates line
// by line), compiled with the same flags.
//
// A library of its own: librtow.so's device code stays byte for
// byte what the committed PMC summaries were collected on.  The context stays
// opaque here; rt_api.cpp's rt_internal_frame_begin / _end (csrc/rt_frame.h)
// give the pass the scene's kernel arguments and keep it serialised with the
// context's renders.
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

#include "rt_aov.h"
#include "rt_device.h"
#include "rt_frame.h"

namespace rtk {

// closest_hit<> re-reads its parameters with kernargs(), a kparams at offset 0
// of the kernarg segment: the kernel's one argument begins with a complete
// kparams, and the pass's own pointers follow it.
struct aov_params {
  kparams k;  // s_lo / s_cnt: this launch's samples of every pixel; out, units, sums: unused
  uint32_t *hits;
  int32_t *id;
  float *depth, *position, *normal, *albedo;
};
static_assert(offsetof(aov_params, k) == 0, "kernargs() reads a kparams at offset 0");

// One wave64 per 8x8 tile, 4 waves per block, one lane per pixel, looping
// over the launch's samples in ascending order: a pixel's fp32 sums are added
// in sample order by one lane (no pool, no LDS sums), so they do not depend
// on the walk, the launch split or the bands.  The first launch of a call
// (s_lo == 0) starts from +0 and writes id; a later one continues the stored
// sums.  Lanes outside the frame tile leave before the first walk; lanes on
// padding rows (global row >= height) trace nothing and store the initial
// values.  No static LDS: every grid placement the context chose for the
// render (kGridLdsMax next to render_kernel's kStaticLds) fits here too.
template <bool OPEN, bool BVH, bool GRID, int GP>
__global__ __launch_bounds__(kBlock) void aov_kernel(const aov_params a) {
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
  const bool first = p.s_lo == 0;
  uint32_t hits = 0;
  int id = -1;
  float dep = 0.0f, sp[3] = {0.0f, 0.0f, 0.0f}, sn[3] = {0.0f, 0.0f, 0.0f}, sa[3] = {0.0f, 0.0f, 0.0f};
  if (!first) {
    if (a.hits) hits = g_hits[o];
    if (a.depth) dep = g_depth[o];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.position) sp[k] = g_pos[3 * o + k];
      if (a.normal) sn[k] = g_nrm[3 * o + k];
      if (a.albedo) sa[k] = g_alb[3 * o + k];
    }
  }
  if (grow < p.height) {
    const uint32_t pix = (uint32_t)grow * (uint32_t)p.width + (uint32_t)col;
    work_ctr wc;
    for (int s = p.s_lo; s < p.s_lo + p.s_cnt; ++s) {
      float ox, oy, oz, dx, dy, dz;
      const float tmin = camera_ray(p, pcg4d(pix, (uint32_t)s, 0u, p.seed32), col, grow, ox, oy, oz, dx, dy, dz);
      float walked = 0.0f;  // distance to the current origin (0 unless a spurious root moved it)
      while (true) {
        // the render's choice of the first extras group's form (kparams
        // extras_fold), taken here at run time: one kernel per walk, the
        // class a wave-uniform branch
        hit_state hs;
        const int fold = GRID ? p.extras_fold : 0;
        if (fold == (kFoldLead | kFoldRest))
          hs = closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldLead | kFoldRest : 0>(ox, oy, oz, dx, dy, dz, tmin, wc);
        else if (fold == kFoldLead)
          hs = closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldLead : 0>(ox, oy, oz, dx, dy, dz, tmin, wc);
        else if (fold == kFoldRest)
          hs = closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldRest : 0>(ox, oy, oz, dx, dy, dz, tmin, wc);
        else
          hs = closest_hit<OPEN, BVH, false, GRID, GP, 0>(ox, oy, oz, dx, dy, dz, tmin, wc);
        const int best = best_of<OPEN>(hs);
        if (best < 0) break;  // a miss adds nothing
        // render_kernel's hit block for a camera ray (origin_sphere = -1)
        const float o2 = dot3(ox, oy, oz, ox, oy, oz);
        const float ox2 = -2.0f * ox, oy2 = -2.0f * oy, oz2 = -2.0f * oz;
        const float tmax = hs.tmax;
        const bool near = near_of(hs) != 0;
        static_assert(sizeof(shade_rec) == 64, "best << 6");
        const shade_rec sr = cload_g((const RT_GLOBAL shade_rec *)((const RT_GLOBAL char *)as_global(p.shade) +
                                                                   ((uint32_t)best << 6)));
        float b;
        const float t = refine_root(sr, tmax, near, ox, oy, oz, dx, dy, dz, o2, ox2, oy2, oz2, b);
        if (b > 0.0f && t < tmin) {
          // a spurious root: the same ray from the scan's root point, same
          // t_min; not a segment
          ox = fmaf(tmax, dx, ox);
          oy = fmaf(tmax, dy, oy);
          oz = fmaf(tmax, dz, oz);
          walked += tmax;
          continue;
        }
        const float px = fmaf(t, dx, ox), py = fmaf(t, dy, oy), pz = fmaf(t, dz, oz);
        const bool front = near != (sr.inv_r < 0.0f);
        const float fir = front ? sr.inv_r : -sr.inv_r;
        const float nx = (px - sr.cx) * fir, ny = (py - sr.cy) * fir, nz = (pz - sr.cz) * fir;
        ++hits;
        if (s == 0) id = best;
        dep += walked + t;
        sp[0] += px;
        sp[1] += py;
        sp[2] += pz;
        sn[0] += nx;
        sn[1] += ny;
        sn[2] += nz;
        sa[0] += sr.ar;
        sa[1] += sr.ag;
        sa[2] += sr.ab;
        break;
      }
    }
  }
  if (a.hits) g_hits[o] = hits;
  if (a.id && first) g_id[o] = id;
  if (a.depth) g_depth[o] = dep;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (a.position) g_pos[3 * o + k] = sp[k];
    if (a.normal) g_nrm[3 * o + k] = sn[k];
    if (a.albedo) g_alb[3 * o + k] = sa[k];
  }
}

// aov_kernel variant V: bit 0 the open interval, bits 1.. the walk (0 scan,
// 1 BVH, 2 + placement the layer grid)
template <int V>
void launch_aov_variant(unsigned blocks, size_t lds, hipStream_t st, const aov_params &ap) {
  constexpr bool O = V & 1;
  constexpr int W = V >> 1;
  constexpr bool B = W >= 1, G = W >= 2;
  constexpr int P = G ? W - 2 : kGridGlobal;
  aov_kernel<O, B, G, P><<<blocks, kBlock, G ? lds : 0, st>>>(ap);
}
using aov_launch_fn = void (*)(unsigned, size_t, hipStream_t, const aov_params &);
template <int... V>
constexpr auto aov_launch_table(std::integer_sequence<int, V...>) {
  return std::array<aov_launch_fn, sizeof...(V)>{&launch_aov_variant<V>...};
}
constexpr auto kAovLaunch = aov_launch_table(std::make_integer_sequence<int, 10>{});
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

bool any_wanted(const rt_aov_buffers *b) {
  return b->hits || b->id || b->depth || b->position || b->normal || b->albedo;
}

// The launches of one pass on fs.stream.  events (may be null): one event is
// appended after each launch, for the synchronous caller to wait on in turn.
int aov_launches(const rt_frame_setup &fs, const rt_params *prm, const rt_aov_buffers *dev,
                 std::vector<hipEvent_t> *events) {
  RT_HIP(rtk::ensure_turn_table());
  rtk::aov_params ap;
  std::memset(&ap, 0, sizeof ap);
  ap.k = fs.kp;
  ap.hits = dev->hits;
  ap.id = dev->id;
  ap.depth = dev->depth;
  ap.position = dev->position;
  ap.normal = dev->normal;
  ap.albedo = dev->albedo;
  const unsigned blocks = (unsigned)rt_frame_blocks(prm);
  const bool bvh = (prm->flags & RT_FLAG_ACCEL_BVH) != 0;
  const int walk = !bvh ? 0 : (fs.grid ? 2 + fs.placement : 1);
  const int v = ((prm->flags & RT_FLAG_OPEN_INTERVAL) ? 1 : 0) | (walk << 1);
  // ascending sample ranges over all pixels: `per` samples per pixel and
  // launch, about RT_OPT_LAUNCH_SAMPLES samples at most, at least one; at most
  // kMaxLaunches launches.  spp = 0: one launch that only initialises.
  const double frame_px = (double)prm->width * (double)prm->local_rows;
  long long per = (long long)std::min((double)std::max(prm->spp, 1), std::floor(fs.launch_samples / frame_px));
  per = std::max({per, 1LL, ((long long)prm->spp + rtk::kMaxLaunches - 1) / rtk::kMaxLaunches});
  for (long long s0 = 0; s0 == 0 || s0 < prm->spp; s0 += per) {
    ap.k.s_lo = (int)s0;
    ap.k.s_cnt = (int)std::min<long long>(per, prm->spp - s0);
    rtk::kAovLaunch[(size_t)v](blocks, fs.lds_bytes, fs.stream, ap);
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

// One pass.  host false: rt_aov_async (bufs are device pointers, nothing
// waits).  Else rt_aov: bufs are host pointers; the pass runs through
// rt_sync_pass and is waited for launch by launch.  Whatever was enqueued, the
// pass ends with the context's ev_done recorded on its stream (rt_pass_scope).
int aov_pass(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_aov_buffers *bufs, void *stream,
             bool host, double *kernel_ms) {
  const size_t npx = (size_t)prm->width * (size_t)prm->local_rows;
  if (!host || npx == 0) {
    rt_pass_scope ps(c, cam, prm, host ? nullptr : stream);
    return ps.end(ps.status != RT_OK || npx == 0 ? ps.status : aov_launches(ps.fs, prm, bufs, nullptr));
  }
  // the wanted buffers
  const rt_sync_part parts[6] = {{bufs->hits ? 4 * npx : 0, nullptr, bufs->hits},
                                 {bufs->id ? 4 * npx : 0, nullptr, bufs->id},
                                 {bufs->depth ? 4 * npx : 0, nullptr, bufs->depth},
                                 {bufs->position ? 12 * npx : 0, nullptr, bufs->position},
                                 {bufs->normal ? 12 * npx : 0, nullptr, bufs->normal},
                                 {bufs->albedo ? 12 * npx : 0, nullptr, bufs->albedo}};
  std::vector<hipEvent_t> events;
  const int r = rt_sync_pass(
      c, cam, prm, parts, kernel_ms,
      [&](void *const *dev, const rt_frame_setup &fs) {
        const rt_aov_buffers d = {static_cast<uint32_t *>(dev[0]), static_cast<int32_t *>(dev[1]),
                                  static_cast<float *>(dev[2]),    static_cast<float *>(dev[3]),
                                  static_cast<float *>(dev[4]),    static_cast<float *>(dev[5])};
        return aov_launches(fs, prm, &d, &events);
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

int rt_aov_version(void) { return RT_AOV_VERSION; }

int rt_aov_async(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_aov_buffers *dev,
                 void *stream) {
  if (!c || !cam || !prm || !dev) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  if (!any_wanted(dev)) return RT_OK;
  return aov_pass(c, cam, prm, dev, stream, false, nullptr);
}

int rt_aov(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_aov_buffers *host,
           double *kernel_ms) {
  if (!c || !cam || !prm || !host) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  if (!any_wanted(host)) return RT_OK;
  return aov_pass(c, cam, prm, host, nullptr, true, kernel_ms);
}

}  // extern "C"
