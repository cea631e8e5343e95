// rt_trace_pass.h -- internal: what the passes that trace the render's rays
// into feature buffers share (the first-hit pass in rt_aov.hip, the
// chain-following ones in rt_guides.hip and rt_route.hip, those two through
// rt_chain.h as well; each includes this once, nothing else does) -- and
// rt_trace.hip and rt_segment.hip (through rt_ray_batch.h), which trace the
// caller's rays with the same walks, hit block, launch table and synchronous
// form.  On the device: the block's LDS copy of the layer grid, the tile ->
// pixel mapping, the run-time choice of closest_hit<>'s fold class, the hit
// block up to the spurious-root test and from it to the shading normal, and
// the six sums both passes write.  On the host: the launch table over a
// kernel's ten variants, this code object's lens table, the launches over the
// sample ranges and the two forms of a pass (enqueue only, or from host arrays
// to host arrays through rt_frame.h's rt_sync_pass).
//
// The device half restates render_kernel's (rt_kernel.hip) grid staging and
// hit block line by line -- the render kernel does not include this header, its
// code object stays what the committed profiles were collected on -- and is
// inlined into kernels compiled with the render kernel's flags.
#ifndef RTOW_RT_TRACE_PASS_H
#define RTOW_RT_TRACE_PASS_H

#include <hip/hip_runtime.h>

#include <array>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <utility>
#include <vector>

#include "rt_device.h"
#include "rt_frame.h"

namespace rtk {

// The six outputs both passes have (include/rt_aov.h's rt_aov_buffers; NULL =
// not wanted).  A pass's kernel parameters hold them right after the kparams
// that closest_hit<> re-reads with kernargs() at offset 0 of the kernarg segment.
struct feature_ptrs {
  uint32_t *hits;
  int32_t *id;
  float *depth, *position, *normal, *albedo;
};
inline feature_ptrs feature_ptrs_of(void *const *d) {
  return {static_cast<uint32_t *>(d[0]), static_cast<int32_t *>(d[1]), static_cast<float *>(d[2]),
          static_cast<float *>(d[3]),    static_cast<float *>(d[4]),   static_cast<float *>(d[5])};
}

// the block's copy of the layer grid, as render_kernel stages it
template <int GP>
__device__ __forceinline__ void stage_grid(const kparams &p) {
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
}

// A lane's pixel: one wave64 per 8x8 tile, 4 waves per block, one lane per
// pixel.  o: its element in the local buffers; inside: on a row of the frame
// (a lane on a padding row, grow >= height, traces nothing and stores the
// initial values).
struct trace_pixel {
  int col, lrow, grow;
  size_t o;
  bool inside;
};
// false: the lane lies outside the frame's tiles and leaves the kernel (after
// stage_grid's barrier).  Written without a branch of its own: inlined, the
// row arithmetic sinks behind the caller's return, where a branch here would
// stay a second one on the same condition.
__device__ __forceinline__ bool trace_pixel_of(const kparams &p, trace_pixel &px) {
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
  const int tile = (int)blockIdx.x * kWavesPerBlock + wave;
  const int lane = lane_now();
  px.col = (tile % p.tiles_x) * kTile + (lane & (kTile - 1));
  px.lrow = (tile / p.tiles_x) * kTile + (lane >> 3);
  const int band = px.lrow / p.row_block;
  px.grow = (band * p.band_stride + p.band_offset) * p.row_block + (px.lrow - band * p.row_block);
  px.o = (size_t)px.lrow * (size_t)p.width + (size_t)px.col;
  px.inside = px.grow < p.height;
  return px.col < p.width && px.lrow < p.local_rows;
}

// closest_hit<> in the render's choice of the first extras group's form
// (kparams extras_fold), taken here at run time: one kernel per walk, the
// class a wave-uniform branch.  seed: closest_hit<>'s (rt_segment.hip's limit).
template <bool OPEN, bool BVH, bool GRID, int GP>
__device__ __forceinline__ hit_state walk(const kparams &p, float ox, float oy, float oz, float dx, float dy, float dz,
                                          float tmin, work_ctr &wc, const hit_state seed = no_hit()) {
  const int fold = GRID ? p.extras_fold : 0;
  if (fold == (kFoldLead | kFoldRest))
    return closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldLead | kFoldRest : 0>(ox, oy, oz, dx, dy, dz, tmin, wc,
                                                                                     seed);
  if (fold == kFoldLead)
    return closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldLead : 0>(ox, oy, oz, dx, dy, dz, tmin, wc, seed);
  if (fold == kFoldRest)
    return closest_hit<OPEN, BVH, false, GRID, GP, GRID ? kFoldRest : 0>(ox, oy, oz, dx, dy, dz, tmin, wc, seed);
  return closest_hit<OPEN, BVH, false, GRID, GP, 0>(ox, oy, oz, dx, dy, dz, tmin, wc, seed);
}

// render_kernel's hit block in two steps, with the caller's spurious-root test
// (b > 0 and t < tmin, or the ray's own sphere again) between them.  Each
// returns its flag by value: a bool written through a reference reaches the
// kernel as a byte in memory and costs rt_guides a VGPR.
// hit_root: sphere `best` of the walk's result hs -- its shading record sr, the
// scan's root tmax, the refined root t with refine_root's b; returns near, the
// root's side.
__device__ __forceinline__ bool hit_root(const kparams &p, const hit_state &hs, int best, float ox, float oy, float oz,
                                         float dx, float dy, float dz, shade_rec &sr, float &tmax, float &t, float &b) {
  const float o2 = dot3(ox, oy, oz, ox, oy, oz);
  const float ox2 = -2.0f * ox, oy2 = -2.0f * oy, oz2 = -2.0f * oz;
  tmax = hs.tmax;
  const bool near = near_of(hs) != 0;
  static_assert(sizeof(shade_rec) == 64, "best << 6");
  sr = cload_g((const RT_GLOBAL shade_rec *)((const RT_GLOBAL char *)as_global(p.shade) + ((uint32_t)best << 6)));
  t = refine_root(sr, tmax, near, ox, oy, oz, dx, dy, dz, o2, ox2, oy2, oz2, b);
  return near;
}
// hit_surface: the hit point P and the shading normal N (the face rule: 1/r
// signed towards the ray's side); returns front, the side the ray came from.
__device__ __forceinline__ bool hit_surface(const shade_rec &sr, bool near, float t, float ox, float oy, float oz,
                                            float dx, float dy, float dz, float &px, float &py, float &pz, float &nx,
                                            float &ny, float &nz) {
  px = fmaf(t, dx, ox), py = fmaf(t, dy, oy), pz = fmaf(t, dz, oz);
  const bool front = near != (sr.inv_r < 0.0f);
  const float fir = front ? sr.inv_r : -sr.inv_r;
  nx = (px - sr.cx) * fir, ny = (py - sr.cy) * fir, nz = (pz - sr.cz) * fir;
  return front;
}

// A pixel's six sums.  One lane adds its pixel's samples in ascending order (no
// pool, no LDS sums), so the fp32 sums do not depend on the walk, the launch
// split or the bands.  The first launch of a call (first: s_lo == 0) starts
// from +0 and writes id; a later one continues the stored sums.
struct feature_sums {
  uint32_t hits = 0;
  int id = -1;
  float dep = 0.0f, sp[3] = {0.0f, 0.0f, 0.0f}, sn[3] = {0.0f, 0.0f, 0.0f}, sa[3] = {0.0f, 0.0f, 0.0f};

  __device__ __forceinline__ void load(const feature_ptrs &a, size_t o, bool first) {
    if (!first) {
      if (a.hits) hits = as_global(a.hits)[o];
      if (a.depth) dep = as_global(a.depth)[o];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (a.position) sp[k] = as_global(a.position)[3 * o + k];
        if (a.normal) sn[k] = as_global(a.normal)[3 * o + k];
        if (a.albedo) sa[k] = as_global(a.albedo)[3 * o + k];
      }
    }
  }
  // sample s hit: sphere `sphere` (kept for s = 0), at `depth` along its path
  __device__ __forceinline__ void add(int sphere, int s, float depth, float px, float py, float pz, float nx, float ny,
                                      float nz, float ar, float ag, float ab) {
    ++hits;
    if (s == 0) id = sphere;
    dep += depth;
    sp[0] += px;
    sp[1] += py;
    sp[2] += pz;
    sn[0] += nx;
    sn[1] += ny;
    sn[2] += nz;
    sa[0] += ar;
    sa[1] += ag;
    sa[2] += ab;
  }
  __device__ __forceinline__ void store(const feature_ptrs &a, size_t o, bool first) const {
    if (a.hits) as_global(a.hits)[o] = hits;
    if (a.id && first) as_global(a.id)[o] = id;
    if (a.depth) as_global(a.depth)[o] = dep;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.position) as_global(a.position)[3 * o + k] = sp[k];
      if (a.normal) as_global(a.normal)[3 * o + k] = sn[k];
      if (a.albedo) as_global(a.albedo)[3 * o + k] = sa[k];
    }
  }
};

}  // namespace rtk

// The host half has internal linkage: each of the libraries keeps its own.
namespace {

// A pass's kernel by variant: K<OPEN, BVH, GRID, GP>::kernel is the __global__
// function taking a const Params.  Variant bit 0 is the open interval, bits
// 1.. the walk (0 scan, 1 BVH, 2 + placement the layer grid).
template <template <bool, bool, bool, int> class K, class Params, int V>
void launch_variant(unsigned blocks, size_t lds, hipStream_t st, const Params &a) {
  constexpr bool O = V & 1;
  constexpr int W = V >> 1;
  constexpr bool B = W >= 1, G = W >= 2;
  constexpr int P = G ? W - 2 : rtk::kGridGlobal;
  K<O, B, G, P>::kernel<<<blocks, rtk::kBlock, G ? lds : 0, st>>>(a);
}
template <template <bool, bool, bool, int> class K, class Params, int... V>
constexpr auto launch_table(std::integer_sequence<int, V...>) {
  using fn = void (*)(unsigned, size_t, hipStream_t, const Params &);
  return std::array<fn, sizeof...(V)>{&launch_variant<K, Params, V>...};
}
// one launch over `blocks` blocks, of the variant for these flags and the setup's grid
template <template <bool, bool, bool, int> class K, class Params>
void launch_blocks(const rt_frame_setup &fs, uint32_t flags, unsigned blocks, const Params &a) {
  static constexpr auto table = launch_table<K, Params>(std::make_integer_sequence<int, 10>{});
  static_assert(rtk::kGridGlobal == 0 && rtk::kGridLds == 1 && rtk::kGridCells == 2, "variant = 2 + placement");
  const bool bvh = (flags & RT_FLAG_ACCEL_BVH) != 0;
  const int walk = !bvh ? 0 : (fs.grid ? 2 + fs.placement : 1);
  const int v = ((flags & RT_FLAG_OPEN_INTERVAL) ? 1 : 0) | (walk << 1);
  table[(size_t)v](blocks, fs.lds_bytes, fs.stream, a);
}
// ... over the frame's blocks
template <template <bool, bool, bool, int> class K, class Params>
void launch_frame(const rt_frame_setup &fs, const rt_params *prm, const Params &a) {
  launch_blocks<K>(fs, prm->flags, (unsigned)rt_frame_blocks(prm), a);
}

// This code object's copy of the lens sample's table, once per device.
// g_turn_tab is one table per code object, so "done" has to stay private to
// the library this is compiled into: a static function with function-local
// statics.  An inline function's statics are emitted as unique symbols, which
// the dynamic linker merges across librtow_aov.so and librtow_guides.so
// whether or not they are linked -Bsymbolic: the library called second would
// skip its upload and trace lens samples from a table of zeros.
// (rt_trace.hip draws no lens sample and never calls it.)
[[maybe_unused]] static hipError_t ensure_turn_table() {
  static std::mutex mu;
  static std::vector<char> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  if ((size_t)dev < done.size() && done[(size_t)dev]) return hipSuccess;
  float tab[2 * RT_TURN_TABLE];
  rt_turn_table(tab);
  e = hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_turn_tab), tab, sizeof tab);
  if (e != hipSuccess) return e;
  if ((size_t)dev >= done.size()) done.resize((size_t)dev + 1, 0);
  done[(size_t)dev] = 1;
  return hipSuccess;
}

// After each launch of a pass on fs.stream: its status, and for the
// synchronous caller an event to wait on.
inline int trace_launched(const rt_frame_setup &fs, std::vector<hipEvent_t> *events) {
  RT_HIP(hipGetLastError());  // a launch that cannot start stops the pass here
  if (events) {
    hipEvent_t ev = nullptr;
    RT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    events->push_back(ev);
    RT_HIP(hipEventRecord(ev, fs.stream));
  }
  return RT_OK;
}

// The launches of one pass on fs.stream: launch(s_lo, s_cnt) for each of the
// frame's sample ranges (rt_frame.h).  events (may be null): one event is
// appended after each launch, for the synchronous caller to wait on in turn.
template <class Launch>
int trace_launches(const rt_frame_setup &fs, const rt_params *prm, std::vector<hipEvent_t> *events, Launch launch) {
  RT_HIP(ensure_turn_table());
  const double frame_px = (double)prm->width * (double)prm->local_rows;
  return rt_sample_ranges(prm->spp, rt_samples_per_launch(prm->spp, frame_px, fs.launch_samples),
                          [&](int s_lo, int s_cnt) -> int {
                            launch(s_lo, s_cnt);
                            return trace_launched(fs, events);
                          });
}

// The synchronous form of a pass over explicit parts (rt_frame.h's
// rt_sync_pass): enqueue(fs, prm, dev, events) makes the launches into the
// parts' device addresses dev[0 .. N), and the pass is waited for launch by
// launch.
// trace_sync_in: in a scope the caller began (rt_trace's, without a camera),
// enqueue(fs, dev, events).
template <size_t N, class Enqueue>
int trace_sync_in(rt_pass_scope &ps, const rt_sync_part (&parts)[N], Enqueue enqueue, double *kernel_ms) {
  std::vector<hipEvent_t> events;
  const int r = rt_sync_pass_in(
      ps, parts, kernel_ms, [&](void *const *dev, const rt_frame_setup &fs) { return enqueue(fs, dev, &events); },
      [&]() -> int {
        // wait launch by launch: a fault surfaces after the launch it happened in
        for (hipEvent_t ev : events) RT_HIP(hipEventSynchronize(ev));
        return RT_OK;
      });
  for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
  return r;
}
template <size_t N, class Enqueue>
int trace_sync(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_sync_part (&parts)[N],
               Enqueue enqueue, double *kernel_ms) {
  rt_pass_scope ps(c, cam, prm, nullptr);
  return trace_sync_in(ps, parts,
                       [&](const rt_frame_setup &fs, void *const *dev, std::vector<hipEvent_t> *events) {
                         return enqueue(fs, prm, dev, events);
                       },
                       kernel_ms);
}

// One pass over N buffers (NULL = not wanted; none wanted: nothing to do), of
// px_bytes[k] bytes per pixel.  enqueue(fs, prm, ptrs, events) makes the launches
// (trace_launches) into the device pointers ptrs[0 .. N).  host false: the
// asynchronous form (bufs are device pointers, nothing waits).  Else bufs are
// host arrays; the pass runs through rt_sync_pass and is waited for launch by
// launch.  Whatever was enqueued, the pass ends with the context's ev_done
// recorded on its stream (rt_pass_scope).
template <size_t N, class Enqueue>
int trace_pass(rt_context *c, const rt_camera *cam, const rt_params *prm, void *const (&bufs)[N],
               const uint8_t (&px_bytes)[N], Enqueue enqueue, void *stream, bool host, double *kernel_ms) {
  bool wanted = false;
  for (void *b : bufs) wanted = wanted || b;
  if (!wanted) return RT_OK;
  const size_t npx = (size_t)prm->width * (size_t)prm->local_rows;
  if (!host || npx == 0) {
    rt_pass_scope ps(c, cam, prm, host ? nullptr : stream);
    return ps.end(ps.status != RT_OK || npx == 0 ? ps.status : enqueue(ps.fs, prm, bufs, nullptr));
  }
  rt_sync_part parts[N];
  for (size_t k = 0; k < N; ++k) parts[k] = {bufs[k] ? px_bytes[k] * npx : 0, nullptr, bufs[k]};
  return trace_sync(c, cam, prm, parts, enqueue, kernel_ms);
}

}  // namespace

#endif  // RTOW_RT_TRACE_PASS_H
