// rt_api.cpp -- the host half of the C ABI (include/rt.h): device contexts,
// scene upload, the render launches (pilot schedule, unit shares, bounded
// block- and sample-range launches), stats, the device tonemap and the diagnostics.
// Host C++ over the HIP runtime; the kernels and their launch wrappers live
// in rt_kernel.hip, the acceleration-structure builder in rt_accel.cpp.
//
// Replaces the host side of src/gpu/main.cu:86-156: new_world / new_camera
// (scene and camera reach the device by copy and by value), the one
// render<<<>>> launch (here: one or more bounded launches) and
// checkCudaErrors' exit(99) (status codes; the CLI maps them to exit 99).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "rt_internal.h"
#include "rt_accel.h"
#include "rt_frame.h"
#include "rt_layout.h"

extern "C" hipError_t rt_internal_block_order(const uint32_t *tile_cost, uint32_t blocks, uint32_t units,
                                              uint32_t *order, hipStream_t st);

// ------------------------------------------------------------ context ----
// Everything that belongs to the uploaded scene, freed with the record:
// rt_scene_upload fills one and moves it into the context.
struct scene_state {
  rtk::scene_dims dims;                      // the builder's facts (scene_kparams)
  rt_device_buf<rtk::pair_geom> d_geom;      // brute-force order
  rt_device_buf<rtk::pair_geom> d_bvh_geom;  // BVH leaf order
  rt_device_buf<rtk::bvh_node> d_nodes;
  rt_device_buf<int> d_orig;                 // BVH slot -> original index (-1 = padding)
  rt_device_buf<rtk::shade_rec> d_shade;
  rt_device_buf<uint32_t> d_grid_cells;  // layer grid (p nullptr: none)
  rt_device_buf<float> d_grid_items;     // 4 floats per item
  size_t grid_n_items = 0;
  int grid_placement = rtk::kGridGlobal;  // rtk::kGrid*: where a launch keeps the grid
  rtk::grid_dims grid;                    // of the grid in the buffers (scale NaN: of neither, after a failed copy)
  // the scene's largest lambertian / metal albedo: above 1, 64-bit pixel sums
  // (sum_format), with a 64-bit scratch frame for atomic renders
  double max_albedo = 0.0;
  // the layer grid's cell size fitted per frame geometry (rtk::grid_fitter,
  // DESIGN.md 3.3): the fitter, the geometry its grid was fitted for, and the
  // host copy the last refit uploads from (the context's ev_fit: after that copy)
  std::unique_ptr<rtk::grid_fitter> fitter;
  std::vector<uint64_t> fit_key;
  rtk::grid_geom fit_grid;
  bool fit_pending = false;
};

struct rt_context {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  scene_state sc;
  hipEvent_t ev_fit = nullptr;
  bool grid_fit = true;         // RT_OPT_GRID_FIT
  bool grid_scale_set = false;  // RT_OPT_GRID_SCALE given: no fitting
  rt_device_buf<unsigned long long> d_counters;
  rt_device_buf<float> d_frame;  // rt_render's frame (only it uses it, and it returns after its work is done)
  // block schedule from a pilot render, cached per frame geometry (stream-ordered allocation)
  uint32_t *d_order = nullptr;
  size_t order_n = 0;
  std::vector<uint64_t> order_key;
  uint64_t last_samples = 0;
  uint32_t last_launches = 0;  // launches since the counters were last zeroed
  uint32_t enq_launches = 0;   // launches of the last render_enqueue
  bool last_stats = false;
  // Renders of one context may be enqueued on different streams; they share
  // the scratch buffer above (block order), so each render first
  // waits for the previous one: ev_done is recorded after every render on
  // last_stream, and a render on another stream waits on it (no host sync).
  hipEvent_t ev_done = nullptr;
  hipStream_t last_stream = nullptr;
  bool have_done = false;
  // one event after each bounded launch of the last render: rt_render waits
  // on them in turn (a fault surfaces after the launch it happened in),
  // rt_render_progress queries them
  std::vector<hipEvent_t> ev_launch;
  double tonemap_thr64[257];  // rt_tonemap_async level thresholds (see tonemap_thresholds)
  float tonemap_thr32[257];
  rt_device_buf<double> d_thr64;
  rt_device_buf<float> d_thr32;
  rt_device_buf<uint64_t> d_wide;  // 64-bit scratch frame (sc.max_albedo above 1, atomic renders)
  // rt_context_set_option
  rtk::accel_options opt;
  double launch_samples = rtk::kLaunchSamples;
};

namespace {

// RT_OPT_GRID_PLACEMENT's values (0 = auto) as the builder's
constexpr int kPlacementOpt[4] = {-1, rtk::kGridLds, rtk::kGridCells, rtk::kGridGlobal};

// T[k] = the smallest q >= 0 whose correctly rounded square root reaches
// k / 256 (k = 1..255; T[0] unused), in fp64 and in fp32.  (k / 256)^2 is
// exact in both; step down while the square root still rounds up to k / 256.
void tonemap_thresholds(double *t64, float *t32) {
  t64[0] = 0.0;
  t32[0] = 0.0f;
  for (int k = 1; k < 256; ++k) {
    const double x = k / 256.0;
    double q = x * x;
    while (q > 0.0 && std::sqrt(std::nextafter(q, 0.0)) >= x) q = std::nextafter(q, 0.0);
    t64[k] = q;
    const float xf = (float)k / 256.0f;
    float qf = xf * xf;
    while (qf > 0.0f && std::sqrt(std::nextafter(qf, 0.0f)) >= xf) qf = std::nextafter(qf, 0.0f);
    t32[k] = qf;
  }
  t64[256] = INFINITY;
  t32[256] = INFINITY;
}

bool params_ok(const rt_params *p) {
  return p && p->width >= 1 && p->height >= 1 && p->spp >= 0 && p->spp < (1 << 24) &&
         p->max_depth >= 0 && p->max_depth < (1 << 24) &&
         p->row_block >= 1 && p->band_stride >= 1 && p->band_offset >= 0 &&
         p->band_offset < p->band_stride && p->local_rows >= 0 &&
         (uint64_t)p->width * (uint64_t)p->height < (1ull << 32);
}

// key += the camera's words
void append_camera(std::vector<uint64_t> &key, const rt_camera *cam) {
  const uint32_t *cw = reinterpret_cast<const uint32_t *>(cam);
  for (size_t k = 0; k < sizeof(rt_camera) / 4; ++k) key.push_back(cw[k]);
}

// (an empty vector still gets a buffer: a scene of no spheres is a scene)
template <class T>
hipError_t upload_vec(rt_device_buf<T> &dst, const std::vector<T> &v, hipStream_t st) {
  hipError_t e = dst.grow(v.empty() ? 1 : v.size());
  if (e == hipSuccess && !v.empty())
    e = hipMemcpyAsync(dst.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st);
  return e;
}

// F = 31 - floor(log2(spp)): spp samples of at most 2^F each fit a uint32
int sum_bits(int spp) {
  int f = 31;
  for (int s = spp; s > 1; s >>= 1) --f;
  return f;
}

// The pixel sums' format (the oracle restates it).
// Albedos in [0, 1]: a sample's radiance is at most 1; uint32 sums, F = 31 -
// floor(log2 spp).  An albedo A above 1 (the reference accepts any,
// src/cpu/material.h:17,38): radiance up to A^(max_depth - 1), so 64-bit sums
// with vcap = min(A^(max_depth - 1), 2^24) (rounded down to fp32), a sample's
// radiance clamped at vcap, and F = 62 - floor(log2 spp) - ceil(log2 vcap)
// (spp samples of at most vcap 2^F, +1 each for the dither, fit 64 bits; F >=
// 14).  A^(max_depth - 1) bounds the radiance in exact arithmetic; the fp32
// throughput can exceed it by a few ulps, so below 2^24 the clamp may trim a
// sample at the ulp level (the oracle clamps alike: same bits).  At vcap =
// 2^24 > spp a clamped sample alone makes its pixel's mean >= 1, white in
// either write_color; only the fp32 sums of such pixels saturate.
struct sum_fmt {
  bool wide;
  int f;
  float vcap;
};
sum_fmt sum_format(int spp, int max_depth, double max_albedo) {
  if (!(max_albedo > 1.0)) return {false, sum_bits(spp), 1.0f};
  double v = max_depth > 1 ? std::pow(max_albedo, (double)(max_depth - 1)) : 1.0;
  v = std::min(std::max(v, 1.0), 16777216.0);
  float vc = (float)v;
  if ((double)vc > v) vc = std::nextafter(vc, 0.0f);
  int e = 0;
  const double m = std::frexp((double)vc, &e);  // vc = m 2^e, m in [0.5, 1)
  const int ceil_log2 = m == 0.5 ? e - 1 : e;
  return {true, sum_bits(spp) + 31 - ceil_log2, vc};
}
// the format's kernel arguments
void sum_kparams(const sum_fmt &fmt, rtk::kparams &kp) {
  kp.qscale = std::ldexp(1.0f, fmt.f);
  kp.qinv = std::ldexp(1.0f, -fmt.f);
  kp.vcap = fmt.vcap;
  // F < 20 (spp >= 4096): truncation would bias a dark pixel by up to 2^-F per
  // sample (0.03 level at F = 20); stochastic rounding is unbiased for every
  // spp
  kp.dither = fmt.f < 20 ? 1 : 0;
}

}  // namespace

extern "C" {

int rt_device_count(int *count) {
  if (!count) return RT_ERR_INVALID;
  hipError_t e = hipGetDeviceCount(count);
  if (e == hipErrorNoDevice) {
    *count = 0;
    return RT_OK;
  }
  if (e != hipSuccess) return hip_fail(e);
  return RT_OK;
}

int rt_context_create(int device_ordinal, rt_context **out) {
  if (!out) return RT_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || device_ordinal < 0 || device_ordinal >= n) {
    if (e != hipSuccess) rt_internal_set_hip_error((int)e);
    return RT_ERR_NO_DEVICE;
  }
  rt_context *c = new (std::nothrow) rt_context();
  if (!c) return RT_ERR_NOMEM;
  c->device = device_ordinal;
  int st = RT_OK;
  do {
    if ((e = hipSetDevice(device_ordinal)) != hipSuccess) break;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) break;
    if ((e = hipEventCreate(&c->ev0)) != hipSuccess) break;
    if ((e = hipEventCreate(&c->ev1)) != hipSuccess) break;
    if ((e = hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming)) != hipSuccess) break;
    if ((e = c->d_counters.grow(8 * rtk::kCounterSlots)) != hipSuccess) break;
    tonemap_thresholds(c->tonemap_thr64, c->tonemap_thr32);
    if ((e = c->d_thr64.grow(257)) != hipSuccess) break;
    if ((e = c->d_thr32.grow(257)) != hipSuccess) break;
    if ((e = hipMemcpy(c->d_thr64.p, c->tonemap_thr64, sizeof c->tonemap_thr64, hipMemcpyHostToDevice)) != hipSuccess) break;
    if ((e = hipMemcpy(c->d_thr32.p, c->tonemap_thr32, sizeof c->tonemap_thr32, hipMemcpyHostToDevice)) != hipSuccess) break;
    if ((e = rtk::upload_turn_table()) != hipSuccess) break;
  } while (0);
  if (e != hipSuccess) {
    st = hip_fail(e);
    rt_context_destroy(c);
    return st;
  }
  *out = c;
  return RT_OK;
}

void rt_context_destroy(rt_context *c) {
  if (!c) return;
  if (c->device >= 0) {
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();  // renders on caller streams may still use the buffers
  }
  (void)hipFree(c->d_order);
  for (hipEvent_t ev : c->ev_launch) (void)hipEventDestroy(ev);
  if (c->ev_done) (void)hipEventDestroy(c->ev_done);
  if (c->ev_fit) (void)hipEventDestroy(c->ev_fit);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;  // (frees the buffers the context and its scene own)
}

int rt_context_set_option(rt_context *c, int option, double v) {
  if (!c || !std::isfinite(v)) return RT_ERR_INVALID;
  const bool dflt = v == 0.0;
  switch (option) {
    case RT_OPT_GRID_PLACEMENT:
      if (v != std::floor(v) || v < 0 || v > 3) return RT_ERR_INVALID;
      c->opt.grid_placement = kPlacementOpt[(int)v];
      return RT_OK;
    case RT_OPT_GRID_SCALE:
      if (!dflt && !(v >= 0.05 && v <= 20.0)) return RT_ERR_INVALID;
      c->opt.grid_scale = dflt ? 1.0 : v;
      c->grid_scale_set = !dflt;
      return RT_OK;
    case RT_OPT_GRID_FIT:
      if (v != 0.0 && v != 1.0) return RT_ERR_INVALID;
      c->grid_fit = v != 0.0;
      return RT_OK;
    case RT_OPT_INTERNAL_GRID_PHASE_X:
    case RT_OPT_INTERNAL_GRID_PHASE_Z:
      if (!(v >= 0.0 && v < 1.0)) return RT_ERR_INVALID;
      (option == RT_OPT_INTERNAL_GRID_PHASE_X ? c->opt.grid_phase_x : c->opt.grid_phase_z) = v;
      return RT_OK;
    case RT_OPT_BVH_LEAF:
      if (v != std::floor(v) || v < 0 || v > 4) return RT_ERR_INVALID;
      c->opt.bvh_leaf = dflt ? 4 : (int)v;
      return RT_OK;
    case RT_OPT_BVH_COLLAPSE:
      if (!dflt && !(v > 0.0 && v <= 100.0)) return RT_ERR_INVALID;
      c->opt.collapse = dflt ? 0.35 : v;
      return RT_OK;
    case RT_OPT_BVH_SIDE:
      if (!dflt && !(v > 0.0 && v <= 100.0)) return RT_ERR_INVALID;
      c->opt.side = dflt ? 1.0 : v;
      return RT_OK;
    case RT_OPT_LAUNCH_SAMPLES:
      if (!dflt && !(v >= 1.0)) return RT_ERR_INVALID;
      c->launch_samples = dflt ? rtk::kLaunchSamples : std::floor(v);
      return RT_OK;
    default:
      return RT_ERR_INVALID;
  }
}

int rt_scene_upload(rt_context *c, const rt_scene_view *s) {
  if (!c || !rtk::scene_ok(s)) return RT_ERR_INVALID;
  rtk::accel_build a;
  rtk::accel_options o = c->opt;
  o.wide = rtk::max_albedo(s) > 1.0;
  scene_state sc;  // becomes the context's once its copies have completed
  rtk::grid_fitter *fitter = nullptr;
  rtk::build_accel(s, o, a, c->grid_fit && !c->grid_scale_set ? &fitter : nullptr);
  sc.fitter.reset(fitter);
  sc.dims = a;
  sc.max_albedo = rtk::max_albedo(s);
  sc.grid = a.grid;

  // renders enqueued on caller streams may still read the old scene: they
  // are serialised and each ends by recording ev_done, so the last one's
  // event covers them all (this context's work only, not the whole device)
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess && c->have_done) e = hipEventSynchronize(c->ev_done);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hip_fail(e);  // (the old scene stays)
  c->sc = scene_state{};                    // frees the old scene before the new one is allocated
  c->order_key.clear();                     // the pilot's tile costs belong to the old scene
  e = upload_vec(sc.d_geom, a.scan_geom, c->stream);
  if (e == hipSuccess) e = upload_vec(sc.d_bvh_geom, a.bvh_geom, c->stream);
  if (e == hipSuccess) e = upload_vec(sc.d_nodes, a.nodes, c->stream);
  if (e == hipSuccess) e = upload_vec(sc.d_orig, a.slots, c->stream);
  if (e == hipSuccess) e = upload_vec(sc.d_shade, a.shade, c->stream);
  if (e == hipSuccess && !a.grid.cells.empty()) {
    e = upload_vec(sc.d_grid_cells, a.grid.cells, c->stream);
    if (e == hipSuccess) e = upload_vec(sc.d_grid_items, a.grid.items, c->stream);
    sc.grid_n_items = a.grid.items.size() / 4;
    sc.grid_placement = a.grid_placement;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return hip_fail(e);  // (no scene)
  c->sc = std::move(sc);
  return RT_OK;
}

}  // extern "C"

namespace {

// Local rows that lie inside the frame: a rank's last band slots may be
// padding (global row >= height), which the kernel leaves at zero untraced.
uint64_t valid_rows(const rt_params *prm) {
  uint64_t n = 0;
  for (int r0 = 0; r0 < prm->local_rows; r0 += prm->row_block) {
    const long long g0 = ((long long)(r0 / prm->row_block) * prm->band_stride + prm->band_offset) *
                         (long long)prm->row_block;
    const long long in_band = std::min<long long>(prm->row_block, prm->local_rows - r0);
    n += (uint64_t)std::max<long long>(0, std::min<long long>(in_band, prm->height - g0));
  }
  return n;
}

// the kernel arguments of the scene's layer grid in device memory (the one place
// that knows both spellings of its geometry, rtk::grid_dims' and rtk::kparams')
void grid_kparams(const scene_state &s, rtk::kparams &kp) {
  const rtk::grid_dims &g = s.grid;
  kp.grid_cells = s.d_grid_cells.p;
  kp.grid_items = (const rtk::f4 *)s.d_grid_items.p;
  kp.grid_n_items = (int)s.grid_n_items;
  kp.grid_n_cells = g.nx * g.nz;
  kp.grid_x0 = g.x0;
  kp.grid_xi = g.xi;
  kp.grid_zi = g.zi;
  kp.grid_z0 = g.z0;
  kp.grid_x1 = g.x1;
  kp.grid_z1 = g.z1;
  kp.grid_g = g.g;
  kp.grid_invg = g.g > 0.0f ? 1.0f / g.g : 0.0f;
  kp.grid_nx = g.nx;
  kp.grid_nz = g.nz;
}

// the kernel arguments of a built scene in device memory (the one place that
// knows both spellings of its facts, rtk::scene_dims' and rtk::kparams')
void scene_kparams(const scene_state &s, rtk::kparams &kp) {
  const rtk::scene_dims &d = s.dims;
  kp.n_pad = (int)d.n_pad;
  kp.n_nodes = (int)(uint32_t)d.per_order;  // nodes holds 8 orders of this many
  kp.oref2 = (float)(0.99 * d.oref * d.oref);
  kp.layer = rtk::f2{d.layer_lo, d.layer_hi};
  kp.layer_mode = d.layer_mode ? 1 : 0;
  kp.layer_cy = d.layer_cy;
  kp.extra_pair0 = (int)d.extra_pair0;
  kp.n_extra_pairs = (int)d.n_extra_pairs;
  kp.extras_fold = d.extras_fold;
  kp.extras_cy = d.extras_cy;
  kp.scan_geom = s.d_geom.p;
  kp.geom = s.d_bvh_geom.p;
  kp.nodes = s.d_nodes.p;
  kp.orig = s.d_orig.p;
  kp.extra_geom = s.d_bvh_geom.p ? s.d_bvh_geom.p + d.extra_pair0 : nullptr;
  kp.extra_orig = s.d_orig.p ? s.d_orig.p + 2 * (size_t)d.extra_pair0 : nullptr;
  kp.shade = s.d_shade.p;
}

// The kernel arguments of a render of (cam, prm) into accum_rgb with the
// context's scene and current grid (launch ranges, units and the sum format
// are set by the caller)
void fill_kparams(const rt_context *c, const rt_camera *cam, const rt_params *prm, float *accum_rgb,
                  rtk::kparams &kp) {
  std::memset(&kp, 0, sizeof kp);
  kp.block_stride = 1;  // entry = blockIdx.x (the pilot; the launches below set their ranges)
  kp.cam = *cam;
  kp.width = prm->width;
  kp.height = prm->height;
  kp.spp = prm->spp;
  kp.max_depth = prm->max_depth;
  kp.row_block = prm->row_block;
  kp.band_stride = prm->band_stride;
  kp.band_offset = prm->band_offset;
  kp.local_rows = prm->local_rows;
  kp.tiles_x = (prm->width + rtk::kTile - 1) / rtk::kTile;
  scene_kparams(c->sc, kp);
  grid_kparams(c->sc, kp);
  kp.seed32 = rt_seed32(prm->seed);
  kp.flags = prm->flags;
  kp.inv_wm1 = (float)(1.0 / (prm->width - 1));
  kp.inv_hm1 = (float)(1.0 / (prm->height - 1));
  kp.out = accum_rgb;
  kp.counters = c->d_counters.p;
  {
    uint32_t w = (uint32_t)prm->width, sh = 0;
    while (!(w & 1u)) {
      w >>= 1;
      ++sh;
    }
    uint32_t inv = w;  // Newton: inv = inv (2 - w inv) doubles the correct low bits
    for (int k = 0; k < 5; ++k) inv *= 2u - w * inv;
    kp.wshift = sh;
    kp.winv = inv;
  }
}

// render_kernel variant bits of a render (rt_layout.h kVar*); whether it walks
// the layer grid, and where that lives, are frame_begin's decisions
int render_variant(const rt_frame_setup &fs, const rt_params *prm, bool wide) {
  // the extras' folded forms exist in the grid builds only (rt_kernel.hip launch_variant)
  const int fold = fs.grid && (prm->flags & RT_FLAG_ACCEL_BVH) ? fs.kp.extras_fold : 0;
  return (fold << rtk::kVarFoldShift) | (wide ? rtk::kVarWide : 0) | ((prm->flags & RT_FLAG_OPEN_INTERVAL) ? rtk::kVarOpen : 0) |
         ((prm->flags & RT_FLAG_METAL_UNIT_VECTOR) ? rtk::kVarMetalUnit : 0) |
         ((prm->flags & RT_FLAG_ACCEL_BVH) ? rtk::kVarBvh : 0) |
         ((prm->flags & RT_FLAG_COUNT_WORK) ? rtk::kVarStats : 0) | (fs.grid ? rtk::kVarGrid : 0) |
         (fs.placement << rtk::kVarPlaceShift);
}

// How a render is cut into launches (render_enqueue; rt_internal_launch_plan
// shows it on the host).
struct launch_plan {
  long long units, ranges, chunks, entries;
};
launch_plan plan_launches(const rt_params *prm, double launch_samples) {
  const long long tiles = rt_frame_tiles(prm), blocks = rt_frame_blocks(prm);
  const bool traced = prm->spp > 0 && prm->max_depth > 0;
  const double frame_px = (double)prm->width * (double)prm->local_rows;
  const double total = traced ? frame_px * prm->spp : 0.0;
  const double budget = std::max(launch_samples, total / (double)rtk::kMaxLaunches);
  // How many waves share a tile's samples (even shares; the integer pixel
  // sums make any split give the same image).  One wave per tile traces all
  // of its tile's samples; when a rank holds few tiles (a 1/8 share of a 4K
  // frame is ~2 waves per wave slot), the slowest tiles (long glass / metal
  // paths) then set the frame time, so the samples are split over `units`
  // waves (tools/rank_times.py).
  long long units = prm->units;
  if (units <= 0) {
    const bool pilot = (prm->flags & RT_FLAG_PILOT_SCHEDULE) != 0;
    units = pilot ? std::llround((double)rtk::kPilotTilesPerUnit / (double)std::max(1LL, tiles))
                  : (tiles < rtk::kSplitTiles ? rtk::kUnits : 1);
    units = std::min<long long>(std::max(units, 1LL), rtk::kUnits);
  }
  if (!traced) units = 1;  // nothing is traced
  units = std::max(1LL, std::min<long long>(units, prm->spp));  // >= 1 sample per unit
  // Bounded launches: about `budget` samples per launch at most.
  // The plain split is by samples: `chunks` launches over every work entry
  // (a block of 4 tiles and a unit's share of their samples), each tracing
  // spp / chunks samples per pixel.  That keeps the launches wide (their
  // tails short) but shortens each wave's sample pool, whose own tail idles
  // lanes: ~2.2 / s of them at s samples per pixel per wave (lane efficiency
  // 0.995 at 500, 0.981 at 125, 0.861 at 16: C4's full frame on one GPU,
  // profiles/r03n_bench_c4.log).  Below kMinPoolSpp the work entries are
  // split too, into `ranges` strided subsets (range r runs entries r, r +
  // ranges, ... of block_order, so every launch keeps the expensive-first
  // order over a mix of the frame), and the samples into fewer, longer
  // chunks of about kPoolSpp per wave.  (Contiguous entry ranges lost 6 % on
  // C3's full frame to their launch tails,
  // profiles/r03o_contiguous_ranges_bench_c3.log.)  The
  // integer pixel sums make every split give the same image.
  long long entries = (long long)blocks * units;
  long long ranges = 1, chunks = 1;
  if (total > budget) {
    chunks = std::min<long long>(prm->spp, (long long)std::ceil(total / budget));
    const long long u1 = std::max(1LL, std::min<long long>(units, prm->spp / chunks));
    if ((double)prm->spp / (double)(u1 * chunks) >= rtk::kMinPoolSpp) {
      units = u1;
    } else {
      chunks = std::max(1LL, (long long)std::floor((double)prm->spp / ((double)units * rtk::kPoolSpp)));
      units = std::max(1LL, std::min<long long>(units, prm->spp / chunks));
      entries = (long long)blocks * units;
      ranges = std::min<long long>(entries, (long long)std::ceil(total / ((double)chunks * budget)));
      // entries too few for the budget: more sample ranges
      if (total / ((double)ranges * (double)chunks) > budget)
        chunks = std::min<long long>(prm->spp, (long long)std::ceil(total / ((double)ranges * budget)));
      units = std::max(1LL, std::min<long long>(units, prm->spp / chunks));
      entries = (long long)blocks * units;
      ranges = std::max(1LL, std::min({ranges, entries, rtk::kMaxLaunches / chunks}));
    }
  }
  return launch_plan{units, ranges, chunks, entries};
}

// What every pass over the context's scene does before its launches
// (rt_internal_frame_begin: the render below and librtow_aov.so's first-hit
// pass): the device, the wait on the context's previous pass, the kernel
// arguments and the layer grid's refit for this frame geometry.
// (pass_begin alone, rt_internal_pass_begin: a pass that reads no scene,
// librtow_denoise.so's filter)
int pass_begin(rt_context *c, hipStream_t st, rt_frame_setup &fs) {
  std::memset(&fs, 0, sizeof fs);
  fs.stream = st;
  fs.placement = rtk::kGridGlobal;
  fs.launch_samples = c->launch_samples;
  fs.ev0 = c->ev0;
  fs.ev1 = c->ev1;
  RT_HIP(hipSetDevice(c->device));
  // passes of one context are serialised, whatever streams they come on:
  // they share the block-order scratch buffer and the grid's buffers
  if (c->have_done && c->last_stream != st) RT_HIP(hipStreamWaitEvent(st, c->ev_done, 0));
  return RT_OK;
}

// The layer grid's cell size for this frame geometry (rtk::grid_fitter: a
// host-side model, once per geometry; the image is the same for every size).
// The new grid is copied into the context's buffers on st, after every
// earlier render (renders of one context are serialised), and written to kp.
int refit_grid(rt_context *c, const rt_camera *cam, const rt_params *prm, hipStream_t st, rtk::kparams &kp) {
  scene_state &s = c->sc;
  std::vector<uint64_t> key = {(uint64_t)prm->width, (uint64_t)prm->height};
  append_camera(key, cam);
  if (key == s.fit_key) return RT_OK;
  const double scale = s.fitter->choose(*cam, prm->width, prm->height, nullptr);
  if (scale != s.grid.scale) {
    if (s.fit_pending) RT_HIP(hipEventSynchronize(c->ev_fit));  // fit_grid is still being read
    s.fit_pending = false;
    rtk::grid_geom &q = s.fit_grid;
    if (!s.fitter->build(scale, q)) return RT_ERR_INVALID;  // (every candidate fits: unreachable)
    // Transactional: larger buffers are allocated before the
    // old ones are freed, so a failed allocation leaves the old grid whole
    // (buffers, fields and fit_key describe it); once a copy into the
    // buffers has failed they hold neither grid, and grid_scale = NaN makes
    // the next grid render refit before it launches.
    if (q.cells.size() > s.d_grid_cells.cap || q.items.size() > s.d_grid_items.cap) {
      rt_device_buf<uint32_t> cells;
      rt_device_buf<float> items;
      hipError_t ea = cells.grow(q.cells.size());
      if (ea == hipSuccess) ea = items.grow(q.items.size());
      if (ea == hipSuccess) ea = hipStreamSynchronize(st);  // earlier renders on st still read the old grid
      if (ea != hipSuccess) return hip_fail(ea);
      s.d_grid_cells = std::move(cells);  // (the old buffers are freed with these two)
      s.d_grid_items = std::move(items);
    }
    s.grid.scale = std::numeric_limits<double>::quiet_NaN();
    s.fit_key.clear();
    RT_HIP(hipMemcpyAsync(s.d_grid_cells.p, q.cells.data(), q.cells.size() * sizeof(uint32_t),
                          hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(s.d_grid_items.p, q.items.data(), q.items.size() * sizeof(float), hipMemcpyHostToDevice,
                          st));
    if (!c->ev_fit) RT_HIP(hipEventCreateWithFlags(&c->ev_fit, hipEventDisableTiming));
    RT_HIP(hipEventRecord(c->ev_fit, st));
    s.fit_pending = true;
    s.grid_n_items = q.items.size() / 4;
    s.grid = q;
    grid_kparams(s, kp);
  }
  s.fit_key = key;
  return RT_OK;
}

int frame_begin(rt_context *c, const rt_camera *cam, const rt_params *prm, hipStream_t st, rt_frame_setup &fs) {
  {
    const int r = pass_begin(c, st, fs);
    if (r != RT_OK) return r;
  }
  if (prm->width == 0 || prm->local_rows == 0) return RT_OK;  // nothing to launch
  rtk::kparams &kp = fs.kp;
  fill_kparams(c, cam, prm, nullptr, kp);
  const scene_state &s = c->sc;
  fs.n_spheres = (uint32_t)s.dims.n;
  // whether this pass walks the layer grid is decided here alone (fs.grid, fs.placement)
  const bool grid = s.d_grid_cells.p && !(prm->flags & RT_FLAG_LAYER_BVH);
  if (grid && s.fitter && (prm->flags & RT_FLAG_ACCEL_BVH)) {
    const int r = refit_grid(c, cam, prm, st, kp);
    if (r != RT_OK) return r;
  }
  fs.grid = grid ? 1 : 0;
  fs.placement = grid ? s.grid_placement : rtk::kGridGlobal;
  fs.lds_bytes = rtk::grid_lds_bytes(fs.placement, kp.grid_n_items, kp.grid_n_cells);
  return RT_OK;
}

// frame_begin without a camera (rt_internal_scene_begin: librtow_trace.so's
// pass over the caller's rays): the scene's and the current grid's kernel
// arguments, the camera and frame fields left zero; no frame geometry, so no
// refit -- the pass walks the grid the context holds.
int scene_begin(rt_context *c, uint32_t flags, hipStream_t st, rt_frame_setup &fs) {
  {
    const int r = pass_begin(c, st, fs);
    if (r != RT_OK) return r;
  }
  rtk::kparams &kp = fs.kp;
  const scene_state &s = c->sc;
  scene_kparams(s, kp);
  grid_kparams(s, kp);
  kp.flags = flags;
  fs.n_spheres = (uint32_t)s.dims.n;
  // refit_grid leaves grid.scale = NaN when a copy into the grid's buffers
  // failed: they hold neither grid until the next grid render refits, and
  // nothing refits here, so the pass walks the layer BVH (the same bits)
  const bool grid = s.d_grid_cells.p && !(flags & RT_FLAG_LAYER_BVH) && !std::isnan(s.grid.scale);
  fs.grid = grid ? 1 : 0;
  fs.placement = grid ? s.grid_placement : rtk::kGridGlobal;
  fs.lds_bytes = rtk::grid_lds_bytes(fs.placement, kp.grid_n_items, kp.grid_n_cells);
  return RT_OK;
}

// Expensive tiles first (RT_FLAG_PILOT_SCHEDULE): a 4-spp pilot (same
// geometry, one wave per tile, the instrumented build that reports each
// tile's segments) runs once per frame geometry; blocks are then launched
// in decreasing cost of their tiles (longest-processing-time first), the
// units of a tile group adjacent.  Without it the hardware launches
// blocks in index order and the last wave slots to fill may get the most
// expensive tiles.  Scheduling only: the image does not depend on it.
// Everything stays on st (the sort runs on the device, rt_sched.hip).
// kp, v: the render's arguments and variant; *order = the context's block order.
// sink (rt_internal_pilot_schedule; null otherwise): told whether the pilot
// ran, and given its tile costs before they are freed.
struct pilot_sink {
  uint32_t *tile_cost = nullptr;  // host, n_cost entries
  size_t n_cost = 0;
  bool ran = false;   // the pilot ran (no cached order for this geometry)
  bool used = false;  // the render reads the context's order
};
hipError_t pilot_order(rt_context *c, const rt_camera *cam, const rt_params *prm, const rtk::kparams &kp, int v,
                       unsigned blocks, long long units, hipStream_t st, const uint32_t **order,
                       pilot_sink *sink = nullptr) {
  std::vector<uint64_t> key = {(uint64_t)prm->width, (uint64_t)prm->height, (uint64_t)prm->local_rows,
                               (uint64_t)prm->row_block, (uint64_t)prm->band_stride,
                               (uint64_t)prm->band_offset, (uint64_t)units, (uint64_t)(prm->flags & 0x12ffu)};
  append_camera(key, cam);
  if (key != c->order_key || c->order_n != (size_t)blocks * units) {
    c->order_key.clear();  // valid again only once the new order is enqueued
    // tile costs, then 8 scratch counters (the context's are not touched)
    const size_t n_cost = (size_t)blocks * rtk::kWavesPerBlock;
    const size_t cost_bytes = (n_cost * sizeof(uint32_t) + 7) / 8 * 8;
    uint32_t *d_cost = nullptr;
    hipError_t e = hipMallocAsync((void **)&d_cost, cost_bytes + 8 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d_cost, 0, cost_bytes + 8 * sizeof(unsigned long long), st);
    if (e == hipSuccess) {
      // the instrumented build with the grid in global memory, 4 samples,
      // one unit, float stores
      rtk::kparams pk = kp;
      pk.s_lo = 0;
      pk.s_cnt = std::min(prm->spp, 4);
      pk.units = 1;
      pk.sum_atomic = 0;
      pk.tile_cost = d_cost;
      pk.counters = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(d_cost) + cost_bytes);
      e = rtk::launch_render((v & ~(3 << rtk::kVarPlaceShift)) | rtk::kVarStats, blocks, 0, st, pk);
    }
    if (e == hipSuccess && c->d_order) e = hipFreeAsync(c->d_order, st);
    if (e == hipSuccess) {
      c->d_order = nullptr;
      c->order_n = 0;
      e = hipMallocAsync((void **)&c->d_order, (size_t)blocks * units * sizeof(uint32_t), st);
    }
    if (e == hipSuccess) e = rt_internal_block_order(d_cost, blocks, (uint32_t)units, c->d_order, st);
    if (e == hipSuccess && sink) {
      sink->ran = true;
      if (sink->tile_cost && sink->n_cost)
        e = hipMemcpyAsync(sink->tile_cost, d_cost, std::min(sink->n_cost, n_cost) * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, st);
    }
    (void)hipFreeAsync(d_cost, st);  // also on error: no leak
    if (e != hipSuccess) return e;
    c->order_n = (size_t)blocks * units;
    c->order_key = key;
  }
  *order = c->d_order;
  if (sink) sink->used = true;
  return hipSuccess;
}

// Where the launches leave a pixel's sum.  One launch and one unit per tile:
// float stores into the caller's frame.  Several units or launches per tile add
// their integer sums into a zeroed frame, which finish_sums converts at the end:
// the caller's, or, for 64-bit sums, which do not fit its fp32 frame, a scratch
// frame of the context's (renders of one context are serialised).
enum sum_target { kSumStore, kSumAtomic, kSumAtomicWide };

hipError_t begin_sums(rt_context *c, sum_target t, float *accum_rgb, uint64_t frame_floats, hipStream_t st,
                      rtk::kparams &kp) {
  if (t == kSumStore) return hipSuccess;
  if (t == kSumAtomic) return hipMemsetAsync(accum_rgb, 0, frame_floats * sizeof(float), st);
  hipError_t e = c->d_wide.grow(frame_floats);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_wide.p, 0, frame_floats * sizeof(uint64_t), st);
  if (e == hipSuccess) kp.out = reinterpret_cast<float *>(c->d_wide.p);
  return e;
}

hipError_t end_sums(rt_context *c, sum_target t, float *accum_rgb, uint64_t frame_floats, float qinv,
                    hipStream_t st) {
  if (t == kSumStore) return hipSuccess;
  if (t == kSumAtomic) return rtk::launch_finish_sums(reinterpret_cast<uint32_t *>(accum_rgb), frame_floats, qinv, st);
  return rtk::launch_finish_sums_wide(c->d_wide.p, accum_rgb, frame_floats, qinv, st);
}

// rt_render_async's body (stream NULL: the context's own).  ev_start (may be
// null) is recorded on the stream just before the render kernel itself, after
// any one-time setup (the pilot, buffer growth), so that rt_render's kernel_ms
// times the render alone.  A render that fails after enqueuing some of its
// work (a refit copy, the pilot, the k-th launch) still ends with ev_done
// recorded behind that work (rt_pass_scope; ADVICE r5: before, only hipFree's
// implicit device synchronisation covered it).
int render_enqueue(rt_context *c, const rt_camera *cam, const rt_params *prm, float *accum_rgb, void *stream,
                   hipEvent_t ev_start, pilot_sink *sink = nullptr) {
  rt_pass_scope ps(c, cam, prm, stream);
  if (ps.status != RT_OK) return ps.status;
  rt_frame_setup &fs = ps.fs;
  const hipStream_t st = fs.stream;
  const uint64_t samples = (uint64_t)prm->width * valid_rows(prm) * (uint64_t)prm->spp;
  if (prm->flags & RT_FLAG_KEEP_COUNTERS) {
    c->last_samples += samples;
  } else {
    RT_HIP(hipMemsetAsync(c->d_counters.p, 0, 8 * rtk::kCounterSlots * sizeof(unsigned long long), st));
    c->last_samples = samples;
    c->last_launches = 0;
  }
  c->last_stats = (prm->flags & RT_FLAG_COUNT_WORK) != 0;
  c->enq_launches = 0;
  if (prm->width == 0 || prm->local_rows == 0) {
    if (ev_start) RT_HIP(hipEventRecord(ev_start, st));
    return RT_OK;
  }

  rtk::kparams &kp = fs.kp;
  kp.out = accum_rgb;
  const unsigned blocks = (unsigned)rt_frame_blocks(prm);
  const sum_fmt fmt = sum_format(prm->spp, prm->max_depth, c->sc.max_albedo);
  sum_kparams(fmt, kp);
  const int v = render_variant(fs, prm, fmt.wide);
  const bool traced = prm->spp > 0 && prm->max_depth > 0;
  const launch_plan lp = plan_launches(prm, c->launch_samples);
  const long long launches = lp.ranges * lp.chunks;
  kp.units = (int)lp.units;
  // disjoint block ranges write disjoint pixels: float stores suffice
  const sum_target sums = !(lp.units > 1 || lp.chunks > 1) ? kSumStore : fmt.wide ? kSumAtomicWide : kSumAtomic;
  kp.sum_atomic = sums != kSumStore ? 1 : 0;
  const uint64_t frame_floats = (uint64_t)prm->local_rows * (uint64_t)prm->width * 3u;
  if ((prm->flags & RT_FLAG_PILOT_SCHEDULE) && traced && blocks > 1)
    RT_HIP(pilot_order(c, cam, prm, kp, v, blocks, lp.units, st, &kp.block_order, sink));
  RT_HIP(begin_sums(c, sums, accum_rgb, frame_floats, st, kp));  // (after the pilot, which renders into accum_rgb too)
  while (c->ev_launch.size() < (size_t)launches) {  // one event per bounded launch (the pool only grows)
    hipEvent_t ev = nullptr;
    RT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    c->ev_launch.push_back(ev);
  }
  if (ev_start) RT_HIP(hipEventRecord(ev_start, st));
  long long k = 0;
  kp.block_stride = (int)lp.ranges;
  for (long long r = 0; r < lp.ranges; ++r) {
    // entries r, r + ranges, r + 2 ranges, ... in block_order's order (most
    // expensive first with the pilot)
    kp.block_base = (int)r;
    const long long n_r = (lp.entries - r + lp.ranges - 1) / lp.ranges;
    for (long long ch = 0; ch < lp.chunks; ++ch, ++k) {
      const long long s0 = ch * prm->spp / lp.chunks, s1 = (ch + 1) * prm->spp / lp.chunks;
      kp.s_lo = (int)s0;
      kp.s_cnt = (int)(s1 - s0);
      // a launch that cannot start (bad configuration, lost device) stops the render here
      RT_HIP(rtk::launch_render(v, (unsigned)n_r, fs.lds_bytes, st, kp));
      RT_HIP(hipEventRecord(c->ev_launch[(size_t)k], st));
    }
  }
  c->last_launches += (uint32_t)launches;
  c->enq_launches = (uint32_t)launches;
  RT_HIP(end_sums(c, sums, accum_rgb, frame_floats, kp.qinv, st));
  return ps.end(RT_OK);
}

}  // namespace

extern "C" {

int rt_internal_frame_check(const rt_context *c, const rt_camera *cam, const rt_params *prm) {
  if (!c || !cam || !params_ok(prm)) return RT_ERR_INVALID;
  if (cam->model != RT_CAMERA_CPU && cam->model != RT_CAMERA_GPU) return RT_ERR_INVALID;
  if (cam->model == RT_CAMERA_CPU && (prm->width < 2 || prm->height < 2)) return RT_ERR_INVALID;
  if (!c->sc.d_geom.p) return RT_ERR_NO_SCENE;
  return RT_OK;
}

int rt_internal_frame_begin(rt_context *c, const rt_camera *cam, const rt_params *prm, void *stream,
                            rt_frame_setup *out) {
  if (!out) return RT_ERR_INVALID;
  const int r = rt_internal_frame_check(c, cam, prm);
  if (r != RT_OK) return r;
  return frame_begin(c, cam, prm, stream ? (hipStream_t)stream : c->stream, *out);
}

int rt_internal_scene_check(const rt_context *c) {
  if (!c) return RT_ERR_INVALID;
  return c->sc.d_geom.p ? RT_OK : RT_ERR_NO_SCENE;
}

int rt_internal_scene_begin(rt_context *c, uint32_t flags, void *stream, rt_frame_setup *out) {
  if (!out) return RT_ERR_INVALID;
  const int r = rt_internal_scene_check(c);
  if (r != RT_OK) return r;
  return scene_begin(c, flags, stream ? (hipStream_t)stream : c->stream, *out);
}

int rt_internal_pass_begin(rt_context *c, void *stream, rt_frame_setup *out) {
  if (!c || !out) return RT_ERR_INVALID;
  return pass_begin(c, stream ? (hipStream_t)stream : c->stream, *out);
}

int rt_internal_frame_end(rt_context *c, hipStream_t stream) {
  if (!c || !c->ev_done) return RT_ERR_INVALID;
  RT_HIP(hipEventRecord(c->ev_done, stream));
  c->last_stream = stream;
  c->have_done = true;
  return RT_OK;
}

int rt_render_async(rt_context *c, const rt_camera *cam, const rt_params *prm, float *accum_rgb,
                    void *stream) {
  if (!c || !cam || !params_ok(prm) || (!accum_rgb && prm->local_rows && prm->width))
    return RT_ERR_INVALID;
  return render_enqueue(c, cam, prm, accum_rgb, stream, nullptr);  // (rt_internal_frame_check first)
}

int rt_render_progress(rt_context *c, uint32_t *done, uint32_t *total) {
  if (!c || !done || !total) return RT_ERR_INVALID;
  const uint32_t n = std::min<uint32_t>(c->enq_launches, (uint32_t)c->ev_launch.size());
  *total = n;
  *done = 0;
  RT_HIP(hipSetDevice(c->device));
  // launches complete in order on their stream: count the leading finished ones
  for (uint32_t k = 0; k < n; ++k) {
    const hipError_t e = hipEventQuery(c->ev_launch[k]);
    if (e == hipErrorNotReady) break;
    if (e != hipSuccess) return hip_fail(e);  // a fault in or before launch k
    ++*done;
  }
  return RT_OK;
}

int rt_reset_stats(rt_context *c, void *stream) {
  if (!c) return RT_ERR_INVALID;
  RT_HIP(hipSetDevice(c->device));
  RT_HIP(hipMemsetAsync(c->d_counters.p, 0, 8 * rtk::kCounterSlots * sizeof(unsigned long long),
                        stream ? (hipStream_t)stream : c->stream));
  c->last_samples = 0;
  c->last_launches = 0;
  return RT_OK;
}

int rt_collect_stats(rt_context *c, rt_stats *stats) {
  if (!c || !stats) return RT_ERR_INVALID;
  unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hs[8 * rtk::kCounterSlots];
  RT_HIP(hipSetDevice(c->device));
  RT_HIP(hipMemcpy(hs, c->d_counters.p, sizeof hs, hipMemcpyDeviceToHost));
  for (int i = 0; i < 8 * rtk::kCounterSlots; ++i) h[i & 7] += hs[i];
  stats->segments = h[0];
  stats->wave_steps = h[1];
  stats->samples = c->last_samples;
  stats->bf_tests = h[0] * (uint64_t)c->sc.dims.n;
  stats->sphere_tests = c->last_stats ? h[2] : 0;
  stats->box_tests = c->last_stats ? h[3] : 0;
  stats->box_hits = c->last_stats ? h[4] : 0;
  stats->root_tests = c->last_stats ? h[5] : 0;
  stats->kernel_ms = 0.0;
  stats->launches = c->last_launches;
  return RT_OK;
}

}  // extern "C"

namespace {

// rt_render's body; host_rgb null: the frame is not copied back, sink: see
// pilot_order (rt_internal_pilot_schedule is this render with both)
int render_sync(rt_context *c, const rt_camera *cam, const rt_params *prm, float *host_rgb, rt_stats *stats,
                pilot_sink *sink) {
  int st = rt_internal_frame_check(c, cam, prm);
  if (st != RT_OK) return st;
  const size_t nf = 3 * (size_t)prm->width * (size_t)prm->local_rows;
  RT_HIP(hipSetDevice(c->device));
  RT_HIP(c->d_frame.grow(nf));
  // ev0 is recorded right before the render kernel (after a first-frame pilot)
  st = render_enqueue(c, cam, prm, c->d_frame.p, nullptr, c->ev0, sink);
  const uint32_t n_launch = std::min<uint32_t>(c->enq_launches, (uint32_t)c->ev_launch.size());
  if (st != RT_OK) return st;
  RT_HIP(hipEventRecord(c->ev1, c->stream));
  // wait launch by launch: a fault surfaces after the launch it happened in
  for (uint32_t k = 0; k < n_launch; ++k) RT_HIP(hipEventSynchronize(c->ev_launch[k]));
  RT_HIP(hipEventSynchronize(c->ev1));
  float ms = 0.f;
  RT_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  if (nf && host_rgb) RT_HIP(hipMemcpy(host_rgb, c->d_frame.p, nf * sizeof(float), hipMemcpyDeviceToHost));
  if (stats) {
    st = rt_collect_stats(c, stats);
    if (st != RT_OK) return st;
    stats->kernel_ms = ms;
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_render(rt_context *c, const rt_camera *cam, const rt_params *prm, float *host_rgb,
              rt_stats *stats) {
  if (!c || !params_ok(prm) || (!host_rgb && prm->local_rows && prm->width)) return RT_ERR_INVALID;
  return render_sync(c, cam, prm, host_rgb, stats, nullptr);
}

// The pilot schedule's diagnostics (include/rt_internal.h;
// tests/test_sched_gpu.py compares them with tests/sched_ref.py on the
// oracle's per-pixel segment counts).
int rt_internal_block_order_host(int device, const uint32_t *tile_cost, uint32_t blocks, uint32_t units,
                                 uint32_t *order) {
  if (!blocks || !units) return RT_OK;
  const uint64_t n_cost = (uint64_t)blocks * rtk::kWavesPerBlock, n_order = (uint64_t)blocks * units;
  if (!tile_cost || !order || n_cost >= (1ull << 32) || n_order >= (1ull << 32)) return RT_ERR_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return RT_ERR_NO_DEVICE;
  RT_HIP(hipSetDevice(device));
  hipStream_t st = nullptr;
  RT_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  rt_device_buf<uint32_t> d_cost, d_order;
  hipError_t e = d_cost.grow(n_cost);
  if (e == hipSuccess) e = d_order.grow(n_order);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cost.p, tile_cost, n_cost * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = rt_internal_block_order(d_cost.p, blocks, units, d_order.p, st);
  if (e == hipSuccess) e = hipMemcpyAsync(order, d_order.p, n_order * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // (also after a failure: the copies read the buffers)
  (void)hipStreamDestroy(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hip_fail(e);
  return RT_OK;
}

int rt_internal_pilot_schedule(rt_context *c, const rt_camera *cam, const rt_params *prm, uint32_t *tile_cost,
                               size_t n_cost, int *pilot_ran, uint32_t *order, size_t n_order, size_t *n_order_out,
                               float *image) {
  if (!c || !params_ok(prm) || !(prm->flags & RT_FLAG_PILOT_SCHEDULE) || !pilot_ran || !n_order_out ||
      (n_cost && !tile_cost) || (n_order && !order))
    return RT_ERR_INVALID;
  *pilot_ran = 0;
  *n_order_out = 0;
  pilot_sink sink;
  sink.tile_cost = tile_cost;
  sink.n_cost = n_cost;
  const int r = render_sync(c, cam, prm, image, nullptr, &sink);  // (waits for the stream: the costs have arrived)
  if (r != RT_OK) return r;
  *pilot_ran = sink.ran ? 1 : 0;
  if (!sink.used) return RT_OK;
  *n_order_out = c->order_n;
  if (std::min(n_order, c->order_n))
    RT_HIP(hipMemcpy(order, c->d_order, std::min(n_order, c->order_n) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_internal_context_order(rt_context *c, uint32_t *order, size_t n_order, size_t *n_order_out) {
  if (!c || !n_order_out || (n_order && !order)) return RT_ERR_INVALID;
  *n_order_out = 0;
  RT_HIP(hipSetDevice(c->device));
  RT_HIP(hipDeviceSynchronize());  // renders on caller streams included
  if (c->order_key.empty() || !c->d_order) return RT_OK;
  *n_order_out = c->order_n;
  if (std::min(n_order, c->order_n))
    RT_HIP(hipMemcpy(order, c->d_order, std::min(n_order, c->order_n) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RT_OK;
}

// Host-only view of how rt_render would cut a render into launches (no
// device needed): tests/test_host.py checks the plans of the BASELINE configs.
int rt_internal_launch_plan(const rt_params *prm, double launch_samples, uint64_t *out, size_t n_out) {
  if (!out || !params_ok(prm) || !(launch_samples >= 0.0)) return RT_ERR_INVALID;
  const launch_plan lp = plan_launches(prm, launch_samples > 0.0 ? launch_samples : rtk::kLaunchSamples);
  const uint64_t v[RT_LAUNCH_PLAN_N] = {(uint64_t)lp.ranges, (uint64_t)lp.chunks, (uint64_t)lp.units,
                                        (uint64_t)lp.entries, (uint64_t)(lp.ranges * lp.chunks)};
  for (size_t i = 0; i < n_out && i < RT_LAUNCH_PLAN_N; ++i) out[i] = v[i];
  return RT_OK;
}

// Host-only view of what rt_scene_upload would build (no device needed):
// tests/test_host.py checks the builder's invariants on CPU, and
// tools/host_sanitize.sh runs it under ASan / UBSan.  See include/rt.h for
// the out[] layout.
int rt_internal_accel_info(const rt_scene_view *s, int grid_placement, double grid_scale, uint64_t *out,
                           size_t n_out) {
  if (!out || !rtk::scene_ok(s) || grid_placement < 0 || grid_placement > 3 ||
      !(grid_scale == 0.0 || (grid_scale >= 0.05 && grid_scale <= 20.0)))
    return RT_ERR_INVALID;
  rtk::accel_options o;
  o.wide = rtk::max_albedo(s) > 1.0;
  o.grid_placement = kPlacementOpt[grid_placement];
  o.grid_scale = grid_scale == 0.0 ? 1.0 : grid_scale;
  rtk::accel_build a;
  rtk::build_accel(s, o, a);
  uint64_t v[RT_ACCEL_INFO_N];
  std::memset(v, 0, sizeof v);
  v[0] = a.per_order;  // (a's rtk::scene_dims)
  v[1] = a.n_slots;
  v[2] = a.layer_mode ? 1u : 0u;
  v[3] = a.extra_pair0;
  v[4] = a.n_extra_pairs;
  const rtk::grid_geom &g = a.grid;
  v[5] = (uint64_t)g.nx;
  v[6] = (uint64_t)g.nz;
  const uint64_t items = g.items.size() / 4, cells = g.cells.size();
  v[7] = items;
  v[8] = cells ? rtk::grid_lds_bytes(a.grid_placement, (long long)items, (long long)cells) : 0u;
  v[9] = cells && a.grid_placement == rtk::kGridLds;
  // every stored cell's first item is the running count (ring cells included),
  // so cell i's items are [first_i, first_{i+1}) -- what the LDS walk reads
  uint64_t maxc = 0, listed = 0;
  bool start_ok = true, ring_ok = true;
  for (uint64_t i = 0; i < cells; ++i) {
    const uint32_t first = g.cells[i] >> 4, cnt = g.cells[i] & 15u;
    const uint64_t next = i + 1 < cells ? (g.cells[i + 1] >> 4) : items;
    start_ok = start_ok && first + cnt == next;
    maxc = std::max<uint64_t>(maxc, cnt);
    listed += cnt ? 1u : 0u;
    const int x = (int)(i % g.nx), z = (int)(i / g.nx);
    if (x == 0 || z == 0 || x == g.nx - 1 || z == g.nz - 1) ring_ok = ring_ok && cnt == 0;
  }
  v[10] = maxc;
  v[11] = cells ? (start_ok ? 1u : 0u) : 0u;
  v[12] = cells ? (ring_ok ? 1u : 0u) : 0u;
  v[13] = (uint64_t)(a.oref * 1000.0);
  v[14] = a.layer_mode ? (uint64_t)(2 * a.extra_pair0) : 0u;
  v[15] = listed;
  static const uint64_t kPlaceOut[3] = {RT_GRID_GLOBAL, RT_GRID_LDS, RT_GRID_CELLS_LDS};
  v[16] = cells ? kPlaceOut[a.grid_placement] : 0u;
  v[17] = (uint64_t)std::llround(g.scale * 1000.0);
  v[18] = (uint64_t)a.extras_fold;
  uint32_t cy_bits;
  std::memcpy(&cy_bits, &a.extras_cy, sizeof cy_bits);
  v[19] = cy_bits;
  for (size_t k = 0; a.layer_mode && k < 16 && k < 2 * (size_t)a.n_extra_pairs; ++k)
    v[20 + k] = (uint64_t)(a.slots[2 * (size_t)a.extra_pair0 + k] + 1);
  // the grid's geometry as the kernel gets it (grid_kparams): float32 bits
  const float geom[7] = {g.xi, g.zi, g.g, g.x1, g.z1, g.x0, g.z0};
  for (size_t k = 0; cells && k < 7; ++k) {
    uint32_t bits;
    std::memcpy(&bits, &geom[k], sizeof bits);
    v[36 + k] = bits;
  }
  std::memcpy(out, v, std::min<size_t>(n_out, RT_ACCEL_INFO_N) * sizeof(uint64_t));
  return RT_OK;
}

int rt_internal_grid_fit(const rt_scene_view *s, const rt_camera *cam, int width, int height, double *scale,
                         double *costs, size_t n_costs, size_t *n) {
  return rt_internal_grid_fit_phase(s, cam, width, height, 0.0, 0.0, scale, costs, n_costs, n);
}

int rt_internal_grid_fit_phase(const rt_scene_view *s, const rt_camera *cam, int width, int height, double phase_x,
                               double phase_z, double *scale, double *costs, size_t n_costs, size_t *n) {
  if (!rtk::scene_ok(s) || !cam || !scale || width < 1 || height < 1 || (n_costs && !costs)) return RT_ERR_INVALID;
  if (!(phase_x >= 0.0 && phase_x < 1.0 && phase_z >= 0.0 && phase_z < 1.0)) return RT_ERR_INVALID;
  rtk::accel_options o;
  o.grid_phase_x = phase_x;
  o.grid_phase_z = phase_z;
  o.wide = rtk::max_albedo(s) > 1.0;
  rtk::accel_build a;
  rtk::grid_fitter *f = nullptr;
  rtk::build_accel(s, o, a, &f);
  *scale = 0.0;
  if (n) *n = 0;
  if (!f) return RT_OK;
  std::vector<std::pair<double, double>> cs;
  *scale = f->choose(*cam, width, height, &cs);
  delete f;
  if (n) *n = cs.size();
  for (size_t i = 0; i < cs.size() && i < n_costs; ++i) {
    costs[2 * i] = cs[i].first;
    costs[2 * i + 1] = cs[i].second;
  }
  return RT_OK;
}

int rt_internal_grid_scale(rt_context *c, double *scale) {
  if (!c || !scale) return RT_ERR_INVALID;
  *scale = c->sc.d_grid_cells.p ? c->sc.grid.scale : 0.0;
  return RT_OK;
}

int rt_internal_sealed(const rt_scene_view *s, uint8_t *out, size_t n_out) {
  if (!rtk::scene_ok(s) || (n_out && !out)) return RT_ERR_INVALID;
  std::vector<uint8_t> v;
  rtk::sealed_spheres(s, v);
  if (n_out && !v.empty()) std::memcpy(out, v.data(), std::min<size_t>(n_out, v.size()));
  return RT_OK;
}

int rt_device_kat(int device, int kind, const double *in, size_t n_cases, double *out) {
  if (kind < RT_KAT_SPHERE_HIT || kind > RT_KAT_REFLECTANCE || (n_cases && (!in || !out)) ||
      n_cases > (1u << 20))
    return RT_ERR_INVALID;
  if (!n_cases) return RT_OK;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return RT_ERR_NO_DEVICE;
  RT_HIP(hipSetDevice(device));
  double *d = nullptr;
  RT_HIP(hipMalloc(&d, 19 * sizeof(double) * n_cases));
  hipError_t e = hipMemcpy(d, in, 10 * sizeof(double) * n_cases, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = rtk::launch_kat(kind, d, (int)n_cases, d + 10 * n_cases);
  if (e == hipSuccess) e = hipMemcpy(out, d + 10 * n_cases, 9 * sizeof(double) * n_cases, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(e);
  return RT_OK;
}

int rt_tonemap_async(rt_context *c, const float *d_sums, size_t n_pixels, int spp, int mode, uint8_t *d_out,
                     void *stream) {
  if (!c || spp < 1 || (mode != RT_TONEMAP_CPU && mode != RT_TONEMAP_GPU) || ((!d_sums || !d_out) && n_pixels))
    return RT_ERR_INVALID;
  if (!n_pixels) return RT_OK;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  RT_HIP(hipSetDevice(c->device));
  const uint64_t n = 3 * (uint64_t)n_pixels;
  if (mode == RT_TONEMAP_CPU)
    RT_HIP(rtk::launch_tonemap(false, d_sums, n, spp, c->d_thr64.p, d_out, st));
  else
    RT_HIP(rtk::launch_tonemap(true, d_sums, n, spp, c->d_thr32.p, d_out, st));
  return RT_OK;
}

}  // extern "C"
