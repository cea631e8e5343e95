// rt_accel.h -- internal to librtow: the host-side builder of the render
// kernel's scene records and acceleration structures (rt_accel.cpp), used by
// rt_scene_upload and rt_internal_accel_info (rt_api.cpp).
#ifndef RTOW_RT_ACCEL_H
#define RTOW_RT_ACCEL_H

#include <cstdint>
#include <cstring>
#include <vector>

#include "rt_internal.h"
#include "rt_layout.h"

namespace rtk {

// builder options (rt_context_set_option; scheduling and placement only:
// every value renders the same image)
struct accel_options {
  int bvh_leaf = 4;          // RT_OPT_BVH_LEAF: spheres per BVH leaf, 1..4
  double collapse = 0.35;    // RT_OPT_BVH_COLLAPSE
  double side = 1.0;         // RT_OPT_BVH_SIDE
  double grid_scale = 1.0;   // RT_OPT_GRID_SCALE
  double grid_phase_x = 0.0, grid_phase_z = 0.0;  // RT_OPT_INTERNAL_GRID_PHASE_X / _Z
  int grid_placement = -1;   // RT_OPT_GRID_PLACEMENT: -1 auto, else kGridGlobal / kGridLds / kGridCells
  bool wide = false;         // 64-bit pixel sums (an albedo above 1): less LDS for the grid
};

// The layer grid's geometry, in one spelling from the builder to the context
// (grid_kparams in rt_api.cpp turns it into the kernel's): the stored cells'
// origin (x0, z0), the listed region [xi, x1) x [zi, z1), the cell side g, the
// stored counts nx x nz (ring included) and the cell scale it was built with.
struct grid_dims {
  float x0 = 0, z0 = 0, xi = 0, zi = 0, x1 = 0, z1 = 0, g = 0;
  int nx = 0, nz = 0;
  double scale = 1.0;
  bool operator==(const grid_dims &o) const {
    return x0 == o.x0 && z0 == o.z0 && xi == o.xi && zi == o.zi && x1 == o.x1 && z1 == o.z1 && g == o.g &&
           nx == o.nx && nz == o.nz && scale == o.scale;
  }
};
struct grid_geom : grid_dims {
  std::vector<uint32_t> cells;
  std::vector<float> items;  // 4 floats per item (the fourth a tie key's bits: compared as bits)
  bool operator==(const grid_geom &o) const {
    return grid_dims::operator==(o) && cells == o.cells && items.size() == o.items.size() &&
           (items.empty() || !std::memcmp(items.data(), o.items.data(), items.size() * sizeof(float)));
  }
};

// The scalar facts of a built scene, each once, in one spelling from the builder
// to the context (scene_kparams in rt_api.cpp turns them into the kernel's).
struct scene_dims {
  uint32_t n = 0, n_pad = 0;  // spheres; scan slots (whole kSpherePad groups)
  size_t per_order = 0;       // BVH nodes per DFS order (the node array holds 8 orders)
  size_t n_slots = 0;         // BVH slots (leaves, then the extras in layer mode)
  double oref = 64.0;         // the ray-origin bound the boxes' padding is valid for
  bool layer_mode = false;
  float layer_lo = 0.0f, layer_hi = 0.0f, layer_cy = 0.0f;
  uint32_t extra_pair0 = 0, n_extra_pairs = 0;
  int extras_fold = 0;     // kFold* bits of the first extras group (classify_extras)
  float extras_cy = 0.0f;  // kFoldRest: the centre y its spheres share
  bool operator==(const scene_dims &o) const {
    return n == o.n && n_pad == o.n_pad && per_order == o.per_order && n_slots == o.n_slots && oref == o.oref &&
           layer_mode == o.layer_mode && layer_lo == o.layer_lo && layer_hi == o.layer_hi &&
           layer_cy == o.layer_cy && extra_pair0 == o.extra_pair0 && n_extra_pairs == o.n_extra_pairs &&
           extras_fold == o.extras_fold && extras_cy == o.extras_cy;
  }
};

// everything rt_scene_upload copies to the device, plus the builder's facts
struct accel_build : scene_dims {
  std::vector<pair_geom> scan_geom;  // brute-force order, n_pad / 2 pairs
  std::vector<shade_rec> shade;      // n
  std::vector<pair_geom> bvh_geom;   // BVH leaf order (+ extras in layer mode)
  std::vector<int> slots;            // BVH slot -> original index, -1 padding (n_slots)
  std::vector<bvh_node> nodes;       // 8 DFS orders of per_order
  grid_geom grid;                        // layer grid (cells empty: none)
  int grid_placement = kGridGlobal;
};

// Layer-grid cell size per frame geometry (rt_api.cpp).  The
// walk's cost is not smooth in the cell size: what counts is where the cell
// borders fall relative to the spheres the frame's rays meet most (C4's rank
// share: 246-258 ms between scales 0.01 apart).  The fitter keeps a copy of a
// scene's layer spheres and, for a camera, models each candidate scale
// s0 (1 + 0.01 k), k = 0..kFitSteps, that fits the placement: the items per
// cell averaged over where 64 x 64 camera directions meet the layer plane
// (smoothed over 3 x 3 cells: bounces stay near), plus kFitCellCost for the
// cell step, per cell side, i.e. per unit of ray length.  It keeps the
// cheapest.  Fitted on round-4 sweeps: picks within 0.4 % of the best fixed
// scale on C4's share and the best on the headline frame (tools/grid_fit.py).
constexpr int kFitSteps = 30;
constexpr double kFitCellCost = 0.5;
class grid_fitter {
 public:
  // nullptr unless the scene walks a layer grid in an LDS placement
  static grid_fitter *make(const rt_scene_view *s, const accel_options &o, int placement, double scale0);
  ~grid_fitter();
  // the modelled cheapest candidate scale for this camera and frame (scale0
  // when the camera does not see the layer); costs (may be null) receives
  // (scale, modelled cost) per candidate that fits
  double choose(const rt_camera &cam, int width, int height, std::vector<std::pair<double, double>> *costs) const;
  // the grid at that scale (false: it does not fit the placement)
  bool build(double scale, grid_geom &out) const;
  double scale0() const;
  // the same from build_accel's builder (moved in; internal)
  static grid_fitter *make_from(const rt_scene_view *s, const accel_options &o, int placement, double scale0,
                                void *builder);

 private:
  struct impl;
  impl *p_ = nullptr;
};

// arrays present, known materials, finite centres and radii, non-zero radii,
// finite albedos >= 0 (rt_scene_upload's contract, include/rt.h)
bool scene_ok(const rt_scene_view *s);
// the largest lambertian / metal albedo channel (0 if none): above 1 the
// render needs 64-bit pixel sums (rt_api.cpp sum_format)
double max_albedo(const rt_scene_view *s);
// per sphere: 1 if the opaque-inside rule applies to it (sealed lambertian ball)
void sealed_spheres(const rt_scene_view *s, std::vector<uint8_t> &out);
// The class of a layer scene's first extras group, slots[0..4) of the extras
// (original indices, -1 padding): kFold* bits, and with kFoldRest the shared
// centre y in *cy.  Compares bit patterns: only +0 is zero (-0 is declined),
// and "one centre y" means one bit pattern.
int classify_extras(const rt_scene_view *s, const int *slots, size_t n_slots, float *cy);
// fitter (may be null): a grid fitter for the scene's layer grid, when it sits
// in an LDS placement (else null); the caller owns it
void build_accel(const rt_scene_view *s, const accel_options &o, accel_build &out, grid_fitter **fitter = nullptr);

}  // namespace rtk

#endif  // RTOW_RT_ACCEL_H
