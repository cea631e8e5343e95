/*
 * rt_internal.h -- librtow.so's diagnostic and tuning entry points.
 *
 * NOT part of the drop-in boundary (include/rt.h): nothing here
 * replaces reference code.  These functions exist for the test suite
 * (tests/), the measurement tools (tools/) and host sanitizer runs: the
 * device arithmetic's known-answer vectors, and host-only views of what the
 * BVH / layer-grid builder, the launch planner and the grid fitter decide,
 * and views of the pilot schedule (its tile costs and block order).
 * A caller of the reference's render path needs rt.h only.
 */
#ifndef RTOW_RT_INTERNAL_H
#define RTOW_RT_INTERNAL_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning options for rt_context_set_option beyond rt_option (tools only):
 * the layer grid's origin shifted by this fraction of a cell in x / z,
 * [0, 1) (default 0: the grid starts at the layer's padded bounds).  Read by
 * the next rt_scene_upload; applies to the fitter's candidates too.
 * Scheduling only: every grid renders the same image.  Measured in round 5
 * and not adopted by the fitter. */
enum { RT_OPT_INTERNAL_GRID_PHASE_X = 8, RT_OPT_INTERNAL_GRID_PHASE_Z = 9 };

/* Known-answer evaluation of the render kernel's own device arithmetic on
 * `device` (synchronous).  10 doubles in, 9 out per case (layouts in
 * rt_kernel.hip, kat_kernel):
 *   RT_KAT_SPHERE_HIT   sphere::hit            src/cpu/sphere.h:24-51
 *   RT_KAT_REFLECT      reflect                src/cpu/vec3.h:122-124
 *   RT_KAT_REFRACT      refract                src/cpu/vec3.h:126-131
 *   RT_KAT_REFLECTANCE  dielectric::reflectance src/cpu/material.h:82-87 */
enum { RT_KAT_SPHERE_HIT = 0, RT_KAT_REFLECT = 1, RT_KAT_REFRACT = 2, RT_KAT_REFLECTANCE = 3 };
int rt_device_kat(int device, int kind, const double *in, size_t n_cases, double *out);

/* Host only (no device): what rt_scene_upload would build for `scene` with
 * the given RT_OPT_GRID_PLACEMENT / RT_OPT_GRID_SCALE values (0 = default) --
 * BVH size, layer split, layer-grid dimensions, LDS footprint and the grid's
 * invariants (cell i's items are [first_i, first_{i+1}); ring cells empty).
 * Writes min(n_out, RT_ACCEL_INFO_N) values:
 *   0 nodes per DFS order   1 BVH slots          2 layer mode     3 extra_pair0
 *   4 n_extra_pairs         5 grid_nx (w/ ring)  6 grid_nz        7 grid items
 *   8 grid LDS bytes        9 whole grid in LDS 10 max items/cell 11 start invariant
 *  12 empty ring cells ok  13 oref * 1000      14 layer slots    15 listed cells
 *  16 placement (RT_GRID_*, 0: no grid)         17 cell scale * 1000
 *  18 class of the first extras group (RT_EXTRAS_* bits: it picks the grid
 *     build's form of that group's test)        19 bits of the centre y its
 *     coaxial spheres share (float32; 0 without RT_EXTRAS_COAXIAL)
 *  20..35 the first 16 extras slots in scan order: 1 + original index (the
 *     slot's tie key), 0 = padding or no such slot
 *  36..42 the layer grid's geometry as the kernel gets it, each the bits of a
 *     float32 (0 without a grid): 36 grid_xi, 37 grid_zi (the listed region's
 *     low corner), 38 grid_g (the cell side), 39 grid_x1, 40 grid_z1 (its high
 *     corner), 41 grid_x0, 42 grid_z0 (the stored cells' origin, one ring
 *     cell before the listed region: the walk's border between stored columns
 *     k - 1 and k is fmaf((float)k, grid_g, grid_x0), likewise in z)
 * Classes compare bit patterns; only +0 is zero:
 *   RT_EXTRAS_AXIAL    slot 0 has cx = cz = +0
 *   RT_EXTRAS_COAXIAL  the group's other spheres share one cy and have cz = +0
 * For tests and sanitizer runs. */
#define RT_ACCEL_INFO_N 43
enum { RT_EXTRAS_AXIAL = 1, RT_EXTRAS_COAXIAL = 2 };
int rt_internal_accel_info(const rt_scene_view *scene, int grid_placement, double grid_scale, uint64_t *out,
                           size_t n_out);

/* Host only (no device): how rt_render would cut a render with these
 * parameters into launches under a launch-sample budget (0 = the default,
 * 2^35; see RT_OPT_LAUNCH_SAMPLES).  Writes min(n_out, RT_LAUNCH_PLAN_N)
 * values: 0 block ranges, 1 sample ranges per block range, 2 units (waves per
 * tile), 3 work entries (blocks x units), 4 launches (ranges x sample ranges).
 * For tests. */
#define RT_LAUNCH_PLAN_N 5
int rt_internal_launch_plan(const rt_params *params, double launch_samples, uint64_t *out, size_t n_out);

/* Host only (no device): the layer-grid cell scale RT_OPT_GRID_FIT would
 * pick for `scene` (default builder options, the automatic placement) seen by
 * `cam` in a width x height frame; *scale = 0 without a grid in an LDS
 * placement.  With costs != NULL, the modelled cost of each candidate that
 * fits: (scale, cost) pairs, min(n_costs, *n) of them (*n = their count).
 * For tests and tools. */
int rt_internal_grid_fit(const rt_scene_view *scene, const rt_camera *cam, int width, int height, double *scale,
                         double *costs, size_t n_costs, size_t *n);
/* The same with the grid's origin shifted by (phase_x, phase_z) cells, each
 * in [0, 1) (RT_OPT_INTERNAL_GRID_PHASE_X / _Z).  For tools. */
int rt_internal_grid_fit_phase(const rt_scene_view *scene, const rt_camera *cam, int width, int height,
                               double phase_x, double phase_z, double *scale, double *costs, size_t n_costs,
                               size_t *n);
/* The cell scale of the context's current layer grid (after RT_OPT_GRID_FIT
 * refits it for a render's frame geometry); 0 without a grid.  For tests and
 * the bench record. */
int rt_internal_grid_scale(rt_context *ctx, double *scale);

/* Host only (no device): for each sphere of `scene`, 1 if the kernel's
 * opaque-inside rule applies to it (a sealed lambertian sphere: no other
 * ball overlaps its ball), else 0.  Writes
 * min(n_out, scene->n) bytes.  For tests. */
int rt_internal_sealed(const rt_scene_view *scene, uint8_t *out, size_t n_out);

/* The pilot schedule (RT_FLAG_PILOT_SCHEDULE) made visible.  All
 * three are synchronous, work on host arrays and change no render.  For tests.
 *
 * The sort alone on `device`: the launch order the product's device sort
 * (csrc/rt_sched.hip, the very function pilot_order calls) gives for the tile
 * costs.  tile_cost holds blocks * 4 entries (block b's tiles at 4 b .. 4 b +
 * 3), order blocks * units.  A block's cost is the sum of its tiles' (mod
 * 2^32); blocks in decreasing cost, equal costs in increasing block index;
 * order[i * units + u] = sorted[i] * units + u.  blocks = 0 or units = 0:
 * RT_OK, nothing read or written. */
int rt_internal_block_order_host(int device, const uint32_t *tile_cost, uint32_t blocks, uint32_t units,
                                 uint32_t *order);
/* One rt_render of (cam, params) on the context's own stream -- params must
 * carry RT_FLAG_PILOT_SCHEDULE -- that also shows what its schedule was:
 * *pilot_ran = 1 if this render ran the pilot (no order was cached for its
 * frame geometry), and then tile_cost gets the pilot's segment count of each
 * tile, min(n_cost, blocks * 4) entries, tile t of the local frame (row-major
 * over its 8x8 tiles) at t, padding tiles 0; *pilot_ran = 0 if the cached
 * order served, tile_cost untouched.  order gets the first min(n_order,
 * blocks * units) entries of the order the render's launches read, *n_order_out
 * its full length (0: the render took launch order -- one block, or nothing
 * traced).  image (may be NULL): the render's sums, as rt_render's host_rgb. */
int rt_internal_pilot_schedule(rt_context *ctx, const rt_camera *cam, const rt_params *params, uint32_t *tile_cost,
                               size_t n_cost, int *pilot_ran, uint32_t *order, size_t n_order, size_t *n_order_out,
                               float *image);
/* The block order the context holds, after waiting for the device's work (so
 * also after rt_render_async on any stream): min(n_order, *n_order_out)
 * entries; *n_order_out = 0 when it holds none that is valid (no pilot render
 * yet, or a scene upload since). */
int rt_internal_context_order(rt_context *ctx, uint32_t *order, size_t n_order, size_t *n_order_out);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_INTERNAL_H */
