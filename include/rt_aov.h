/*
 * rt_aov.h -- first-hit feature buffers (librtow_aov.so, which links
 * librtow.so): per pixel, what the render's primary rays hit -- coverage,
 * object id, depth, world position, shading normal, albedo -- the guide
 * buffers a denoiser, a compositor or a picker asks for next to the beauty
 * sums of rt_render.  The reference has no such output; its primary rays are
 * get_ray (src/cpu/camera.h:28-34, src/gpu/camera.h:153-167) and its first
 * hit hittable_list::hit (src/cpu/hittable_list.h:28-43).
 *
 * Semantics
 *  - Sample s in [0, spp) of a pixel is the render's primary ray for the same
 *    parameters (seed, camera, frame size and bands): the draw
 *    pcg4d(pixel, s, 0, seed32), the same lens sample, the same t_min, 0.001
 *    in units of the unnormalised direction.
 *  - Its hit is the hit of the render's first counted segment: the same
 *    candidate rule and RT_FLAG_OPEN_INTERVAL choice, the same refined root,
 *    and the render's rule for a spurious root (a refined root before t_min
 *    on a sphere the ray moves away from: the ray walks again from the scan's
 *    root point, and that walk is not a segment).  Such a skipped primary ray
 *    keeps its direction's bits here, where the passes that follow the chain
 *    beyond the first hit normalise it again, their one exception in
 *    principle to equality with this pass.  tests/test_features_oracle_gpu.py
 *    compares this pass with the oracle's form of the same name
 *    (test_aov_is_the_oracles, RTO_TERM_KEEP_DIR) and the chain passes with
 *    the other; no primary ray of its cases takes such a skip, so neither
 *    form is pinned yet.
 *  - rt_params.max_depth and RT_FLAG_METAL_UNIT_VECTOR are ignored.  The
 *    acceleration flags select the walk exactly as in a render
 *    (RT_FLAG_ACCEL_BVH, RT_FLAG_LAYER_BVH, the context's grid placement);
 *    the other bookkeeping and scheduling flags and rt_params.units are
 *    ignored, and the render's segment counters are not touched.
 *  - normal, position and albedo are the values the render shades with: P =
 *    fma(t, d, o), N = (P - C) / r flipped to face the ray, the hit sphere's
 *    albedo ((1, 1, 1) for a dielectric).  depth is t on the normalised ray,
 *    world units from the ray's origin (after a spurious root, the distance
 *    walked to the new origin is added first).
 *  - Buffers follow the frame contract of rt.h: W * local_rows entries (x 3
 *    for the vector buffers), row-major, row 0 = top row, rows banded by
 *    row_block / band_stride / band_offset; padding rows (global row >=
 *    height) come out as 0 and id = -1.  Values are UNNORMALISED sums over the
 *    pixel's hit samples: divide by hits (or by spp for a coverage-weighted
 *    mean).  id is sample 0's alone.
 *  - The sums are fp32, added in ascending sample order starting from +0; a
 *    miss adds nothing.  The order is fixed, so the result is a function of
 *    the arguments only: identical bits for every walk (scan, BVH, layer
 *    grid), every grid placement and cell size, every split into launches
 *    (RT_OPT_LAUNCH_SAMPLES) and every band partition -- the same promise the
 *    beauty sums of rt_render make.
 *
 * A pass is serialised with the renders and scene uploads of its context, on
 * whatever stream it runs.  One context, one host thread at a time, as in
 * rt.h.
 */
#ifndef RTOW_RT_AOV_H
#define RTOW_RT_AOV_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_AOV_VERSION 1

typedef struct {           /* DEVICE pointers (rt_aov_async) or HOST pointers (rt_aov); any may be NULL = not wanted */
  uint32_t *hits;          /* W*rows     : samples of the pixel whose primary ray hit something          */
  int32_t  *id;            /* W*rows     : original sphere index hit by sample 0, -1 = miss             */
  float    *depth;         /* W*rows     : sum over hit samples of t (normalised ray, world units)      */
  float    *position;      /* W*rows*3   : sum over hit samples of P = fma(t, d, o)                      */
  float    *normal;        /* W*rows*3   : sum over hit samples of the shading normal the render uses    */
  float    *albedo;        /* W*rows*3   : sum over hit samples of the hit sphere's shading albedo       */
} rt_aov_buffers;

/* RT_AOV_VERSION of the loaded library. */
int rt_aov_version(void);

/* Enqueue the pass on `stream` (a hipStream_t, NULL = the context's own)
 * writing the wanted buffers through DEVICE pointers.  Arguments are checked
 * like rt_render_async's: RT_ERR_INVALID for a bad argument (dev NULL
 * included), RT_ERR_NO_SCENE before rt_scene_upload.  All six pointers NULL:
 * RT_OK, nothing is launched.  The pass is cut into launches of about
 * RT_OPT_LAUNCH_SAMPLES samples at most: ascending sample ranges over all
 * pixels, at least one sample per pixel each; the first range initialises the
 * buffers, the later ones continue the stored sums.  spp = 0 writes zeros and
 * id = -1.  Does not synchronise. */
int rt_aov_async(rt_context *ctx, const rt_camera *cam, const rt_params *params, const rt_aov_buffers *dev,
                 void *stream);

/* Synchronous convenience: the same pass into device buffers of its own,
 * copied to the HOST pointers of `host`; *kernel_ms (may be NULL) receives the
 * hipEvent time of the launches.  Waits launch by launch, so a device fault is
 * reported after the launch it happened in. */
int rt_aov(rt_context *ctx, const rt_camera *cam, const rt_params *params, const rt_aov_buffers *host,
           double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_AOV_H */
