/*
 * rt_trace.h -- closest-hit queries for ray batches of the caller's own
 * (librtow_trace.so, which links librtow.so): n rays in, per ray the sphere
 * hit, the distance, the hit point and the shading normal out.  The way in
 * for everything that is not an image: picking under a cursor, visibility
 * between two points, collision probes, an integrator written over (n, 3)
 * tensors.  The reference has no such entry; its hit is hittable_list::hit
 * (src/cpu/hittable_list.h:28-43).
 *
 * Semantics
 *  - Ray i returns what rt_aov returns at 1 spp for a lens-less primary ray
 *    with the same origin bits and the same unnormalised direction bits.
 *  - origin and direction are 3n floats each, x y z per ray (the layout of an
 *    (n, 3) tensor).  Directions are UNNORMALISED: the pass normalises them as
 *    the render normalises a camera ray, and t_min is the render's, 0.001 in
 *    units of the unnormalised direction (0.001 |d| on the normalised ray).
 *    It is not configurable.
 *  - The hit is the hit of the render's first counted segment (rt_aov.h): the
 *    same candidate rule and RT_FLAG_OPEN_INTERVAL choice, the same refined
 *    root, the render's rule for a spurious root (a refined root before t_min
 *    on a sphere the ray moves away from: the ray walks again from the scan's
 *    root point with the direction's bits kept, and the distance walked is
 *    added to t), the render's face rule.
 *  - id: the original sphere index.  t: world units on the normalised ray,
 *    from the ray's origin.  position: P = fma(t, d, o).  normal: the render's
 *    shading normal (P - C) / r, flipped to face the ray.
 *  - A miss: id = -1, t = +inf, position = normal = +0.
 *  - An invalid ray -- a non-finite origin or direction component, or
 *    l2 = fma(z, z, fma(y, y, x x)) of the direction 0 or non-finite:
 *    id = RT_TRACE_INVALID, t = +inf, position = normal = +0.  It is never
 *    traced and does not affect the other rays.
 *  - flags: RT_FLAG_OPEN_INTERVAL, RT_FLAG_ACCEL_BVH and RT_FLAG_LAYER_BVH
 *    mean what they mean to a render and to rt_aov; other bits are ignored.
 *  - The result is a function of the rays, the scene and
 *    RT_FLAG_OPEN_INTERVAL only: identical bits from every walk (scan, BVH,
 *    layer BVH, layer grid), every grid placement and cell size, every split
 *    into launches (RT_OPT_LAUNCH_SAMPLES) and every position of a ray within
 *    the batch -- a ray's neighbours never matter.
 *  - The render's segment counters are not touched.  Without a camera there
 *    is no RT_OPT_GRID_FIT refit: the pass walks the layer grid the context
 *    holds, the builder's or the last frame's fit (same bits either way).
 *
 * A pass is serialised with the renders, feature passes and scene uploads of
 * its context, on whatever stream it runs.  One context, one host thread at a
 * time, as in rt.h.
 */
#ifndef RTOW_RT_TRACE_H
#define RTOW_RT_TRACE_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_TRACE_VERSION 1
#define RT_TRACE_MISS (-1)    /* id of a ray that hit nothing */
#define RT_TRACE_INVALID (-2) /* id of a ray that was not traced (see above) */

typedef struct {            /* DEVICE pointers (rt_trace_async) or HOST pointers (rt_trace) */
  uint64_t n;               /* rays, at most 2^31 - 1                                       */
  const float *origin;      /* n*3 : x y z per ray                                          */
  const float *direction;   /* n*3 : x y z per ray, unnormalised                            */
} rt_trace_rays;

typedef struct {            /* DEVICE or HOST pointers like the rays; any may be NULL = not wanted */
  int32_t *id;              /* n   : original sphere index, RT_TRACE_MISS, RT_TRACE_INVALID        */
  float   *t;               /* n   : distance on the normalised ray, +inf without a hit            */
  float   *position;        /* n*3 : P = fma(t, d, o), +0 without a hit                            */
  float   *normal;          /* n*3 : the shading normal facing the ray, +0 without a hit           */
} rt_trace_hits;

/* RT_TRACE_VERSION of the loaded library. */
int rt_trace_version(void);

/* Enqueue the pass on `stream` (a hipStream_t, NULL = the context's own),
 * reading the rays and writing the wanted outputs through DEVICE pointers.
 * Checked before any HIP call: RT_ERR_INVALID for a NULL ctx, rays or hits,
 * for n > 2^31 - 1, for a NULL origin or direction when n > 0, and for a
 * wanted output whose n (or 3n) elements share a byte with either input or
 * with another wanted output; RT_ERR_NO_SCENE before rt_scene_upload.  n = 0
 * or all four outputs NULL: RT_OK, nothing is launched.  The pass is cut into
 * launches of RT_OPT_LAUNCH_SAMPLES rays at most (at least one), ascending
 * ranges of the batch.  Does not synchronise. */
int rt_trace_async(rt_context *ctx, const rt_trace_rays *dev, const rt_trace_hits *dev_out, uint32_t flags,
                   void *stream);

/* Synchronous convenience: the same pass from HOST arrays, through device
 * buffers of its own, into the HOST pointers of `host_out`; *kernel_ms (may
 * be NULL) receives the hipEvent time of the launches.  The same checks, on
 * the host ranges.  Waits launch by launch, so a device fault is reported
 * after the launch it happened in. */
int rt_trace(rt_context *ctx, const rt_trace_rays *host, const rt_trace_hits *host_out, uint32_t flags,
             double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_TRACE_H */
