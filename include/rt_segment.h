/*
 * rt_segment.h -- closest hits within a per-ray distance limit
 * (librtow_segment.so, which links librtow.so): rt_trace.h's query with a far
 * end.  n rays and n limits in, per ray whether anything lies on the segment,
 * and the sphere, the distance, the hit point and the shading normal of the
 * closest such thing out.  The way in for shadow rays towards a light,
 * ambient-occlusion rays of a fixed length, visibility between two points and
 * "nearest obstacle within range" probes: the walks stop at the limit instead
 * of crossing the scene.  Embree's tfar, OptiX's tmax; the reference has no
 * such entry.
 *
 * Semantics
 *  - origin and direction are rt_trace's: 3n floats each, directions
 *    UNNORMALISED, t_min the render's 0.001 in units of the unnormalised
 *    direction, not configurable, with rt_trace's bits.
 *  - t_max holds n floats in units of the unnormalised direction, like t_min:
 *    t_max[i] = 1 is the segment from o to o + d.  t_max == NULL means +inf for
 *    every ray.
 *  - The limit on the normalised ray is tlim = t_max len in fp32, where
 *    len = l2 r is the value normalize3 multiplies by 0.001f (l2 the
 *    direction's squared length, r its reciprocal root as the render computes
 *    it).
 *  - A sphere's candidate root counts only if it is strictly below tlim.  The
 *    root meant is the scan's root, the one the candidate rule orders by -- not
 *    the refined root reported as t, which differs from it by the scan's
 *    rounding.  Everything else is rt_trace's: the candidate rule and
 *    RT_FLAG_OPEN_INTERVAL choice, the refined root, the face rule, and the
 *    render's rule for a spurious root (the ray walks again from the scan's
 *    root point); after such a skip the next walk's limit is tlim - tmax in
 *    fp32, tmax the scan root walked, and once the limit is not above t_min the
 *    ray is a miss.
 *  - So, for a valid ray: rt_trace's record when that ray's scan roots lie
 *    below the limit, a miss otherwise.  With t_max = +inf, with t_max == NULL
 *    and when the product overflows to +inf, the result is rt_trace's, bit for
 *    bit.
 *  - blocked: 1 for a hit, 0 for a miss and for an invalid ray.  id, t,
 *    position, normal: as in rt_trace; a miss has id = -1, t = +inf,
 *    position = normal = +0.
 *  - An invalid ray -- rt_trace's forms, or a NaN t_max: id =
 *    RT_SEGMENT_INVALID, t = +inf, position = normal = +0, blocked = 0.  It is
 *    never traced and does not affect the other rays.  t_max <= 0 (either
 *    zero, -inf) or tlim <= t_min is a miss, never traced either.
 *  - flags: RT_FLAG_OPEN_INTERVAL, RT_FLAG_ACCEL_BVH and RT_FLAG_LAYER_BVH
 *    mean what they mean to a render and to rt_trace; other bits are ignored.
 *  - The result is a function of the ray, its t_max, the scene and
 *    RT_FLAG_OPEN_INTERVAL only: identical bits from every walk (scan, BVH,
 *    layer BVH, layer grid), every grid placement and cell size, every split
 *    into launches (RT_OPT_LAUNCH_SAMPLES) and every position of a ray within
 *    the batch.
 *  - The render's segment counters are not touched; the grid is the one the
 *    context holds, as for rt_trace.
 *  - The pass reports the CLOSEST hit on the segment.  It does not stop at the
 *    first sphere found (any-hit): the spurious-root rule needs the closest
 *    candidate.
 *
 * A pass is serialised with the renders, feature passes and scene uploads of
 * its context, on whatever stream it runs.  One context, one host thread at a
 * time, as in rt.h.
 */
#ifndef RTOW_RT_SEGMENT_H
#define RTOW_RT_SEGMENT_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_SEGMENT_VERSION 1
#define RT_SEGMENT_MISS (-1)    /* id of a ray with nothing on its segment */
#define RT_SEGMENT_INVALID (-2) /* id of a ray that was not traced (see above) */

typedef struct {            /* DEVICE pointers (rt_segment_async) or HOST pointers (rt_segment) */
  uint64_t n;               /* rays, at most 2^31 - 1                                           */
  const float *origin;      /* n*3 : x y z per ray                                              */
  const float *direction;   /* n*3 : x y z per ray, unnormalised                                */
  const float *t_max;       /* n   : the far end in units of direction; NULL = +inf for all     */
} rt_segment_rays;

typedef struct {            /* DEVICE or HOST pointers like the rays; any may be NULL = not wanted */
  uint8_t *blocked;         /* n   : 1 with a hit on the segment, else 0                           */
  int32_t *id;              /* n   : original sphere index, RT_SEGMENT_MISS, RT_SEGMENT_INVALID    */
  float   *t;               /* n   : distance on the normalised ray, +inf without a hit            */
  float   *position;        /* n*3 : P = fma(t, d, o), +0 without a hit                            */
  float   *normal;          /* n*3 : the shading normal facing the ray, +0 without a hit           */
} rt_segment_hits;

/* RT_SEGMENT_VERSION of the loaded library. */
int rt_segment_version(void);

/* Enqueue the pass on `stream` (a hipStream_t, NULL = the context's own),
 * reading the rays and writing the wanted outputs through DEVICE pointers.
 * Checked before any HIP call: RT_ERR_INVALID for a NULL ctx, rays or hits,
 * for n > 2^31 - 1, for a NULL origin or direction when n > 0, and for a
 * wanted output whose n (blocked: bytes; else 4n or 12n bytes) share a byte
 * with an input (origin, direction, and t_max's 4n bytes where given) or with
 * another wanted output; RT_ERR_NO_SCENE before rt_scene_upload.  n = 0 or all
 * five outputs NULL: RT_OK, nothing is launched.  The pass is cut into
 * launches of RT_OPT_LAUNCH_SAMPLES rays at most (at least one), ascending
 * ranges of the batch.  Does not synchronise. */
int rt_segment_async(rt_context *ctx, const rt_segment_rays *dev, const rt_segment_hits *dev_out, uint32_t flags,
                     void *stream);

/* Synchronous convenience: the same pass from HOST arrays, through device
 * buffers of its own, into the HOST pointers of `host_out`; *kernel_ms (may
 * be NULL) receives the hipEvent time of the launches.  The same checks, on
 * the host ranges.  Waits launch by launch, so a device fault is reported
 * after the launch it happened in. */
int rt_segment(rt_context *ctx, const rt_segment_rays *host, const rt_segment_hits *host_out, uint32_t flags,
               double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_SEGMENT_H */
