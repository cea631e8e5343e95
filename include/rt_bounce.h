/*
 * rt_bounce.h -- the render's path step for ray batches of the caller's own
 * (librtow_bounce.so, which links librtow.so): n rays in, per ray the closest
 * hit as rt_trace reports it AND what the render does there -- the material's
 * scatter direction and attenuation, or the sky's factor on a miss.  With
 * rt_bounce_camera_rays, which writes the render's camera rays as such a
 * batch, a wavefront path tracer over (n, 3) tensors is a loop of ten lines
 * (INTEGRATION.md), and that loop reproduces rt_render bit for bit.  The way
 * in for direct lighting with rt_segment shadow rays, per-bounce outputs,
 * another path-length rule or Russian roulette, path regeneration, an
 * accumulator of the caller's own.  The reference has no such entry; its step
 * is ray_color (src/cpu/main.cc:14-30) and material.h's scatter functions.
 *
 * Semantics
 *  - A ray with key = (pix, s, k) and from = f is one lane's pass through the
 *    render's segment loop, from a walk to the next counted hit or the miss:
 *    sample s of pixel pix after k counted hits, starting on sphere f.
 *  - origin and direction are 3n floats each, x y z per ray.  Directions are
 *    UNNORMALISED: the pass normalises them as the render normalises a camera
 *    ray or a scatter direction, and t_min is that normalisation's value, 0.001
 *    in units of the unnormalised direction.  Feeding a step's `scatter` back
 *    as the next step's `direction` (and `position` as `origin`, `id` as
 *    `from`, the key's depth + 1) continues the path exactly as the render does.
 *  - from: the sphere the ray starts on (the previous hit's id), -1 = none (a
 *    camera ray).  from == NULL means -1 for every ray.
 *  - The hit is the render's: the same candidate rule and
 *    RT_FLAG_OPEN_INTERVAL choice, the same refined root, the face rule.
 *  - BOTH arms of the render's spurious-root rule apply (a refined root on a
 *    sphere the ray moves away from, b > 0).  A refined root before t_min: the
 *    ray walks again from the scan's root point, and the distance walked is
 *    added to t.  The exiting root of sphere `from` itself: the ray walks again
 *    from the same origin with t_min raised to the float after the scan's root.
 *    After either skip the direction is NORMALISED AGAIN and t_min is kept:
 *    the render's form and rt_guides', not rt_trace's, which keeps the
 *    direction's bits.  So a camera ray that takes a skip gets rt_guides'
 *    record at max_bounces = -1 here, and rt_aov's from rt_trace; the two can
 *    differ in the last bits.
 *  - At the hit one draw r = pcg4d(pix, s, k + 1, seed32) is made, and the
 *    render's material blocks run on it (lambertian with the opaque-inside
 *    rule, metal with the fuzz form RT_FLAG_METAL_UNIT_VECTOR selects,
 *    dielectric).  status is RT_BOUNCE_SCATTERED or RT_BOUNCE_ABSORBED as the
 *    render's `scattered` says.  The pass knows nothing of max_depth: the cap
 *    is the caller's loop.
 *  - attenuation: at a hit the sphere's albedo (1, 1, 1 for glass), absorbed
 *    or not.  At a miss the sky's factor for the normalised direction,
 *    a = 0.5 (dy + 1), s0 = 1 - a, (fma(a, .5, s0), fma(a, .7, s0), s0 + a):
 *    the caller's throughput * attenuation in fp32 is the render's sample
 *    radiance.  The pass holds no throughput; the caller multiplies per hit,
 *    and in scenes with an albedo above 1 clamps with fminf(., 2^100) after
 *    each multiply as the render does.
 *  - scatter: at a SCATTERED hit the next ray's UNNORMALISED direction (its
 *    origin is `position`); +0 otherwise.
 *  - id, t, position, normal: as rt_trace (t = distance walked + the refined
 *    root).  A miss: id = -1, t = +inf, position = normal = scatter = +0.
 *  - An invalid ray -- rt_trace's forms (a non-finite origin or direction
 *    component, l2 of the direction 0 or non-finite), from outside
 *    [-1, n_spheres), key sample >= 2^24 or key depth >= 2^24 - 1 (pcg4d
 *    multiplies them as 24-bit numbers): status RT_BOUNCE_INVALID, id = -2,
 *    t = +inf, everything else +0.  It is never traced and does not affect the
 *    other rays.  rt_bounce_camera_rays writes such a ray for a padding row.
 *  - seed: reduced to 32 bits exactly as rt_params.seed is.
 *  - flags: RT_FLAG_OPEN_INTERVAL, RT_FLAG_ACCEL_BVH, RT_FLAG_LAYER_BVH and
 *    RT_FLAG_METAL_UNIT_VECTOR mean what they mean to a render; other bits are
 *    ignored.
 *  - The result is a function of the ray, its from, its key, the seed, the
 *    scene, RT_FLAG_OPEN_INTERVAL and RT_FLAG_METAL_UNIT_VECTOR only:
 *    identical bits from every walk (scan, BVH, layer BVH, layer grid), every
 *    grid placement and cell size, every split into launches
 *    (RT_OPT_LAUNCH_SAMPLES) and every position of a ray within the batch.
 *  - The render's segment counters are not touched; the grid is the one the
 *    context holds, as for rt_trace.
 *
 * A pass is serialised with the renders, feature passes and scene uploads of
 * its context, on whatever stream it runs.  One context, one host thread at a
 * time, as in rt.h.
 */
#ifndef RTOW_RT_BOUNCE_H
#define RTOW_RT_BOUNCE_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_BOUNCE_VERSION 1
#define RT_BOUNCE_MISS 0      /* status: the ray left the scene; attenuation is the sky's factor */
#define RT_BOUNCE_SCATTERED 1 /* status: a hit, and `scatter` continues the path                 */
#define RT_BOUNCE_ABSORBED 2  /* status: a hit that ends the path black                          */
#define RT_BOUNCE_INVALID 3   /* status: the ray was not traced (see above)                      */

typedef struct {            /* DEVICE pointers (rt_bounce_async) or HOST pointers (rt_bounce)      */
  uint64_t n;               /* rays, at most 2^31 - 1                                              */
  const float *origin;      /* n*3 : x y z per ray                                                 */
  const float *direction;   /* n*3 : x y z per ray, UNNORMALISED (the previous step's `scatter`)   */
  const int32_t *from;      /* n   : sphere the ray starts on; -1 = none; NULL = -1 for all        */
  const uint32_t *key;      /* n*3 : pix, sample, depth (counted hits so far) per ray              */
  uint64_t seed;            /* reduced to seed32 exactly as rt_params.seed is                      */
} rt_bounce_rays;

typedef struct {            /* DEVICE or HOST pointers like the rays; any may be NULL = not wanted */
  uint8_t *status;          /* n   : RT_BOUNCE_MISS, _SCATTERED, _ABSORBED, _INVALID               */
  int32_t *id;              /* n   : original sphere index, -1 miss, -2 invalid                    */
  float *t;                 /* n   : distance walked + refined root, +inf without a hit            */
  float *position, *normal; /* n*3 : as rt_trace                                                   */
  float *scatter;           /* n*3 : the next ray's UNNORMALISED direction; +0 unless SCATTERED    */
  float *attenuation;       /* n*3 : hit: the albedo (glass 1,1,1); miss: the sky factor; invalid: +0 */
} rt_bounce_out;

/* RT_BOUNCE_VERSION of the loaded library. */
int rt_bounce_version(void);

/* Enqueue the step on `stream` (a hipStream_t, NULL = the context's own),
 * reading the rays and writing the wanted outputs through DEVICE pointers.
 * Checked before any HIP call: RT_ERR_INVALID for a NULL ctx, rays or out, for
 * n > 2^31 - 1, for a NULL origin, direction or key when n > 0, and for a
 * wanted output whose elements share a byte with any of the four inputs or
 * with another wanted output; RT_ERR_NO_SCENE before rt_scene_upload.  n = 0
 * or all seven outputs NULL: RT_OK, nothing is launched.  The pass is cut into
 * launches of RT_OPT_LAUNCH_SAMPLES rays at most (at least one), ascending
 * ranges of the batch.  Does not synchronise. */
int rt_bounce_async(rt_context *ctx, const rt_bounce_rays *dev, const rt_bounce_out *dev_out, uint32_t flags,
                    void *stream);

/* Synchronous convenience: the same step from HOST arrays, through device
 * buffers of its own, into the HOST pointers of `host_out`; *kernel_ms (may be
 * NULL) receives the hipEvent time of the launches.  The same checks, on the
 * host ranges.  Waits launch by launch, so a device fault is reported after
 * the launch it happened in. */
int rt_bounce(rt_context *ctx, const rt_bounce_rays *host, const rt_bounce_out *host_out, uint32_t flags,
              double *kernel_ms);

/* The render's camera rays of (cam, params) as a batch for rt_bounce: ray
 * [lrow][col][j], lrow < params->local_rows (banded as a render's rows),
 * col < width, j < samples, is the camera ray of sample sample0 + j of that
 * pixel -- camera_dir on pcg4d(pix, s, 0, seed32), the lens sample included --
 * with the direction left UNNORMALISED and key = (pix, s, 0), pix = global row
 * * width + col as the render counts it.  A padding row (global row >= height)
 * gets origin = direction = +0 and key = (0, s, 0): rt_bounce and rt_trace
 * report such a ray INVALID.  params->spp and max_depth are not read beyond
 * their range checks.  Checked before any HIP call: RT_ERR_INVALID for a NULL
 * argument (with at least one ray), for params or a camera a render rejects,
 * for sample0 < 0, samples < 0, sample0 + samples > 2^24 or more than
 * 2^31 - 1 rays; RT_ERR_NO_SCENE before rt_scene_upload.  No rays: RT_OK,
 * nothing is launched.  origin and direction hold 3 floats per ray, key 3
 * uint32.  The asynchronous form takes DEVICE pointers and does not
 * synchronise; the synchronous one takes HOST pointers. */
int rt_bounce_camera_rays_async(rt_context *ctx, const rt_camera *cam, const rt_params *params, int32_t sample0,
                                int32_t samples, float *origin, float *direction, uint32_t *key, void *stream);
int rt_bounce_camera_rays(rt_context *ctx, const rt_camera *cam, const rt_params *params, int32_t sample0,
                          int32_t samples, float *origin, float *direction, uint32_t *key, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_BOUNCE_H */
