/*
 * rt_guides.h -- feature buffers that follow mirror and glass paths
 * (librtow_guides.so, which links librtow.so and no other pass library): the
 * buffers of rt_aov.h, but per sample the pass follows the render's own path
 * through specular surfaces -- dielectrics, and metals smooth enough to give a
 * mirror image -- and reports the first rough surface that path reaches.  A
 * pixel inside a mirror then carries the normal, position, albedo and virtual
 * depth of what is seen in the mirror, which is what rt_denoise, rt_temporal,
 * rt_resolve and rt_upscale need to tell reflected detail apart.  The buffers
 * keep rt_aov's layout and sum contract, so the four passes take them as they
 * are.  The reference has no such output.
 *
 * Semantics
 *  - The path.  Sample s in [0, spp) of a pixel is the render's sample s for
 *    the same parameters (seed, camera, frame size and bands), segment by
 *    segment: the camera draw pcg4d(pixel, s, 0, seed32) with the same lens
 *    sample and t_min; the hit at depth k (k counted hits before it) draws
 *    pcg4d(pixel, s, k + 1, seed32); the closest hit by the same candidate rule
 *    and RT_FLAG_OPEN_INTERVAL choice, the same refined root, and both arms of
 *    the render's spurious-root rule (a refined root before t_min on a sphere
 *    the ray moves away from: the ray walks again from the scan's root point;
 *    the exiting root of the very sphere the ray starts on while it moves away
 *    from its centre: the ray walks again with t_min raised just past that
 *    root).  Such a skip is not a segment and not a bounce, as in the render,
 *    and like the render's it normalises the direction again.  The face rule,
 *    the metal block (RT_FLAG_METAL_UNIT_VECTOR or the ball radius, the
 *    absorption test dot(s, n) <= 0) and the dielectric block (total internal
 *    reflection, Schlick's reflectance against unif(r.x), the refraction) are
 *    the render's arithmetic, operation for operation.
 *  - Stopping.  A hit continues the chain iff its sphere is a dielectric, or a
 *    metal whose fuzz (clamped to 1 as the scene upload does) is <= max_fuzz
 *    and which scattered (was not absorbed), and fewer than max_bounces
 *    bounces have been followed.  Otherwise that hit is the sample's terminal.
 *  - Escaping.  If the chain then misses everything, the terminal is the last
 *    surface it hit, and `escaped` counts the sample.  A sample is a hit sample
 *    iff its primary ray hits something, so `hits` equals rt_aov's `hits` bit
 *    for bit at every setting (but for the one exception in principle named
 *    under "Agreement with rt_aov" below).  Sky seen in a mirror keeps the
 *    mirror's own normal and position, which separates it from the real sky
 *    (hits = 0) in the consumers' sky test.
 *  - position and normal are the terminal's P = fma(t, d, o) and shading
 *    normal N (flipped to face the arriving ray).  albedo is the render's
 *    throughput after the terminal hit: the running product thr *= albedo in
 *    path order, starting from 1 ((1, 1, 1) for a dielectric; like the render's
 *    in a scene with an albedo above 1, the product is held at 2^100).  depth
 *    is the total length walked from the primary ray's origin to the terminal
 *    over all segments, world units, distances of skips included: the depth of
 *    the virtual image, which rt_resolve can reproject with.
 *  - id is sample 0's terminal sphere (-1 = miss).  bounces sums the bounces
 *    followed over the hit samples; an escaped sample counts the bounce that
 *    left the scene.
 *  - Agreement with rt_aov.  max_bounces = -1 (follow nothing) gives rt_aov's
 *    six buffers for the same arguments, bit for bit, with bounces = escaped =
 *    0, and `hits` is rt_aov's at every setting.  One exception in principle,
 *    to both statements: a primary ray that starts within t_min of a sphere
 *    it leaves is skipped as the render skips it, with the direction
 *    normalised again, where rt_aov keeps the direction's bits; the walk that
 *    follows may then differ in the last bit and, at a limb, in what it hits.
 *    The CPU oracle models both forms (oracle/rt_oracle.h, RTO_TERM_KEEP_DIR),
 *    and tests/test_features_oracle_gpu.py compares this pass with the
 *    renormalising one (test_guides_are_the_oracles) and rt_aov with the other
 *    (test_aov_is_the_oracles); no primary ray of its cases takes such a skip,
 *    so neither form is pinned yet and the exception stays one in principle.
 *  - rt_params.max_depth is ignored (max_bounces bounds the chain); the
 *    acceleration flags select the walk exactly as in a render; the other
 *    bookkeeping and scheduling flags and rt_params.units are ignored, and the
 *    render's segment counters are not touched.
 *  - Buffers follow the frame contract of rt.h and rt_aov.h: W * local_rows
 *    entries (x 3 for the vector buffers), row-major, row 0 = top row, banded
 *    rows; padding rows come out as 0 and id = -1.  Values are UNNORMALISED
 *    fp32 sums over the pixel's hit samples, added in ascending sample order
 *    starting from +0; a miss adds nothing.  The result is a function of the
 *    arguments only: identical bits from the scan, both BVH walks and the grid
 *    in every placement and cell size, from every split into launches
 *    (RT_OPT_LAUNCH_SAMPLES) and every band partition.
 *
 * Options: the struct reads 0 as "default" (rt_denoise.h's convention), so the
 * literal 0 of max_bounces is spelled -1; max_fuzz's default is 0 itself.
 *
 * A pass is serialised with the renders and scene uploads of its context, on
 * whatever stream it runs.  One context, one host thread at a time, as in
 * rt.h.
 */
#ifndef RTOW_RT_GUIDES_H
#define RTOW_RT_GUIDES_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_GUIDES_VERSION 1

typedef struct {
  int32_t max_bounces;   /* specular bounces followed, 1..64; 0 = default 8; -1 = none (rt_aov's buffers) */
  float   max_fuzz;      /* a metal continues the chain iff its (clamped) fuzz <= max_fuzz; default 0;
                            NaN or < 0 rejected */
  uint32_t reserved;     /* must be 0 */
} rt_guides_options;

typedef struct {           /* DEVICE pointers (rt_guides_async) or HOST pointers (rt_guides); any may be NULL = not wanted */
  uint32_t *hits;          /* W*rows     : samples of the pixel whose primary ray hit something (= rt_aov's)   */
  int32_t  *id;            /* W*rows     : original index of sample 0's terminal sphere, -1 = miss            */
  float    *depth;         /* W*rows     : sum over hit samples of the length walked to the terminal          */
  float    *position;      /* W*rows*3   : sum over hit samples of the terminal's P                           */
  float    *normal;        /* W*rows*3   : sum over hit samples of the terminal's shading normal              */
  float    *albedo;        /* W*rows*3   : sum over hit samples of the throughput after the terminal hit      */
  uint32_t *bounces;       /* W*rows     : sum over hit samples of specular bounces followed                  */
  uint32_t *escaped;       /* W*rows     : hit samples whose chain left the scene after >= 1 bounce           */
} rt_guides_buffers;

/* RT_GUIDES_VERSION of the loaded library. */
int rt_guides_version(void);

/* Enqueue the pass on `stream` (a hipStream_t, NULL = the context's own)
 * writing the wanted buffers through DEVICE pointers.  opts NULL = the
 * defaults.  RT_ERR_INVALID, before any HIP call and before the context is
 * read, for a NULL ctx / cam / params / dev, max_bounces < -1 or > 64, a NaN
 * or negative max_fuzz, reserved != 0; then the checks of rt_aov_async
 * (RT_ERR_INVALID for bad parameters, RT_ERR_NO_SCENE before rt_scene_upload).
 * All eight pointers NULL: RT_OK, nothing is launched.  Launches are cut as
 * rt_aov_async cuts them (RT_OPT_LAUNCH_SAMPLES): the first range initialises
 * the buffers, the later ones continue the stored sums.  spp = 0 writes zeros
 * and id = -1.  Does not synchronise. */
int rt_guides_async(rt_context *ctx, const rt_camera *cam, const rt_params *params, const rt_guides_options *opts,
                    const rt_guides_buffers *dev, void *stream);

/* Synchronous convenience: the same pass into device buffers of its own,
 * copied to the HOST pointers of `host`; *kernel_ms (may be NULL) receives the
 * hipEvent time of the launches.  Waits launch by launch, so a device fault is
 * reported after the launch it happened in.  A rejected call writes nothing. */
int rt_guides(rt_context *ctx, const rt_camera *cam, const rt_params *params, const rt_guides_options *opts,
              const rt_guides_buffers *host, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_GUIDES_H */
