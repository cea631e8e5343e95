/*
 * rt_route.h -- guide buffers of each pixel's dominant specular route
 * (librtow_route.so, which links librtow.so and no other pass library).  The
 * chain-following feature pass (the one that sums every hit sample's terminal)
 * gives means over several terminals wherever a pixel's samples take different
 * routes through glass: reflection off a shell, refraction through two or four
 * surfaces.  This pass traces the same chains, votes per pixel for the route
 * most samples took, and reports the features of that route's samples only,
 * in rt_aov.h's layout and sum contract, so rt_denoise, rt_temporal,
 * rt_resolve and rt_upscale take the buffers as they are.  The reference has
 * no such output.
 *
 * Semantics
 *  - Sample and chain.  Sample s in [0, spp) of a pixel is the chain-following
 *    pass's sample s for the same arguments and the same max_bounces /
 *    max_fuzz: the render's sample s segment by segment (the camera draw
 *    pcg4d(pixel, s, 0, seed32), the hit at depth k drawing pcg4d(pixel, s,
 *    k + 1, seed32), the closest hit by the render's candidate rule and
 *    RT_FLAG_OPEN_INTERVAL choice, the refined root, both arms of the
 *    spurious-root rule, the face rule, the metal and the dielectric block,
 *    operation for operation).  A hit continues the chain iff its sphere is a
 *    dielectric, or a metal whose clamped fuzz is <= max_fuzz and which
 *    scattered, and fewer than max_bounces bounces have been followed;
 *    otherwise it is the sample's terminal.  A chain that then misses
 *    everything escaped: its terminal is the last surface it hit.  A sample is
 *    a hit sample iff its primary ray hits something.  Its features x are ten
 *    floats: depth, the total length walked to the terminal over all segments;
 *    P = fma(t, d, o) and the shading normal N of the terminal; albedo, the
 *    throughput after the terminal hit (the running product of the albedos in
 *    path order from 1, held at 2^100).
 *  - The route key.  With b_s the bounces sample s followed (an escaped sample
 *    counts the bounce that left the scene) and e_s = 1 iff it escaped,
 *        k_s = ((b_s << 1) | e_s) + 1,
 *    a uint32 that is never 0.
 *  - Per-pixel state: key, votes, n, hits (uint32), ten fp32 sums (depth, P, N,
 *    albedo) and id (int32).  It starts as all zero with id = -1 and is
 *    updated in ascending sample order by one lane.  A miss changes nothing.
 *    A hit sample first does hits += 1, and sample 0 sets id to its terminal
 *    sphere's original index.  Then, with its key k and features x:
 *        votes == 0 :  key = k; votes = 1; n = 1; each sum = (+0) + x   (adopt)
 *        k == key   :  votes += 1; n += 1; each sum = sum + x
 *        otherwise  :  votes -= 1
 *    This is the one-sweep majority vote: a key held by more than half of the
 *    hit samples is always the final key, and votes never goes below 0.  The
 *    sums cover the final key's samples since its last adoption; n counts them.
 *  - Finalize, after the last sample, per pixel:
 *        hits    = the state's hits (rt_aov's, bit for bit)
 *        id      = the state's id: sample 0's terminal, -1 = miss
 *        depth, position, normal, albedo:
 *                  n == hits : the state's sums, copied;
 *                  otherwise : per component (sum / float(n)) * float(hits),
 *                  with correctly rounded fp32 division and multiplication,
 *                  not contracted: the dominant route's mean features in
 *                  rt_aov's sum contract, so that a consumer's "/ hits" and
 *                  "spp - hits" arithmetic stays right
 *        route   = key - 1 in uint32 arithmetic: (b << 1) | e of the dominant
 *                  route; 0xFFFFFFFF when hits == 0
 *        matched = n
 *    A pixel with hits == 0 has an all-zero state: zeros, id = -1, route =
 *    0xFFFFFFFF.  Padding rows (the frame contract of rt.h) get the same.
 *  - Consequences.  With max_bounces = -1 every key is 1, so the six shared
 *    buffers are rt_aov's bytes (but for rt_aov's one exception in principle,
 *    a primary ray starting within t_min of a sphere it leaves: this pass
 *    normalises the skipped direction again, rt_aov keeps its bits;
 *    tests/test_features_oracle_gpu.py compares each pass with the oracle's
 *    form of it, but no primary ray of its cases takes such a skip, so
 *    neither form is pinned yet).  Wherever
 *    matched == hits and the candidate never changed, the six are the
 *    chain-following pass's bytes.  hits is rt_aov's at every setting.
 *  - rt_params.max_depth, units and the bookkeeping and scheduling flags are
 *    ignored; the acceleration flags select the walk as in a render; the
 *    render's segment counters are not touched.  The result (outputs and
 *    state) is a function of the arguments only: identical bits from the
 *    scan, both BVH walks and the grid in every placement and cell size, from
 *    every split into launches (RT_OPT_LAUNCH_SAMPLES) and every band
 *    partition.
 *
 * The state buffer: rt_route_state_bytes(W, local_rows) = 64 bytes per pixel,
 * 16-byte aligned, four planes of W * local_rows 16-byte entries each, pixel
 * o = local_row * W + col at entry o of every plane:
 *        plane 0 : uint32 key, votes, n, hits
 *        plane 1 : float  P.x, P.y, P.z, depth
 *        plane 2 : float  N.x, N.y, N.z; int32 id (its bits)
 *        plane 3 : float  albedo.r, albedo.g, albedo.b; uint32 0
 * The first sample range of a call initialises it, later ranges read it,
 * continue it and write it back, and the finalize kernel reads it; after the
 * call it holds the final state.
 *
 * Options: the struct reads 0 as "default", so the literal 0 of max_bounces is
 * spelled -1; max_fuzz's default is 0 itself.
 *
 * A pass is serialised with the renders and scene uploads of its context, on
 * whatever stream it runs.  One context, one host thread at a time, as in
 * rt.h.
 */
#ifndef RTOW_RT_ROUTE_H
#define RTOW_RT_ROUTE_H

#include <stddef.h>

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ROUTE_VERSION 1
#define RT_ROUTE_STATE_BYTES_PER_PIXEL 64

typedef struct {
  int32_t max_bounces;   /* specular bounces followed, 1..64; 0 = default 8; -1 = none (rt_aov's buffers) */
  float   max_fuzz;      /* a metal continues the chain iff its (clamped) fuzz <= max_fuzz; default 0;
                            NaN or < 0 rejected */
  uint32_t reserved;     /* must be 0 */
} rt_route_options;

typedef struct {           /* DEVICE pointers (rt_route_async) or HOST pointers (rt_route); any may be NULL = not wanted */
  uint32_t *hits;          /* W*rows     : samples of the pixel whose primary ray hit something (= rt_aov's)       */
  int32_t  *id;            /* W*rows     : original index of sample 0's terminal sphere, -1 = miss                */
  float    *depth;         /* W*rows     : the dominant route's mean length walked to the terminal, times hits    */
  float    *position;      /* W*rows*3   : the dominant route's mean terminal P, times hits                       */
  float    *normal;        /* W*rows*3   : the dominant route's mean terminal shading normal, times hits          */
  float    *albedo;        /* W*rows*3   : the dominant route's mean throughput after the terminal, times hits    */
  uint32_t *route;         /* W*rows     : (bounces << 1) | escaped of the dominant route, 0xFFFFFFFF = no hit    */
  uint32_t *matched;       /* W*rows     : samples the six buffers above are the mean of (n)                      */
  void     *state;         /* rt_route only: HOST array of rt_route_state_bytes that receives the final state,
                              any alignment; rt_route_async: must be NULL (its state is an argument)              */
} rt_route_buffers;

/* RT_ROUTE_VERSION of the loaded library. */
int rt_route_version(void);

/* Bytes of the state of a width x local_rows frame: 64 per pixel; 0 when
 * either is < 1. */
size_t rt_route_state_bytes(int width, int local_rows);

/* Enqueue the pass on `stream` (a hipStream_t, NULL = the context's own):
 * the launches over the sample ranges into `state` (DEVICE memory of
 * rt_route_state_bytes(width, local_rows), 16-byte aligned), then the finalize
 * kernel writing the wanted buffers through DEVICE pointers.  opts NULL = the
 * defaults.  RT_ERR_INVALID, before any HIP call and before the context is
 * read, for a NULL ctx / cam / params / dev, max_bounces < -1 or > 64, a NaN
 * or negative max_fuzz, reserved != 0, a NULL or misaligned state, dev->state
 * != NULL, and a state that overlaps one of the wanted buffers (for a params
 * with width and local_rows >= 1); then the checks of rt_aov_async
 * (RT_ERR_INVALID for bad parameters, RT_ERR_NO_SCENE before rt_scene_upload).
 * All eight output pointers NULL: RT_OK, nothing is launched and the state is
 * not written.  Launches are cut as rt_aov_async cuts them
 * (RT_OPT_LAUNCH_SAMPLES).  spp = 0 writes zeros, id = -1 and route =
 * 0xFFFFFFFF.  Does not synchronise. */
int rt_route_async(rt_context *ctx, const rt_camera *cam, const rt_params *params, const rt_route_options *opts,
                   const rt_route_buffers *dev, void *state, void *stream);

/* Synchronous convenience: the same pass into device buffers and a state of
 * its own, copied to the HOST pointers of `host` (host->state, if not NULL,
 * receives the final state); *kernel_ms (may be NULL) receives the hipEvent
 * time of the launches.  Waits launch by launch, so a device fault is reported
 * after the launch it happened in.  All nine pointers NULL: RT_OK, nothing is
 * launched.  A rejected call writes nothing. */
int rt_route(rt_context *ctx, const rt_camera *cam, const rt_params *params, const rt_route_options *opts,
             const rt_route_buffers *host, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_ROUTE_H */
