/*
 * rt_resolve.h -- clamped temporal resolve with centre reprojection
 * (librtow_resolve.so, which links librtow.so): temporal accumulation as in
 * rt_temporal.h, with the three remedies that header's "Known limitation"
 * paragraphs name.  The point that is looked up in the previous frame is the
 * pixel CENTRE's ray at the mean first-hit depth, not the mean first-hit
 * position, so a partly covered pixel does not look to one side and a standing
 * camera does not resample; a pixel that is only partly covered restarts; and
 * the history's colour is clamped to the mean +- gamma standard deviations of
 * this frame's 3 x 3 neighbourhood, which bounds what a stale reflection or a
 * wrong tap can carry over.  rt_temporal stays what it is, next to this pass.
 * The reference has no such step.
 *
 * Semantics
 *  - Frame, History, Output, View: as in rt_temporal.h, whose rt_temporal_view
 *    and 48 B per pixel history layout (rt_temporal_history_bytes) this pass
 *    shares; include that header for the types, its library is not needed.
 *    A history written by rt_temporal is a valid history_in here and the
 *    other way round: both write plane 0 (mean, len), plane 1 (P, sky ? 1 : 0),
 *    plane 2 (n, 0) and validate taps against planes 1 and 2 alike; only how P
 *    is formed differs (there the mean hit position, here a point on the
 *    centre ray).
 *  - Inputs.  cur: W*H*3 fp32 sums over spp samples (rt_render_async's beauty
 *    or rt_denoise_async's out).  hits (W*H uint32), depth (W*H fp32), normal
 *    (W*H*3 fp32): the sums rt_aov_async writes for THIS frame, traced with the
 *    same spp.  history_in, prev: as in rt_temporal.h.  now: the centre rays
 *    (rt_resolve_rays) of the camera THIS frame was rendered with.
 *  - Rays.  The unnormalised centre ray of pixel (col i, row j), fp32, per
 *    component:  D = (d00 + float(i) * du) + float(j) * dv.
 *    rt_resolve_rays_from_camera computes the fields in fp64 from the fp32
 *    rt_camera fields and rounds each number once:
 *      RT_CAMERA_GPU:  d00 = corner - eye,  du = horiz,  dv = vert
 *      RT_CAMERA_CPU:  d00 = corner - eye + (0.5 / (W-1)) horiz + ((H-0.5) / (H-1)) vert
 *                      du = horiz / (W-1),  dv = -vert / (H-1)
 *    the render's camera_dir at the pixel centre (u1 = u2 = 0.5), consistent
 *    with rt_temporal.h's "View": the view of the same camera maps eye + t D,
 *    t > 0, to (i, j).  A lens is ignored.
 *  - Per pixel p = (i, j), h = hits, S = float(spp), M = float(max_len), all
 *    fp32, in this order; a dot product a.b is (ax*bx + ay*by) + az*bz:
 *    1. Prepare.
 *         sky = (h == 0);  c = cur / S
 *         n = normal_sum / float(h); nn = n.n; n = nn > 0 ? n / sqrt(nn) : 0
 *         tm = depth_sum / float(h)
 *         D as under "Rays";  dl = sqrt(D.D);  u = D / dl
 *         P = eye + u * tm   (per component, eye = now.eye)
 *         sky: n = P = 0
 *    2. Neighbourhood.  The up to nine pixels (i + dx, j + dy), dy = -1 .. 1
 *       outer, dx = -1 .. 1 inner, those outside the frame skipped; per
 *       channel, with cq = cur_q / S:
 *         m1 += cq;  m2 += cq * cq;  k += 1      (all from +0)
 *         mu = m1 / float(k);  v = m2 / float(k) - mu * mu;  v = v > 0 ? v : 0
 *         sd = sqrt(v);  lo = mu - gamma * sd;  hi = mu + gamma * sd
 *       Left out entirely for gamma = +infinity.
 *    3. No history (history_in == NULL, or sky, or h < spp without
 *       RT_RESOLVE_KEEP_PARTIAL): len' = 1, m = c.
 *    4. Reproject and gather: steps 3 and 4 of rt_temporal.h, verbatim, with
 *       this P and n.
 *    5. Blend.  valid = ok && sw > 0.  When valid:
 *         hist = sc / sw;  hl = sl / sw
 *         clamp on, per channel:  hist = hist < lo ? lo : (hist > hi ? hi : hist)
 *         t = hl + 1;  len' = t < M ? t : M
 *         m = hist + (c - hist) * (1 / len')
 *       else len' = 1, m = c.
 *    6. Write history_out: plane 0 (m, len'), plane 1 (P, sky ? 1 : 0),
 *       plane 2 (n, 0); and out_c = m_c * S when out != NULL.
 *  - Arithmetic.  As rt_temporal.h: only + - x / sqrt floor, conversions,
 *    comparisons and selects, fp32, round to nearest, no contraction:
 *    tests/resolve_ref.py restates it in numpy float32 and gets the same bits.
 *    Inputs are taken to be finite.
 *  - Options.  A zero field means its default:
 *      max_len     0 -> 2;      1 .. 1024 frames (1 = no accumulation)
 *      plane_tol   0 -> 0.003;  > 0, +infinity = test off.  A fraction of the
 *                               distance from the previous eye, as in rt_temporal.h;
 *                               ten times looser than there, because P lies on the
 *                               centre ray at a MEAN depth and so a little off a
 *                               curved or grazing surface
 *      normal_cos  0 -> 0.9;    in [-1, 1], -1 = test off
 *      gamma       0 -> 1;      > 0, +infinity = clamp off
 *      flags       bit 0, RT_RESOLVE_KEEP_PARTIAL: pixels with 0 < h < spp keep
 *                  their history (default: they restart); other bits must be 0
 *    Anything else is RT_ERR_INVALID.  DESIGN.md 12 has the sweeps behind the
 *    defaults (8-frame orbits at 128 x 72): a two-frame history still wins
 *    there; plane_tol and gamma are the values that do best over max_len 2, 4
 *    and 8 together (a looser plane_tol gains a little at 2 and loses much at 8).
 *  - In place.  The kernel reads the 3 x 3 neighbourhood of cur while other
 *    lanes write out, so rt_resolve_async does NOT allow out to be cur, or to
 *    overlap it: RT_ERR_INVALID.  The synchronous rt_resolve stages out in a
 *    device buffer of its own, so there host out == cur (exactly) is allowed;
 *    any other overlap of the two is RT_ERR_INVALID there too.
 *
 * A pass is serialised with the renders, feature passes, filters and scene
 * uploads of its context, on whatever stream it runs; it needs no uploaded
 * scene.  One context, one host thread at a time, as in rt.h.
 */
#ifndef RTOW_RT_RESOLVE_H
#define RTOW_RT_RESOLVE_H

#include "rt_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_RESOLVE_VERSION 1

#define RT_RESOLVE_KEEP_PARTIAL 1u /* flags: pixels with 0 < hits < spp keep their history */

typedef struct {          /* unnormalised centre ray of pixel (col i, row j): */
  float eye[3];           /* D = (d00 + float(i) * du) + float(j) * dv        */
  float d00[3], du[3], dv[3];
} rt_resolve_rays;

typedef struct {
  int32_t width, height, spp;      /* whole frame 1..32768; spp >= 1: what cur AND the rt_aov sums were traced with */
  int32_t max_len;                 /* 0 = default, else 1..1024 frames (1 = no accumulation) */
  float plane_tol;                 /* 0 = default, else > 0; +inf = plane test off */
  float normal_cos;                /* 0 = default, else in [-1, 1]; -1 = normal test off */
  float gamma;                     /* 0 = default, else > 0; +inf = colour clamp off */
  uint32_t flags;                  /* RT_RESOLVE_KEEP_PARTIAL */
  int32_t reserved;                /* 0 */
  rt_temporal_view prev;           /* the view history_in was made with (ignored when history_in == NULL) */
  rt_resolve_rays now;             /* the centre rays of THIS frame's camera */
  /* DEVICE pointers (async) or HOST pointers (sync) */
  const float *cur;                /* W*H*3 sums over spp: rt_render's beauty or rt_denoise's out */
  const uint32_t *hits; const float *depth, *normal;   /* rt_aov sums of THIS frame */
  const void *history_in;          /* rt_temporal_history_bytes(W,H), or NULL = no history */
  void *history_out;               /* same size; must not overlap history_in */
  float *out;                      /* W*H*3 sums (mean x spp); may be NULL; see "In place" */
} rt_resolve_desc;

/* RT_RESOLVE_VERSION of the loaded library. */
int rt_resolve_version(void);

/* The centre rays of `cam` for a width x height frame (see "Rays").  Host
 * code, no HIP call.  RT_ERR_INVALID for a NULL pointer, a size outside
 * 1 .. 32768, RT_CAMERA_CPU with width < 2 or height < 2, an unknown model
 * and a non-finite result; *out is then left alone. */
int rt_resolve_rays_from_camera(const rt_camera *cam, int width, int height, rt_resolve_rays *out);

/* Enqueue the pass on `stream` (a hipStream_t, NULL = the context's own): one
 * launch, no scratch.  history_in and history_out are 16-byte aligned device
 * memory.  RT_ERR_INVALID before any HIP call, and before the context is
 * read, for a NULL context, desc or pointer (history_in and out may be NULL),
 * a size, spp or option out of range or NaN, an unknown flag, reserved != 0,
 * a misaligned history, history_out overlapping any buffer the pass reads or
 * out, out overlapping history_in, and out overlapping cur.  Does not
 * synchronise. */
int rt_resolve_async(rt_context *ctx, const rt_resolve_desc *desc, void *stream);

/* Synchronous convenience: the desc's pointers are HOST pointers (no
 * alignment asked; out may be cur itself); the pass runs in device buffers of
 * its own on the context's stream; *kernel_ms (may be NULL) receives the
 * hipEvent time of its launch. */
int rt_resolve(rt_context *ctx, const rt_resolve_desc *host, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_RESOLVE_H */
