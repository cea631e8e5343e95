/*
 * rt_upscale.h -- guided upsampling of a low-resolution frame
 * (librtow_upscale.so, which links librtow.so): the stage an interactive path
 * tracer puts behind the filters when the render and the denoiser run at a
 * fraction of the output's pixels.  Only the cheap first-hit guide buffers
 * (rt_aov.h) are traced at the output's resolution; the full-resolution frame
 * is rebuilt from the low-resolution colour, steered by both sets of guides:
 * an output pixel takes the bilinear mix of those of its low-resolution
 * neighbours that lie on its own surface, on albedo-demodulated colour, and
 * its own albedo is multiplied back in.  The reference has no such step.
 *
 * Semantics
 *  - Frames.  Two whole assembled frames, row-major, row 0 = top row: the
 *    low-resolution one of w x h = lo_width x lo_height pixels, and the output
 *    of W x H = width x height pixels.  Any pair of sizes is allowed (the
 *    output may be the smaller one).  The two cameras share the eye: without
 *    parallax a pixel maps from one frame into the other without its depth.
 *    rays.eye must equal lo_view.eye bit for bit.  A lens is ignored.
 *  - Inputs.  cur: w*h*3 fp32 sums over lo_spp samples (rt_render_async's
 *    beauty, rt_denoise_async's out or a temporal pass's out).  hits_lo (w*h
 *    uint32), position_lo, normal_lo, albedo_lo (w*h*3 fp32): the sums
 *    rt_aov_async writes for the low-resolution frame, traced with lo_spp.
 *    hits_hi, position_hi, normal_hi, albedo_hi: the same for the output
 *    frame, traced with spp.  lo_view: rt_temporal_view_from_camera(lo camera,
 *    w, h), rt_temporal.h's "View".  rays: rt_resolve_rays_from_camera(hi
 *    camera, W, H), rt_resolve.h's "Rays".  With RT_UPSCALE_NO_ALBEDO the two
 *    albedo buffers are not read and may be NULL.
 *  - Output.  out: W*H*3 fp32 in the sum contract of the LOW-resolution frame
 *    (mean x lo_spp), so rt_tonemap_async with lo_spp works on it unchanged.
 *    stage (may be NULL): W*H bytes, which step below produced the pixel (1,
 *    2 or 3).
 *  - Scratch.  rt_upscale_scratch_bytes(w, h) = 48 * w * h bytes: three planes
 *    of w*h float4, plane-major, each row-major, written by launch 1:
 *      plane 0  (u_r, u_g, u_b, sky ? 1 : 0)
 *      plane 1  (Px, Py, Pz, 0)
 *      plane 2  (nx, ny, nz, 0)
 *  - A dot product a.b is (ax*bx + ay*by) + az*bz everywhere.
 *  - Launch 1, per low-resolution pixel t, h = hits_lo, S = float(lo_spp):
 *      sky, n, P as rt_denoise.h's Prepare
 *      a_c = (albedo_lo_c + float(lo_spp - h)) / S;  m_c = a_c > 1e-3f ? a_c : 1e-3f
 *      (RT_UPSCALE_NO_ALBEDO: m_c = 1)
 *      u_c = (cur_c / S) / m_c
 *    and the three planes are written.
 *  - Launch 2, per output pixel p = (col i, row j), h = hits_hi, S = float(spp):
 *    1. Prepare sky, n, P and m from the hi sums in the same way (a miss
 *       counts as albedo 1; RT_UPSCALE_NO_ALBEDO: m_c = 1).
 *    2. Map the pixel into the low-resolution frame:
 *         D = (d00 + float(i) * du) + float(j) * dv        (rays)
 *         wq = pw.D;  x = (px.D) / wq - x0;  y = (py.D) / wq - y0   (lo_view; its eye is not used)
 *         x = x > 0 ? x : 0  (NaN becomes 0);  xm = float(w - 1);  x = x < xm ? x : xm
 *         y likewise with float(h - 1)
 *         xf = floor(x), fx = x - xf, xi = int(xf);  yf, fy, yi likewise
 *    3. Tap validity.  q = P - rays.eye, d2 = q.q, pt2 = plane_tol * plane_tol.
 *       A low-resolution pixel t is VALID for p when it lies in the frame; its
 *       sky flag equals p's; and, for a non-sky p, e*e <= pt2*d2 with
 *       e = n.(P_t - P) (left out entirely for plane_tol = +infinity) and
 *       n.n_t >= normal_cos (left out for normal_cos = -1).
 *    4. Stage 1.  The four taps (dy, dx) = (0,0), (0,1), (1,0), (1,1) in that
 *       order, t = (xi + dx, yi + dy), b = (dx ? fx : 1 - fx) * (dy ? fy : 1 - fy).
 *       For each valid tap:  sw += b;  sc_c += b * u_t,c.  Every sum starts
 *       from +0.  Done if sw > 0.
 *    5. Stage 2, when sw == 0.  The sixteen taps dy = -1 .. 2 (outer), dx =
 *       -1 .. 2 (inner), t = (xi + dx, yi + dy).  For each valid tap:
 *       sw += 1;  sc_c += u_t,c, again from +0.  Done if sw > 0.
 *    6. Stage 3, when sw is still 0.  Stage 1's four taps and weights, from
 *       +0, with validity reduced to "lies in the frame".  Tap (0,0) always
 *       does and its b is > 0, so sw > 0 now.
 *    7. out_c = ((sc_c / sw) * m_c) * float(lo_spp); stage = the stage's number.
 *  - Arithmetic.  Only + - x / sqrt floor, float <-> int conversion,
 *    comparisons and selects, fp32, round to nearest, denormals kept, no
 *    contraction and no fast-math forms: tests/upscale_ref.py restates it in
 *    numpy float32 and gets the same bits.  Inputs are taken to be finite.
 *  - Options.  A zero field means its default:
 *      plane_tol   0 -> 0.1;   > 0, +infinity = test off.  A fraction of the
 *                              distance from the eye, as in rt_temporal.h
 *      normal_cos  0 -> -0.5;  in [-1, 1], -1 = test off
 *      flags       bit 0, RT_UPSCALE_NO_ALBEDO; other bits must be 0
 *    Anything else is RT_ERR_INVALID.  DESIGN.md 13 has the sweep behind the
 *    defaults (64 x 36 -> 128 x 72, 16 spp, denoised, both scenes).  Both are
 *    far looser than the temporal passes': a low-resolution pixel covers four
 *    output pixels, so on a small sphere its mean position and normal lie well
 *    off the output pixel's own, and turning such taps away costs more (a
 *    noisier stage 2, an unguided stage 3) than letting them in.
 *  - Known limitation.  A partly covered output pixel (0 < hits_hi < spp) is
 *    treated as surface and takes one surface's guides: its P and n are means
 *    over the samples that hit, and the sky's share of its colour comes from
 *    whatever its surface taps hold.
 *  - Known limitation.  The guides are first-hit: what is seen in a mirror or
 *    through glass has the mirror's or the glass's own smooth guides, so
 *    reflections and refractions are upsampled as plain bilinear detail.
 *    rt_guides.h gives buffers of the same layout that follow such paths to
 *    what is seen.
 *
 * A pass is serialised with the renders, feature passes, filters and scene
 * uploads of its context, on whatever stream it runs; it needs no uploaded
 * scene.  One context, one host thread at a time, as in rt.h.
 */
#ifndef RTOW_RT_UPSCALE_H
#define RTOW_RT_UPSCALE_H

#include "rt_resolve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_UPSCALE_VERSION 1

#define RT_UPSCALE_NO_ALBEDO 1u /* flags: no demodulation; albedo_lo / albedo_hi may be NULL */

typedef struct {
  int32_t lo_width, lo_height, lo_spp; /* the low-res frame; 1..32768; spp >= 1: what cur AND the lo rt_aov sums were traced with */
  int32_t width, height, spp;          /* the output frame; 1..32768; spp >= 1: what the hi rt_aov sums were traced with */
  float plane_tol;                     /* 0 = default, else > 0; +inf = plane test off */
  float normal_cos;                    /* 0 = default, else in [-1, 1]; -1 = normal test off */
  uint32_t flags;                      /* RT_UPSCALE_NO_ALBEDO */
  int32_t reserved;                    /* 0 */
  rt_temporal_view lo_view;            /* rt_temporal_view_from_camera(lo camera, lo_width, lo_height) */
  rt_resolve_rays rays;                /* rt_resolve_rays_from_camera(hi camera, width, height) */
  /* DEVICE pointers (async) or HOST pointers (sync) */
  const float *cur;                    /* w*h*3 sums over lo_spp: beauty, rt_denoise's or a temporal pass's out */
  const uint32_t *hits_lo; const float *position_lo, *normal_lo, *albedo_lo;   /* rt_aov sums of the low-res frame */
  const uint32_t *hits_hi; const float *position_hi, *normal_hi, *albedo_hi;   /* rt_aov sums of the output frame */
  float *out;                          /* W*H*3 sums: mean x lo_spp */
  uint8_t *stage;                      /* W*H, may be NULL: which step produced the pixel (1, 2, 3) */
} rt_upscale_desc;

/* RT_UPSCALE_VERSION of the loaded library. */
int rt_upscale_version(void);

/* Bytes of device scratch rt_upscale_async needs for a lo_width x lo_height
 * low-resolution frame: 48 * w * h; 0 for a frame size out of range. */
size_t rt_upscale_scratch_bytes(int lo_width, int lo_height);

/* Enqueue the pass on `stream` (a hipStream_t, NULL = the context's own): two
 * launches.  scratch: rt_upscale_scratch_bytes(lo_width, lo_height) bytes of
 * device memory, 16-byte aligned, the caller's until the work is done.
 * RT_ERR_INVALID before any HIP call, and before the context is read, for a
 * NULL context, desc or pointer (stage may be NULL; the albedos only with
 * RT_UPSCALE_NO_ALBEDO), a size, spp or option out of range or NaN, an
 * unknown flag, reserved != 0, a NULL or misaligned scratch, out, stage or
 * scratch overlapping each other or any buffer the pass reads, and rays.eye
 * not bitwise equal to lo_view.eye.  Does not synchronise. */
int rt_upscale_async(rt_context *ctx, const rt_upscale_desc *desc, void *scratch, void *stream);

/* Synchronous convenience: the desc's pointers are HOST pointers; the pass
 * runs in device buffers and scratch of its own on the context's stream;
 * *kernel_ms (may be NULL) receives the hipEvent time of its launches. */
int rt_upscale(rt_context *ctx, const rt_upscale_desc *host, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_UPSCALE_H */
