/*
 * rt_temporal.h -- temporal accumulation with camera reprojection
 * (librtow_temporal.so, which links librtow.so): the stage interactive path
 * tracers put next to the spatial filter.  The previous frame's result is
 * looked up through the previous camera at the world position of this frame's
 * first hit (rt_aov.h), history that belongs to another surface is rejected,
 * and what is left is blended with the new frame, so that a slowly moving
 * camera gathers samples over frames instead of starting from nothing.  The
 * reference has no such step.
 *
 * Semantics
 *  - Frame.  A whole assembled frame of width x height pixels, row-major,
 *    row 0 = top row; a banded rank share is not a valid input (rt_denoise.h).
 *    The scene is static; only the camera moves.
 *  - Inputs.  cur: W*H*3 fp32 sums over spp samples (rt_render_async's beauty
 *    or rt_denoise_async's out).  hits (W*H uint32), position, normal (W*H*3
 *    fp32): the sums rt_aov_async writes for THIS frame.  history_in: what the
 *    previous frame's pass wrote as history_out, or NULL; prev: the view
 *    (rt_temporal_view) of the camera that frame was rendered with.
 *  - History.  rt_temporal_history_bytes(W, H) = 48 * W * H bytes: three
 *    planes of W*H float4, plane-major, each row-major:
 *      plane 0  (r, g, b, len)   the accumulated mean and the history length in frames
 *      plane 1  (Px, Py, Pz, sky ? 1 : 0)
 *      plane 2  (nx, ny, nz, 0)
 *    Planes 1 and 2 are this frame's prepared guides: what the next frame
 *    validates its taps against.
 *  - Output.  out (may be NULL; may be cur itself): W*H*3 fp32 in the sum
 *    contract (accumulated mean x spp), so rt_tonemap_async with the same spp
 *    works on it unchanged.
 *  - View.  A world point X maps to continuous pixel coordinates of a frame
 *    (pixel (col, row)'s centre is (col, row)), all fp32:
 *      q = X - eye;  w = pw.q;  x = (px.q) / w - x0;  y = (py.q) / w - y0
 *    A dot product a.b is (ax*bx + ay*by) + az*bz everywhere below too.
 *    rt_temporal_view_from_camera computes the view in fp64 from the fp32
 *    rt_camera fields and rounds each number once: with c = corner - eye,
 *    n = horiz x vert: pw = n / (c.n); A_h = (vert x n) / (horiz.(vert x n)),
 *    A_v = (n x horiz) / (vert.(n x horiz)), so that a ray through the frame
 *    coordinates (fs, ft) of camera_dir has fs = (A_h.q)/w - A_h.c and ft
 *    likewise; at the pixel centre (u1 = u2 = 0.5)
 *      RT_CAMERA_CPU:  x = fs*(W-1) - 0.5,  y = (H - 0.5) - ft*(H-1)
 *      RT_CAMERA_GPU:  x = fs,              y = ft
 *    and the scales are folded into px, py, x0, y0.  A lens is ignored: the
 *    projection goes through eye, the mean of the lens samples.
 *  - Per pixel p = (i, j), h = hits, S = float(spp), all fp32, in this order:
 *    1. Prepare, as rt_denoise.h:
 *         sky = (h == 0);  c = cur / S
 *         n = normal_sum / float(h); nn = n.n; n = nn > 0 ? n / sqrt(nn) : 0
 *         P = position_sum / float(h)
 *         sky: n = P = 0
 *    2. No history (history_in == NULL, or sky): len' = 1, m = c.  A sky
 *       pixel carries no position, so it restarts every frame; its estimate
 *       is nearly noise-free anyway.
 *    3. Reproject with prev: q, w, x, y as under "View";
 *         ok = (w > 0) && (x > -1) && (x < float(W)) && (y > -1) && (y < float(H))
 *       (false for NaN);  xf = floor(x), fx = x - xf, xi = int(xf); likewise
 *       yf, fy, yi;  d2 = q.q;  pt2 = plane_tol * plane_tol.
 *    4. Gather, when ok, the four taps (dy, dx) = (0,0), (0,1), (1,0), (1,1)
 *       in that order, t = (xi + dx, yi + dy).  A tap is skipped when t is
 *       outside the frame; when the history's sky flag at t is non-zero;
 *       unless e*e <= pt2*d2, with D = P_t - P and e = n.D (the test is left
 *       out entirely for plane_tol = +infinity); unless g >= normal_cos, with
 *       g = n.n_t (left out for normal_cos = -1).  Otherwise
 *         b = (dx ? fx : 1 - fx) * (dy ? fy : 1 - fy)
 *         sw += b;  sc += b * rgb_t (per channel);  sl += b * len_t
 *       Every sum starts from +0.
 *    5. Blend.  valid = ok && sw > 0.  When valid:
 *         hist = sc / sw;  hl = sl / sw
 *         t = hl + 1;  M = float(max_len);  len' = t < M ? t : M
 *         a = 1 / len';  m = hist + (c - hist) * a
 *       else len' = 1, m = c.
 *    6. Write history_out: plane 0 (m, len'), plane 1 (P, sky ? 1 : 0),
 *       plane 2 (n, 0); and out_c = m_c * S when out != NULL.
 *  - Arithmetic.  Only + - x / sqrt floor, float <-> int conversion,
 *    comparisons and selects, fp32, round to nearest, denormals kept, no
 *    contraction and no fast-math forms: tests/temporal_ref.py restates it in
 *    numpy float32 and gets the same bits.  Inputs are taken to be finite.
 *  - Options.  A zero field means its default:
 *      max_len     0 -> 2;     1 .. 1024 frames (1 = no accumulation)
 *      plane_tol   0 -> 0.0003;  > 0, +infinity = test off.  The tolerance
 *                              is a fraction of the distance from the previous eye.
 *      normal_cos  0 -> 0.9;   in [-1, 1], -1 = test off
 *    Anything else is RT_ERR_INVALID.  The defaults were tuned on 8-frame
 *    orbits of the final and the five-sphere scene at 128 x 72 (DESIGN.md
 *    11).  The plane tolerance is tight on purpose, see below; at that size
 *    a short history wins, pixels inside a surface gain from a longer one.
 *  - Known limitation.  P is the mean over the samples that hit: in a pixel
 *    that is partly sky, or partly another surface, it lies off the pixel
 *    centre or off every surface, so such a pixel looks its history up a part
 *    of a pixel to one side, frame after frame, and a long history lets a
 *    surface's colour creep over its silhouette.  The tight default plane_tol
 *    keeps most of those taps out; a loose one (0.01) lets them in.
 *  - Known limitation.  The guides are first-hit: what is seen in a mirror or
 *    through glass is validated against the mirror's or the glass's own
 *    surface, so reflections and refractions lag behind a moving camera by up
 *    to max_len frames.  There is no colour clamp in this version.
 *    rt_guides.h gives buffers of the same layout that follow such paths to
 *    what is seen (its position is the real surface's, not the virtual
 *    image's: DESIGN.md 14 says what this pass would need).
 *
 * A pass is serialised with the renders, feature passes, filters and scene
 * uploads of its context, on whatever stream it runs; it needs no uploaded
 * scene.  One context, one host thread at a time, as in rt.h.
 */
#ifndef RTOW_RT_TEMPORAL_H
#define RTOW_RT_TEMPORAL_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_TEMPORAL_VERSION 1

typedef struct {          /* world point -> continuous pixel coordinates of a frame, */
  float eye[3];           /* pixel (col,row) centre = (col,row), row 0 = top        */
  float px[3], py[3], pw[3];
  float x0, y0;
} rt_temporal_view;

typedef struct {
  int32_t width, height, spp;      /* whole frame 1..32768; spp >= 1 scales cur/out only */
  int32_t max_len;                 /* 0 = default, else 1..1024 frames (1 = no accumulation) */
  float plane_tol;                 /* 0 = default, else > 0; +inf = plane test off */
  float normal_cos;                /* 0 = default, else in [-1, 1]; -1 = normal test off */
  int32_t reserved[2];             /* 0 */
  rt_temporal_view prev;           /* the view history_in was made with (ignored when history_in == NULL) */
  /* DEVICE pointers (async) or HOST pointers (sync) */
  const float *cur;                /* W*H*3 sums over spp: rt_render's beauty or rt_denoise's out */
  const uint32_t *hits; const float *position, *normal;   /* rt_aov sums of THIS frame */
  const void *history_in;          /* rt_temporal_history_bytes(W,H), or NULL = no history */
  void *history_out;               /* same size; must not overlap history_in */
  float *out;                      /* W*H*3 sums (mean x spp); may be == cur; may be NULL */
} rt_temporal_desc;

/* RT_TEMPORAL_VERSION of the loaded library. */
int rt_temporal_version(void);

/* The view of `cam` for a width x height frame (see "View").  Host code, no
 * HIP call.  RT_ERR_INVALID for a NULL pointer, a size outside 1 .. 32768,
 * RT_CAMERA_CPU with width < 2 or height < 2 (its frame coordinates divide by
 * W-1 and H-1), an unknown model, and a non-finite or degenerate camera
 * (c.n == 0, or a zero denominator); *out is then left alone. */
int rt_temporal_view_from_camera(const rt_camera *cam, int width, int height, rt_temporal_view *out);

/* Bytes of one history buffer: 48 * W * H; 0 for a frame size out of range. */
size_t rt_temporal_history_bytes(int width, int height);

/* Enqueue the pass on `stream` (a hipStream_t, NULL = the context's own): one
 * launch, no scratch.  history_in and history_out are 16-byte aligned device
 * memory.  RT_ERR_INVALID before any HIP call, and before the context is
 * read, for a NULL context, desc or pointer (history_in and out may be NULL),
 * a size, spp or option out of range or NaN, reserved != 0, a misaligned
 * history, history_out overlapping any buffer the pass reads or out, and out
 * overlapping history_in.  Does not synchronise. */
int rt_temporal_async(rt_context *ctx, const rt_temporal_desc *desc, void *stream);

/* Synchronous convenience: the desc's pointers are HOST pointers (no
 * alignment asked); the pass runs in device buffers of its own on the
 * context's stream; *kernel_ms (may be NULL) receives the hipEvent time of
 * its launch. */
int rt_temporal(rt_context *ctx, const rt_temporal_desc *host, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_TEMPORAL_H */
