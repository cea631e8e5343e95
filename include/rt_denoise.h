/*
 * rt_denoise.h -- a guided a-trous denoiser for low-sample frames
 * (librtow_denoise.so, which links librtow.so): the edge-avoiding a-trous
 * wavelet filter of Dammertz, Sewtz, Hanika and Lensch (HPG 2010), guided by
 * the first-hit normal and position of rt_aov.h and run on albedo-demodulated
 * colour.  The reference has no such step; it is what turns "16 spp + guide
 * buffers" into a preview frame without a trip through the host.
 *
 * Semantics
 *  - Frame.  The filter runs on a whole assembled frame of width x height
 *    pixels, row-major, row 0 = top row.  A banded rank share (rt_params with
 *    band_stride > 1) is not a valid input: its neighbouring rows are not
 *    neighbours in the image.  Multi-GPU callers denoise after the gather.
 *  - Inputs.  beauty: W*H*3 fp32 sums over spp samples, as rt_render_async
 *    writes them.  hits (W*H uint32), position, normal, albedo (W*H*3 fp32):
 *    the sums rt_aov_async writes for the same parameters.  depth and id are
 *    not used.
 *  - Output.  W*H*3 fp32 in the same sum contract (filtered mean x spp), so
 *    rt_tonemap_async with the same spp works on it unchanged.  out may be
 *    the beauty buffer itself; it must not overlap any other input or the
 *    scratch.
 *  - Prepare, per pixel, h = hits, S = float(spp), all fp32, in this order:
 *      sky = (h == 0)
 *      a_c = (albedo_sum_c + float(spp - h)) / S      (a miss counts as albedo 1)
 *      m_c = a_c > 1e-3f ? a_c : 1e-3f
 *      u_c = (beauty_c / S) / m_c
 *      n   = normal_sum / float(h); nn = n.n; n = nn > 0 ? n / sqrt(nn) : 0
 *      P   = position_sum / float(h)
 *      sky: n = P = 0
 *    A dot product a.b is (ax*bx + ay*by) + az*bz everywhere below too.
 *  - Iteration i = 0 .. iterations-1, step s = 2^i.  Output pixel p gathers
 *    the 25 taps q = p + s*(dx, dy), dy = -2..2 (outer loop), dx = -2..2
 *    (inner loop), in that order; taps outside the frame are skipped.
 *      w     = ((k[dx]*k[dy] * w_n) * w_p) * w_c,  k = (1, 4, 6, 4, 1) / 16
 *      u'(p) = (sum of w*u(q)) / (sum of w), per channel
 *    Both sums are added in tap order starting from +0.  For the centre tap
 *    q == p the three edge weights are 1, so w = k0*k0 = 36/256 exactly and
 *    the sum of weights is never 0.  For q != p:
 *      w_n: 1 when p and q are both sky, 0 when exactly one is; else
 *           x = n_p.n_q; x = x > 0 ? x : 0; then x = x*x, normal_power times
 *           (6 squarings: the exponent 64).
 *      w_p: 1 for a sky-sky pair; else D = P_q - P_p, dd = D.D; dd > 0:
 *           x = 1 - (|n_p.D| / sqrt(dd)) / sigma_plane; w_p = x > 0 ? x : 0;
 *           dd == 0: 1.  |n_p.D| / |D| is the sine of the angle between the
 *           offset and p's tangent plane: scale-free, no camera needed.
 *           sigma_plane = +infinity gives w_p = 1 (the term switched off).
 *      w_c: e = u_p - u_q per channel, d = (er*er + eg*eg) + eb*eb,
 *           w_c = 1 / (1 + d / (sg*sg)) with sg = sigma_color * 2^-i; switched
 *           off: w_c = 1.
 *  - Finish (fused into the last iteration): out_c = (u_c * m_c) * S.
 *  - Arithmetic.  Only + - x / sqrt, comparisons and selects, fp32, round to
 *    nearest, denormals kept, no contraction and no fast-math forms: a numpy
 *    float32 restatement that does the same operations in the same order
 *    gets the same bits (tests/denoise_ref.py), and the result is a function
 *    of the arguments only -- the promise the beauty and the feature sums
 *    make.  Inputs are taken to be finite.
 *  - Options.  A zero field of rt_denoise_desc means its default, as 0 does
 *    in rt_context_set_option:
 *      iterations    0 -> 5;    1 .. 8
 *      normal_power  0 -> 6;    1 .. 10 squarings; -1 = none (w_n = max(0, n_p.n_q))
 *      sigma_plane   0 -> 0.5;  > 0, +infinity = term off
 *      sigma_color   0 -> 0.15;  > 0; -1 = term off
 *    Anything else is RT_ERR_INVALID.  The defaults were tuned on 16-spp
 *    frames of the final and the five-sphere scene against 4096-spp renders
 *    (DESIGN.md 10).
 *  - Known limitation.  The guides are first-hit: detail seen through glass
 *    or in a mirror has smooth guides, and only w_c protects it.  rt_guides.h
 *    gives buffers of the same layout that follow such paths to what is seen.
 *
 * A pass is serialised with the renders, feature passes and scene uploads of
 * its context, on whatever stream it runs; it needs no uploaded scene.  One
 * context, one host thread at a time, as in rt.h.
 */
#ifndef RTOW_RT_DENOISE_H
#define RTOW_RT_DENOISE_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_DENOISE_VERSION 1

typedef struct {
  int32_t width, height;    /* the whole frame, 1 .. 32768 each */
  int32_t spp;              /* samples behind the sums, >= 1 */
  int32_t iterations;       /* 0 = default (5), else 1 .. 8 */
  int32_t normal_power;     /* 0 = default (6), else 1 .. 10 squarings, -1 = none */
  float sigma_plane;        /* 0 = default (0.5), else > 0 (+infinity = off) */
  float sigma_color;        /* 0 = default (0.15), else > 0, -1 = off */
  int32_t reserved;         /* 0 */
  /* DEVICE pointers (rt_denoise_async) or HOST pointers (rt_denoise), none NULL */
  const float *beauty;      /* W*H*3 : rt_render sums                  */
  const uint32_t *hits;     /* W*H   : rt_aov hits                     */
  const float *position;    /* W*H*3 : rt_aov position sums            */
  const float *normal;      /* W*H*3 : rt_aov normal sums              */
  const float *albedo;      /* W*H*3 : rt_aov albedo sums              */
  float *out;               /* W*H*3 : filtered sums; may be == beauty */
} rt_denoise_desc;

/* RT_DENOISE_VERSION of the loaded library. */
int rt_denoise_version(void);

/* Bytes of device scratch rt_denoise_async needs for a width x height frame:
 * the packed guides (2 x 16 B per pixel) and two colour planes (16 B per pixel
 * each).  0 for a frame size out of range. */
size_t rt_denoise_scratch_bytes(int width, int height);

/* Enqueue the filter on `stream` (a hipStream_t, NULL = the context's own):
 * one prepare launch and one launch per iteration, the last of which writes
 * out.  scratch: rt_denoise_scratch_bytes(width, height) bytes of device
 * memory, 16-byte aligned, the caller's until the work is done.
 * RT_ERR_INVALID for a NULL or out-of-range argument, before any HIP call.
 * Does not synchronise. */
int rt_denoise_async(rt_context *ctx, const rt_denoise_desc *desc, void *scratch, void *stream);

/* Synchronous convenience: the desc's pointers are HOST pointers; the filter
 * runs in device buffers and scratch of its own on the context's stream;
 * *kernel_ms (may be NULL) receives the hipEvent time of its launches. */
int rt_denoise(rt_context *ctx, const rt_denoise_desc *host, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_DENOISE_H */
