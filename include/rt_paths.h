/*
 * rt_paths.h -- the wavefront loop's device step between two rt_bounce calls
 * (librtow_paths.so, which links librtow.so): what rtow.path_trace does in
 * numpy after every bounce -- multiply the throughput, deposit the rays that
 * missed into the render's fixed-point pixel sums, drop the finished paths,
 * compact the survivors into the next batch and raise the key's depth -- as one
 * step on the device, and the sums' final conversion to the frame.  A loop of
 * rt_bounce_camera_rays, rt_bounce and rt_paths_step with only the step's count
 * (4 bytes) crossing to the host reproduces rt_render bit for bit
 * (rtow.path_trace_device): integer atomics do not depend on
 * order.  The glue every use rt_bounce.h lists needs: direct lighting with
 * rt_segment shadow rays, Russian roulette, per-bounce outputs, path
 * regeneration.  The reference has no such entry; its loop is ray_color's
 * recursion (src/cpu/main.cc:14-30).
 *
 * Semantics of a step over n rays, all fp32, every operation rounded on its own
 * (no fused multiply-add), so that numpy float32 rounds alike
 *  - Ray i brings what rt_bounce just wrote for it (status, id, position,
 *    scatter, attenuation) and what it carried into that call: key = (pix, s,
 *    k), throughput and slot, the index of the pixel sum its sample belongs to,
 *    local to the caller's frame.
 *  - thr' = throughput * attenuation per channel.
 *  - status RT_BOUNCE_MISS and slot < n_slots: for each channel c,
 *    q = (uint32) fminf(fmaxf(thr'_c * 2^shift, 0), 4294967040.f) is added to
 *    sums[3 slot + c] with a 32-bit integer atomic; fmaxf sends a NaN to 0.  For
 *    thr' <= 1 and shift <= 31 this is the render's truncating q(v 2^F)
 *    unchanged.  The sum wraps modulo 2^32.  sums is
 *    accumulated into and never cleared by the step.
 *  - status RT_BOUNCE_MISS and slot >= n_slots: nothing is deposited, and the
 *    other rays are not affected.
 *  - status RT_BOUNCE_SCATTERED: the ray becomes element r(i) of the next
 *    batch, r(i) the number of scattered rays j < i: the compaction is STABLE.
 *    origin = position, direction = scatter, from = id, key = (pix, s, k + 1)
 *    (a plain uint32 add), throughput = thr', slot = slot; every copy is bit
 *    for bit.
 *  - RT_BOUNCE_ABSORBED, RT_BOUNCE_INVALID and every other status value: the
 *    ray is dropped and deposits nothing.
 *  - *count receives the number of scattered rays.  Elements of the next batch
 *    at or beyond it are not written.
 *  - The step knows no max_depth, as rt_bounce knows none: the cap is the
 *    caller's loop.
 *  - Only narrow, truncating sums: the render's dither (spp >= 4096) and its
 *    wide sums (an albedo above 1, with the 2^100 clamp) are not restated, as
 *    in rtow.path_trace.
 *  - The result is a function of the inputs alone: the deposits commute, and
 *    the ranks are global whatever the tile size.  The step is not cut into
 *    several launches (RT_OPT_LAUNCH_SAMPLES does not apply: a ray costs a few
 *    loads and stores here).
 *
 * The pass reads no scene and asks for none: it takes the context only for the
 * ordering, as the image-space passes do.  It is serialised with the renders,
 * feature passes and scene uploads of its context, on whatever stream it runs.
 * One context, one host thread at a time, as in rt.h.
 *
 * Device work: three launches over tiles of rt_paths_tile() rays, ordered by
 * the stream alone -- count (every block counts its tile's scattered rays, and
 * deposits its misses), scan (one block of rt_paths_scan_block() threads turns
 * the tile counts into offsets and writes *count), scatter (every block writes
 * its tile's scattered rays from its offset on).  No kernel waits for another
 * block.
 */
#ifndef RTOW_RT_PATHS_H
#define RTOW_RT_PATHS_H

#include "rt.h"
#include "rt_bounce.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_PATHS_VERSION 1

typedef struct {            /* DEVICE pointers (rt_paths_step_async) or HOST pointers (rt_paths_step) */
  uint64_t n;               /* rays, at most 2^31 - 1                                                 */
  const uint8_t *status;    /* n   : rt_bounce's status                                               */
  const int32_t *id;        /* n   : rt_bounce's id                                                   */
  const float *position;    /* n*3 : rt_bounce's position                                             */
  const float *scatter;     /* n*3 : rt_bounce's scatter                                              */
  const float *attenuation; /* n*3 : rt_bounce's attenuation                                          */
  const uint32_t *key;      /* n*3 : the key the ray carried into rt_bounce                           */
  const float *throughput;  /* n*3 : the throughput it carried                                        */
  const uint32_t *slot;     /* n   : the pixel sum its sample belongs to                              */
  uint64_t n_slots;         /* pixel sums, 3 n_slots <= 2^32 - 1                                      */
  int32_t shift;            /* the render's F, 0 .. 31 (rt_paths_shift)                               */
  int32_t reserved;         /* 0                                                                      */
} rt_paths_in;

typedef struct {            /* DEVICE or HOST pointers like the input                                 */
  uint32_t *sums;           /* 3 n_slots : accumulated into; NULL = no deposit                        */
  float *origin;            /* n*3 : the next batch; each of the six may be NULL = not wanted         */
  float *direction;         /* n*3                                                                    */
  int32_t *from;            /* n                                                                      */
  uint32_t *key;            /* n*3                                                                    */
  float *throughput;        /* n*3                                                                    */
  uint32_t *slot;           /* n                                                                      */
  uint32_t *count;          /* 1   : the rays in the next batch; never NULL                           */
} rt_paths_out;

/* RT_PATHS_VERSION of the loaded library. */
int rt_paths_version(void);

/* The rays per block of the count and scatter kernels, and the threads of the
 * scan kernel's one block: compile-time constants of the library. */
int rt_paths_tile(void);
int rt_paths_scan_block(void);

/* The render's F for narrow sums, 31 - floor(log2 spp), for 1 <= spp < 4096;
 * -1 for spp < 1 and for spp >= 4096, the dithered range this pass does not
 * restate. */
int rt_paths_shift(int32_t spp);

/* Bytes of scratch a step over n rays needs (one uint32 per tile, a multiple
 * of 16 and never 0 for n <= 2^31 - 1; 0 beyond). */
size_t rt_paths_scratch_bytes(uint64_t n);

/* The argument rules of a step, without a context and without a HIP call:
 * RT_ERR_INVALID for a NULL in or out, n > 2^31 - 1, shift outside 0 .. 31,
 * 3 n_slots > 2^32 - 1, reserved != 0, a NULL count, a NULL input when n > 0,
 * and for a forbidden overlap, judged on the byte ranges: no output (sums and
 * count included) may share a byte with another output or with an input of the
 * step.  So the outgoing key, throughput and slot are other arrays than the
 * incoming ones (a caller ping-pongs those three), while origin, direction and
 * from MAY be the very arrays the bounce read: the step does not read them.
 * Else RT_OK. */
int rt_paths_step_check(const rt_paths_in *in, const rt_paths_out *out);

/* Enqueue a step on `stream` (a hipStream_t, NULL = the context's own) through
 * DEVICE pointers.  scratch: rt_paths_scratch_bytes(n) bytes of device memory,
 * 16-byte aligned, the step's own until it has run.  Checked before any HIP
 * call and before the context is read: RT_ERR_INVALID for a NULL ctx, a NULL or
 * misaligned scratch (n > 0) and whatever rt_paths_step_check rejects.  n = 0:
 * *count is set to 0 and nothing else happens.  Does not synchronise. */
int rt_paths_step_async(rt_context *ctx, const rt_paths_in *dev, const rt_paths_out *dev_out, void *scratch,
                        void *stream);

/* Synchronous convenience: the same step from HOST arrays through device
 * buffers and a scratch of its own; *kernel_ms (may be NULL) receives the
 * hipEvent time of the launches.  The same checks, on the host ranges.  sums is
 * read and written back; of the next batch the elements beyond *count keep
 * what the host arrays held. */
int rt_paths_step(rt_context *ctx, const rt_paths_in *host, const rt_paths_out *host_out, double *kernel_ms);

/* The render's final conversion: frame[i] = (float) sums[i] * 2^-shift for
 * 3 n_slots elements.  RT_ERR_INVALID, before any HIP call, for a NULL ctx,
 * shift outside 0 .. 31, 3 n_slots > 2^32 - 1, a NULL sums or frame when
 * n_slots > 0, and for frame sharing a byte with sums.  n_slots = 0: RT_OK,
 * nothing is launched.  The asynchronous form takes DEVICE pointers and does
 * not synchronise; the synchronous one takes HOST pointers. */
int rt_paths_frame_async(rt_context *ctx, const uint32_t *sums, uint64_t n_slots, int32_t shift, float *frame,
                         void *stream);
int rt_paths_frame(rt_context *ctx, const uint32_t *sums, uint64_t n_slots, int32_t shift, float *frame,
                   double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_RT_PATHS_H */
