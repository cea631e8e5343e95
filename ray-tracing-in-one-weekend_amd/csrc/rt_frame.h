// rt_frame.h -- internal: how a pass of a context starts and ends on a stream,
// and the host helpers its passes share.  A pass over the context's scene (the
// render in rt_api.cpp, the first-hit feature pass in rt_aov.hip /
// librtow_aov.so, the chain-following ones in rt_guides.hip /
// librtow_guides.so and rt_route.hip / librtow_route.so) begins with
// rt_internal_frame_begin, the pass over the caller's own rays (rt_trace.hip /
// librtow_trace.so) with rt_internal_scene_begin; an image-space pass
// that only shares the context's ordering (the denoiser in rt_denoise.hip /
// librtow_denoise.so, temporal accumulation in rt_temporal.hip /
// librtow_temporal.so, the resolve in rt_resolve.hip / librtow_resolve.so,
// upsampling in rt_upscale.hip / librtow_upscale.so) with
// rt_internal_pass_begin; what those share beyond this header is in rt_post.h
// and rt_reproject.h, and what the traced feature passes share (device
// and host) in rt_trace_pass.h and rt_chain.h.  The helpers: hip_fail /
// RT_HIP, the traced passes' cut of a frame's samples into launches
// (rt_samples_per_launch, rt_sample_ranges: no HIP in them, so that
// tools/host_sanitize.cpp checks them), rt_pass_scope, rt_device_buf and
// rt_sync_pass, the one host sequence of the synchronous rt_aov / rt_denoise /
// rt_temporal / rt_resolve / rt_upscale / rt_guides / rt_route.  Not
// installed; rt_context stays opaque outside rt_api.cpp, so the other
// libraries get what they need through rt_frame_setup.
#ifndef RTOW_RT_FRAME_H
#define RTOW_RT_FRAME_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <utility>

#include "rt_layout.h"

struct rt_frame_setup {
  rtk::kparams kp;        // fill_kparams for (cam, params): scene, current grid, camera, frame; out = nullptr
  hipStream_t stream;     // the stream the pass runs on (the caller's, or the context's own)
  int grid;               // the layer-grid walk serves RT_FLAG_ACCEL_BVH for these flags
  int placement;          // rtk::kGrid*: where a launch keeps that grid
  size_t lds_bytes;       // dynamic LDS of a launch that walks it
  double launch_samples;  // RT_OPT_LAUNCH_SAMPLES
  hipEvent_t ev0, ev1;    // the context's timing events (synchronous callers)
  uint32_t n_spheres;     // the scene's spheres (rt_bounce checks a ray's `from` against it)
};

// rt_params.seed as the kernels take it (kparams seed32): the one definition,
// for the render's arguments (rt_api.cpp fill_kparams) and rt_bounce_rays.seed
inline uint32_t rt_seed32(uint64_t seed) { return (uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x9E3779B9u); }

extern "C" {

void rt_internal_set_hip_error(int e);

// The argument checks of rt_render_async without its buffer: RT_ERR_INVALID
// or RT_ERR_NO_SCENE, else RT_OK.  No HIP call.
int rt_internal_frame_check(const rt_context *ctx, const rt_camera *cam, const rt_params *params);

// What every pass does before its launches: hipSetDevice, the wait on the
// previous pass of this context when that ran on another stream, the
// RT_OPT_GRID_FIT refit of the layer grid for this frame geometry (enqueued
// on the stream) and fill_kparams.  stream NULL = the context's own.
// Arguments as checked by rt_internal_frame_check.
int rt_internal_frame_begin(rt_context *ctx, const rt_camera *cam, const rt_params *params, void *stream,
                            rt_frame_setup *out);

// rt_internal_frame_begin without a camera, for a pass that traces the
// caller's own rays (rt_trace.hip / librtow_trace.so): hipSetDevice, the wait
// on the previous pass, the walk and grid placement for `flags` over the grid
// the context currently holds (the builder's or the last frame's fit: without
// a frame geometry there is no RT_OPT_GRID_FIT refit) and the scene's and the
// grid's kernel arguments; the camera and frame fields of out->kp stay zero.
// RT_ERR_INVALID for a NULL argument, RT_ERR_NO_SCENE before rt_scene_upload
// (rt_internal_scene_check: the same two without a HIP call).  Ends with
// rt_internal_frame_end like the others.
int rt_internal_scene_check(const rt_context *ctx);
int rt_internal_scene_begin(rt_context *ctx, uint32_t flags, void *stream, rt_frame_setup *out);

// The same for a pass that reads no scene (the image-space passes): hipSetDevice
// and the wait on the context's previous pass; of *out only stream, ev0 and
// ev1 are set, the rest is zero.  RT_ERR_INVALID for a NULL argument, no HIP
// call before that.  Ends with rt_internal_frame_end like the others.
int rt_internal_pass_begin(rt_context *ctx, void *stream, rt_frame_setup *out);

// After the pass's last launch (also when enqueuing failed half way): records
// the context's ev_done on the stream, so that renders, feature passes and
// rt_scene_upload of one context stay serialised.
int rt_internal_frame_end(rt_context *ctx, hipStream_t stream);

}  // extern "C"

// A failed HIP call's status; rt_last_hip_error reports e
inline int hip_fail(hipError_t e) {
  rt_internal_set_hip_error((int)e);
  return RT_ERR_HIP;
}

#define RT_HIP(call)                           \
  do {                                         \
    hipError_t _e = (call);                    \
    if (_e != hipSuccess) return hip_fail(_e); \
  } while (0)

// The frame's 8x8 tiles (one wave each) and its blocks of kWavesPerBlock tiles
inline long long rt_frame_tiles(const rt_params *prm) {
  return (long long)((prm->width + rtk::kTile - 1) / rtk::kTile) * ((prm->local_rows + rtk::kTile - 1) / rtk::kTile);
}
inline long long rt_frame_blocks(const rt_params *prm) {
  return (rt_frame_tiles(prm) + rtk::kWavesPerBlock - 1) / rtk::kWavesPerBlock;
}

// How a traced feature pass (rt_trace_pass.h) cuts a frame's spp samples per
// pixel into launches: `per` samples of every pixel per launch, about
// launch_samples (RT_OPT_LAUNCH_SAMPLES) samples of the frame_px pixels at
// most, at least one; at most kMaxLaunches launches.  No HIP in either.
inline long long rt_samples_per_launch(int spp, double frame_px, double launch_samples) {
  const long long per = (long long)std::min((double)std::max(spp, 1), std::floor(launch_samples / frame_px));
  return std::max({per, 1LL, ((long long)spp + rtk::kMaxLaunches - 1) / rtk::kMaxLaunches});
}
// f(s_lo, s_cnt) for the ranges in ascending order, until one fails.  spp = 0:
// one range (0, 0), a launch that only initialises.
template <class F>
int rt_sample_ranges(int spp, long long per, F f) {
  for (long long s0 = 0; s0 == 0 || s0 < spp; s0 += per) {
    const int r = f((int)s0, (int)std::min<long long>(per, spp - s0));
    if (r != RT_OK) return r;
  }
  return RT_OK;
}

// The flags of a pass over the scene without a camera (rt_pass_scope's third
// constructor: rt_internal_scene_begin)
struct rt_scene_flags {
  uint32_t flags;
};

// How rt_trace cuts a batch of n rays into launches: ascending ranges of
// launch_samples (RT_OPT_LAUNCH_SAMPLES) rays at most, at least one; at most
// kMaxLaunches launches.  No HIP.
inline unsigned long long rt_rays_per_launch(unsigned long long n, double launch_samples) {
  const double per = std::floor(std::min(std::max(launch_samples, 1.0), (double)std::max(n, 1ULL)));
  return std::max((unsigned long long)per, (n + rtk::kMaxLaunches - 1) / rtk::kMaxLaunches);
}

// One pass on a stream: begins it (cam NULL: rt_internal_pass_begin, else
// rt_internal_frame_begin; with rt_scene_flags: rt_internal_scene_begin) and,
// exactly when the begin got as far as a stream,
// ends it with rt_internal_frame_end -- in end(), or on leaving the scope: a
// pass that fails after enqueuing some of its work still has ev_done recorded
// behind that work, so that the context's next pass on another stream, and
// rt_scene_upload before it frees the scene, wait for it too.
struct rt_pass_scope {
  rt_frame_setup fs;
  int status;  // of the begin
  rt_pass_scope(rt_context *c, const rt_camera *cam, const rt_params *prm, void *stream) : c_(c) {
    std::memset(&fs, 0, sizeof fs);
    status = cam ? rt_internal_frame_begin(c, cam, prm, stream, &fs) : rt_internal_pass_begin(c, stream, &fs);
  }
  rt_pass_scope(rt_context *c, rt_scene_flags sf, void *stream) : c_(c) {
    std::memset(&fs, 0, sizeof fs);
    status = rt_internal_scene_begin(c, sf.flags, stream, &fs);
  }
  rt_pass_scope(const rt_pass_scope &) = delete;
  ~rt_pass_scope() { (void)end(RT_OK); }
  // ends the pass; r, the status of its launches, with the end's folded in (the first error wins)
  int end(int r) {
    if (!fs.stream || ended_) return r;
    ended_ = true;
    const int re = rt_internal_frame_end(c_, fs.stream);
    return r != RT_OK ? r : re;
  }

 private:
  rt_context *c_;
  bool ended_ = false;
};

// A device buffer and its capacity in elements, freed with its owner (move
// only).  grow(n): nothing when it already holds n elements, else the old
// buffer is freed and a new one allocated (the contents are not kept); after
// a failed allocation it holds nothing.
template <class T>
struct rt_device_buf {
  T *p = nullptr;
  size_t cap = 0;
  rt_device_buf() = default;
  rt_device_buf(rt_device_buf &&o) noexcept { *this = std::move(o); }
  rt_device_buf &operator=(rt_device_buf &&o) noexcept {  // (o then frees what *this held)
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~rt_device_buf() { (void)hipFree(p); }
  hipError_t grow(size_t n) {
    if (n <= cap) return hipSuccess;
    *this = rt_device_buf();
    const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
};

// One part of a synchronous pass's staging.
struct rt_sync_part {
  size_t bytes;    // 0: the part is left out (its device address is null)
  const void *up;  // the host array copied in before the launches; null: none
  void *down;      // the host array copied out after them; null: none
};

// A synchronous pass on the context's own stream, from host arrays to host
// arrays: one device allocation cut into the parts (256-byte aligned), the
// uploads, enqueue(dev, fs) -- dev[k] the device address of part k; it
// enqueues the launches on fs.stream and returns their status -- between the
// context's timing events, the wait, the downloads and *kernel_ms (0 unless
// all of it succeeded).  The caller validates the arguments first; the first
// error wins.  Whatever was enqueued, ev_done is recorded behind it
// (rt_pass_scope), and the stream is drained before the allocation is freed,
// also after a failure: the copies and launches read it and the host arrays.
// wait() runs after a successful enqueue, before that drain: rt_aov waits
// launch by launch there.
// rt_sync_pass_in: the same in a scope the caller began on the context's own
// stream (rt_trace's, which has no camera).
template <size_t N, class Enqueue, class Wait>
int rt_sync_pass_in(rt_pass_scope &ps, const rt_sync_part (&parts)[N], double *kernel_ms, Enqueue enqueue, Wait wait) {
  if (kernel_ms) *kernel_ms = 0.0;
  size_t off[N], total = 0;
  for (size_t k = 0; k < N; ++k) off[k] = total, total += (parts[k].bytes + 255) / 256 * 256;
  rt_device_buf<char> stage;  // (freed on leaving, after the drain)
  void *dev[N] = {};
  const rt_frame_setup &fs = ps.fs;
  const auto run = [&]() -> int {
    if (ps.status != RT_OK) return ps.status;
    RT_HIP(stage.grow(total));
    for (size_t k = 0; k < N; ++k) {
      dev[k] = parts[k].bytes ? stage.p + off[k] : nullptr;
      if (dev[k] && parts[k].up)
        RT_HIP(hipMemcpyAsync(dev[k], parts[k].up, parts[k].bytes, hipMemcpyHostToDevice, fs.stream));
    }
    RT_HIP(hipEventRecord(fs.ev0, fs.stream));
    const int r = enqueue(dev, fs);
    if (r == RT_OK) RT_HIP(hipEventRecord(fs.ev1, fs.stream));
    return r;
  };
  int r = ps.end(run());
  if (r == RT_OK) r = wait();
  if (fs.stream) {
    const hipError_t es = hipStreamSynchronize(fs.stream);
    if (r == RT_OK && es != hipSuccess) r = hip_fail(es);
  }
  if (r != RT_OK) return r;
  float ms = 0.0f;
  RT_HIP(hipEventElapsedTime(&ms, fs.ev0, fs.ev1));
  for (size_t k = 0; k < N; ++k)
    if (dev[k] && parts[k].down) RT_HIP(hipMemcpy(parts[k].down, dev[k], parts[k].bytes, hipMemcpyDeviceToHost));
  if (kernel_ms) *kernel_ms = ms;
  return RT_OK;
}
template <size_t N, class Enqueue, class Wait = int (*)()>
int rt_sync_pass(rt_context *c, const rt_camera *cam, const rt_params *prm, const rt_sync_part (&parts)[N],
                 double *kernel_ms, Enqueue enqueue, Wait wait = [] { return (int)RT_OK; }) {
  rt_pass_scope ps(c, cam, prm, nullptr);  // (sets the device)
  return rt_sync_pass_in(ps, parts, kernel_ms, enqueue, wait);
}

#endif  // RTOW_RT_FRAME_H
