// rt_frame.h -- internal: how a pass over the context's scene (the render in
// rt_api.cpp, the first-hit feature pass in rt_aov.hip / librtow_aov.so), or a
// pass that only shares the context's ordering (the denoiser in
// rt_denoise.hip / librtow_denoise.so), starts and ends on a stream.  Not installed; rt_context stays opaque outside
// rt_api.cpp, so the second library gets what it needs through this struct.
#ifndef RTOW_RT_FRAME_H
#define RTOW_RT_FRAME_H

#include <hip/hip_runtime.h>

#include "rt_layout.h"

struct rt_frame_setup {
  rtk::kparams kp;        // fill_kparams for (cam, params): scene, current grid, camera, frame; out = nullptr
  hipStream_t stream;     // the stream the pass runs on (the caller's, or the context's own)
  int grid;               // the layer-grid walk serves RT_FLAG_ACCEL_BVH for these flags
  int placement;          // rtk::kGrid*: where a launch keeps that grid
  size_t lds_bytes;       // dynamic LDS of a launch that walks it
  double launch_samples;  // RT_OPT_LAUNCH_SAMPLES
  hipEvent_t ev0, ev1;    // the context's timing events (synchronous callers)
};

extern "C" {

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

// The same for a pass that reads no scene (librtow_denoise.so): hipSetDevice
// and the wait on the context's previous pass; of *out only stream, ev0 and
// ev1 are set, the rest is zero.  RT_ERR_INVALID for a NULL argument, no HIP
// call before that.  Ends with rt_internal_frame_end like the others.
int rt_internal_pass_begin(rt_context *ctx, void *stream, rt_frame_setup *out);

// After the pass's last launch (also when enqueuing failed half way): records
// the context's ev_done on the stream, so that renders, feature passes and
// rt_scene_upload of one context stay serialised.
int rt_internal_frame_end(rt_context *ctx, hipStream_t stream);

}  // extern "C"

#endif  // RTOW_RT_FRAME_H
