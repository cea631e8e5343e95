// rt_trace.hip -- closest-hit queries for the caller's own ray batches
// (include/rt_trace.h, librtow_trace.so): ray i of a batch traced to its first
// hit, and the sphere, the distance, the hit point and the shading normal
// written.  The gfx950 kernel and the host half are csrc/rt_ray_batch.h's
// without a limit (LIMIT false: no t_max, no blocked, nothing of them compiled);
// rt_segment.hip is the same header with one.
//
// A library of its own: librtow.so's device code stays byte for
// byte what the committed PMC summaries were collected on.  The context stays
// opaque here; rt_api.cpp's rt_internal_scene_begin / rt_internal_frame_end
// (csrc/rt_frame.h) give the pass the scene's kernel arguments without a
// camera and keep it serialised with the context's renders.
#include <hip/hip_runtime.h>

#include "rt_trace.h"
#include "rt_ray_batch.h"

static_assert(RT_TRACE_MISS == rtk::kRayMiss && RT_TRACE_INVALID == rtk::kRayInvalid, "the kernel's ids");

namespace {

// the public structs as a batch; NULL where one of them is
const ray_batch *batch_of(const rt_trace_rays *r, const rt_trace_hits *h, ray_batch &b) {
  if (!r || !h) return nullptr;
  b = {r->n, {r->origin, r->direction, nullptr}, {nullptr, h->id, h->t, h->position, h->normal}};
  return &b;
}

}  // namespace

extern "C" {

int rt_trace_version(void) { return RT_TRACE_VERSION; }

int rt_trace_async(rt_context *c, const rt_trace_rays *dev, const rt_trace_hits *out, uint32_t flags, void *stream) {
  ray_batch b;
  return batch_async<false>(c, batch_of(dev, out, b), flags, stream);
}

int rt_trace(rt_context *c, const rt_trace_rays *host, const rt_trace_hits *out, uint32_t flags, double *kernel_ms) {
  ray_batch b;
  return batch_sync<false>(c, batch_of(host, out, b), flags, kernel_ms);
}

}  // extern "C"
