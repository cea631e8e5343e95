// rt_segment.hip -- closest hits within a per-ray distance limit
// (include/rt_segment.h, librtow_segment.so): rt_trace.hip's query with a far
// end per ray.  The gfx950 kernel and the host half are csrc/rt_ray_batch.h's
// with the limit compiled in (LIMIT true); how the limit reaches the walks is
// told there.  With t_max NULL the pass is rt_trace bit for bit.
//
// A library of its own: the nine other code objects stay
// byte for byte what they were.
#include <hip/hip_runtime.h>

#include "rt_segment.h"
#include "rt_ray_batch.h"

static_assert(RT_SEGMENT_MISS == rtk::kRayMiss && RT_SEGMENT_INVALID == rtk::kRayInvalid, "the kernel's ids");

namespace {

// the public structs as a batch; NULL where one of them is
const ray_batch *batch_of(const rt_segment_rays *r, const rt_segment_hits *h, ray_batch &b) {
  if (!r || !h) return nullptr;
  b = {r->n, {r->origin, r->direction, r->t_max}, {h->blocked, h->id, h->t, h->position, h->normal}};
  return &b;
}

}  // namespace

extern "C" {

int rt_segment_version(void) { return RT_SEGMENT_VERSION; }

int rt_segment_async(rt_context *c, const rt_segment_rays *dev, const rt_segment_hits *out, uint32_t flags,
                     void *stream) {
  ray_batch b;
  return batch_async<true>(c, batch_of(dev, out, b), flags, stream);
}

int rt_segment(rt_context *c, const rt_segment_rays *host, const rt_segment_hits *out, uint32_t flags,
               double *kernel_ms) {
  ray_batch b;
  return batch_sync<true>(c, batch_of(host, out, b), flags, kernel_ms);
}

}  // extern "C"
