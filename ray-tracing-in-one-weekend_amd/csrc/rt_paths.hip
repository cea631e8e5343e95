// rt_paths.hip -- the wavefront loop's device step between two rt_bounce calls
// (include/rt_paths.h, librtow_paths.so): throughput, the misses' deposits into
// the fixed-point pixel sums, a stable compaction of the scattered rays into
// the next batch, and the sums' conversion to the frame.  Four small gfx950
// kernels and their host half.
//
// The step is a stream compaction with a deposit, in three launches over tiles
// of kPathsTile rays that only the stream orders:
//   count_kernel    a block counts its tile's scattered rays (ballot + popcount
//                   per wave, one LDS add per wave) into tile[b], and deposits
//                   its tile's misses (integer atomics: any order, same sums);
//   scan_kernel     ONE block turns tile[] into its exclusive prefix in place
//                   and writes *count; it loops when there are more tiles than
//                   threads;
//   scatter_kernel  a block ranks its scattered lanes again (mbcnt within the
//                   wave, the waves' counts through LDS) and writes their
//                   records from tile[b] on.
// No kernel waits for another block: no look-back, no flag in memory, no grid
// sync.  A tile is kPathsRounds rounds of kPathsBlock consecutive rays, lane t
// of round k holding ray b * kPathsTile + k * kPathsBlock + t: a wave's loads
// are runs of 64 records, and the tile's sixteen 64-ray segments are in ray
// order, so the ranks are stable.
//
// The deposit sits in count_kernel (RT_PATHS_DEPOSIT_IN_SCATTER moves it to
// scatter_kernel for a measurement; DESIGN.md 19 has both times).
//
// The arithmetic is the header's, operation by operation with
// -ffp-contract=off: tests/paths_ref.py restates it in numpy float32.  A
// library of its own: the eleven other code objects stay byte
// for byte what they were.  It includes rt_post.h for the address space, not
// rt_device.h: none of the render's device helpers, no turn table.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "rt_frame.h"
#include "rt_paths.h"
#include "rt_post.h"

namespace rtk {

constexpr int kPathsBlock = 256;                           // threads of a count / scatter block
constexpr int kPathsWaves = kPathsBlock / 64;              // its waves
constexpr int kPathsRounds = 4;                            // rays per thread
constexpr int kPathsTile = kPathsBlock * kPathsRounds;     // rays per block
constexpr int kPathsSegments = kPathsWaves * kPathsRounds; // 64-ray segments of a tile, in ray order
constexpr int kPathsScanBlock = 1024;                      // threads of the scan's one block
constexpr int kPathsScanWaves = kPathsScanBlock / 64;
constexpr uint32_t kNoRay = 0x100u;                        // a lane past the batch: no status byte has this value

struct paths_params {
  // what rt_bounce wrote, and what the rays carried into it
  const uint8_t *status;
  const int32_t *id;
  const float *position, *scatter, *attenuation;
  const uint32_t *key;
  const float *throughput;
  const uint32_t *slot;
  // the sums and the next batch; NULL: not wanted
  uint32_t *sums;
  float *origin, *direction;
  int32_t *from;
  uint32_t *okey;
  float *othroughput;
  uint32_t *oslot;
  uint32_t *count;
  uint32_t *tile;  // scratch: a tile's count, then its offset
  uint32_t n, n_slots, n_tiles;
  float scale;  // 2^shift
};

// thr' = throughput * attenuation of ray i
__device__ __forceinline__ void throughput_of(const paths_params &a, size_t o3, float &r, float &g, float &b) {
  const RT_GLOBAL float *gt = as_global(a.throughput) + o3;
  const RT_GLOBAL float *ga = as_global(a.attenuation) + o3;
  r = gt[0] * ga[0];
  g = gt[1] * ga[1];
  b = gt[2] * ga[2];
}

// the render's q(v 2^F), kept inside uint32 for any v: a NaN and a negative give 0
__device__ __forceinline__ uint32_t fixed_of(float v, float scale) {
  return (uint32_t)__builtin_fminf(__builtin_fmaxf(v * scale, 0.0f), 4294967040.0f);
}

// a missed ray's sample radiance into its pixel sum
__device__ __forceinline__ void deposit(const paths_params &a, uint32_t i) {
  const uint32_t slot = as_global(a.slot)[i];
  if (slot >= a.n_slots) return;
  float r, g, b;
  throughput_of(a, 3 * (size_t)i, r, g, b);
  RT_GLOBAL uint32_t *acc = as_global(a.sums) + 3 * (size_t)slot;
  __hip_atomic_fetch_add(acc + 0, fixed_of(r, a.scale), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(acc + 1, fixed_of(g, a.scale), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(acc + 2, fixed_of(b, a.scale), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the status of this lane's ray of round k, kNoRay past the batch, and the ray's index
__device__ __forceinline__ uint32_t status_of(const paths_params &a, int k, uint32_t &i) {
  i = (uint32_t)blockIdx.x * (uint32_t)kPathsTile + (uint32_t)(k * kPathsBlock) + (uint32_t)threadIdx.x;
  return i < a.n ? (uint32_t)as_global(a.status)[i] : kNoRay;
}

template <bool DEPOSIT>
__global__ __launch_bounds__(kPathsBlock) void count_kernel(const paths_params a) {
  __shared__ uint32_t s_total;
  if (threadIdx.x == 0) s_total = 0u;
  __syncthreads();
  uint32_t mine = 0u;  // this wave's scattered rays
#pragma unroll
  for (int k = 0; k < kPathsRounds; ++k) {
    uint32_t i;
    const uint32_t st = status_of(a, k, i);
    mine += (uint32_t)__builtin_popcountll(__ballot(st == RT_BOUNCE_SCATTERED));
    if (DEPOSIT && st == RT_BOUNCE_MISS) deposit(a, i);
  }
  if ((threadIdx.x & 63u) == 0u) atomicAdd(&s_total, mine);
  __syncthreads();
  if (threadIdx.x == 0) as_global(a.tile)[blockIdx.x] = s_total;
}

// One block: tile[] becomes its exclusive prefix, *count its total.  Every
// thread walks the same number of rounds, so the barriers are uniform.
__global__ __launch_bounds__(kPathsScanBlock) void scan_kernel(const paths_params a) {
  __shared__ uint32_t s_wave[kPathsScanWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  RT_GLOBAL uint32_t *tile = as_global(a.tile);
  uint32_t carry = 0u;  // the tiles before this round
  for (uint32_t t0 = 0u; t0 < a.n_tiles; t0 += (uint32_t)kPathsScanBlock) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t c = t < a.n_tiles ? tile[t] : 0u;
    uint32_t inc = c;  // the inclusive prefix within the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t v = __shfl_up(inc, d);
      if (lane >= (uint32_t)d) inc += v;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < kPathsScanWaves; ++w) {
      const uint32_t v = s_wave[w];
      all += v;
      before += (uint32_t)w < wave ? v : 0u;
    }
    if (t < a.n_tiles) tile[t] = carry + before + (inc - c);
    carry += all;
    __syncthreads();  // s_wave is written again
  }
  if (threadIdx.x == 0) *as_global(a.count) = carry;
}

__device__ __forceinline__ void copy3(float *dst, size_t r3, const float *src, size_t o3) {
  if (dst) {
    const RT_GLOBAL float *s = as_global(src) + o3;
    RT_GLOBAL float *d = as_global(dst) + r3;
    d[0] = s[0], d[1] = s[1], d[2] = s[2];
  }
}

template <bool DEPOSIT>
__global__ __launch_bounds__(kPathsBlock) void scatter_kernel(const paths_params a) {
  __shared__ uint32_t s_seg[kPathsSegments];  // segment k * kPathsWaves + wave: its scattered rays
  const uint32_t wave = threadIdx.x >> 6;
  uint32_t st[kPathsRounds], idx[kPathsRounds], rank[kPathsRounds];
#pragma unroll
  for (int k = 0; k < kPathsRounds; ++k) {
    st[k] = status_of(a, k, idx[k]);
    const unsigned long long m = __ballot(st[k] == RT_BOUNCE_SCATTERED);
    rank[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if ((threadIdx.x & 63u) == 0u) s_seg[k * kPathsWaves + (int)wave] = (uint32_t)__builtin_popcountll(m);
    if (DEPOSIT && st[k] == RT_BOUNCE_MISS) deposit(a, idx[k]);
  }
  __syncthreads();
  // the scattered rays of the segments before this lane's, per round
  uint32_t before[kPathsRounds] = {};
#pragma unroll
  for (int s = 0; s < kPathsSegments; ++s) {
    const uint32_t v = s_seg[s];
#pragma unroll
    for (int k = 0; k < kPathsRounds; ++k) before[k] += (uint32_t)s < (uint32_t)(k * kPathsWaves) + wave ? v : 0u;
  }
  const uint32_t first = as_global(a.tile)[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kPathsRounds; ++k) {
    if (st[k] != RT_BOUNCE_SCATTERED) continue;
    const uint32_t i = idx[k], r = first + before[k] + rank[k];  // r <= i: the scattered rays before ray i
    const size_t o3 = 3 * (size_t)i, r3 = 3 * (size_t)r;
    copy3(a.origin, r3, a.position, o3);
    copy3(a.direction, r3, a.scatter, o3);
    if (a.from) as_global(a.from)[r] = as_global(a.id)[i];
    if (a.okey) {
      const RT_GLOBAL uint32_t *gk = as_global(a.key) + o3;
      RT_GLOBAL uint32_t *ok = as_global(a.okey) + r3;
      ok[0] = gk[0], ok[1] = gk[1], ok[2] = gk[2] + 1u;
    }
    if (a.othroughput) {
      float tr, tg, tb;
      throughput_of(a, o3, tr, tg, tb);
      RT_GLOBAL float *ot = as_global(a.othroughput) + r3;
      ot[0] = tr, ot[1] = tg, ot[2] = tb;
    }
    if (a.oslot) as_global(a.oslot)[r] = as_global(a.slot)[i];
  }
}

struct frame_params {
  const uint32_t *sums;
  float *frame;
  uint32_t n;  // 3 n_slots
  float inv;   // 2^-shift
};

__global__ __launch_bounds__(256) void frame_kernel(const frame_params a) {
  const uint32_t i = (uint32_t)blockIdx.x * 256u + (uint32_t)threadIdx.x;
  if (i < a.n) as_global(a.frame)[i] = (float)as_global(a.sums)[i] * a.inv;
}

}  // namespace rtk

static_assert(RT_BOUNCE_MISS == 0 && RT_BOUNCE_SCATTERED == 1, "the kernels' status values");

namespace {

#ifdef RT_PATHS_DEPOSIT_IN_SCATTER
constexpr bool kDepositInCount = false;
#else
constexpr bool kDepositInCount = true;
#endif

constexpr uint64_t kMaxRays = 0x7fffffffu;             // 2^31 - 1
constexpr uint64_t kMaxSlots = 0xffffffffull / 3;      // 3 n_slots <= 2^32 - 1
constexpr int kIn = 8, kOut = 8, kSums = kIn, kCount = kIn + kOut - 1;
constexpr uint8_t kRayBytes[kIn + kOut] = {1, 4, 12, 12, 12, 12, 12, 4, /* sums */ 0, 12, 12, 4, 12, 12, 4, /* count */ 0};

// A step's arrays, the pointers all host or all device
struct paths_batch {
  uint64_t n, n_slots;
  int32_t shift;
  const void *in[kIn];  // status, id, position, scatter, attenuation, key, throughput, slot
  void *out[kOut];      // sums, origin, direction, from, key, throughput, slot, count
  const void *part(int k) const { return k < kIn ? in[k] : out[k - kIn]; }
  uint64_t bytes(int k) const { return k == kSums ? 12 * n_slots : k == kCount ? 4 : kRayBytes[k] * n; }
};

uint64_t tiles_of(uint64_t n) { return (n + rtk::kPathsTile - 1) / rtk::kPathsTile; }
bool shift_ok(int32_t shift) { return shift >= 0 && shift <= 31; }

// rt_paths_step_check's rules; b is filled when they hold
int step_check(const rt_paths_in *i, const rt_paths_out *o, paths_batch &b) {
  if (!i || !o) return RT_ERR_INVALID;
  if (i->n > kMaxRays || i->n_slots > kMaxSlots || !shift_ok(i->shift) || i->reserved != 0) return RT_ERR_INVALID;
  b = {i->n,
       i->n_slots,
       i->shift,
       {i->status, i->id, i->position, i->scatter, i->attenuation, i->key, i->throughput, i->slot},
       {o->sums, o->origin, o->direction, o->from, o->key, o->throughput, o->slot, o->count}};
  if (!o->count) return RT_ERR_INVALID;
  for (int k = 0; k < kIn; ++k)
    if (i->n > 0 && !b.in[k]) return RT_ERR_INVALID;
  for (int k = kIn; k < kIn + kOut; ++k)
    for (int j = 0; b.part(k) && j < k; ++j)
      if (rtk::overlap(b.part(k), (size_t)b.bytes(k), b.part(j), (size_t)b.bytes(j))) return RT_ERR_INVALID;
  return RT_OK;
}

// the three launches of a step over device pointers (n > 0)
int step_enqueue(const paths_batch &b, void *scratch, hipStream_t st) {
  rtk::paths_params a;
  std::memset(&a, 0, sizeof a);
  a.status = static_cast<const uint8_t *>(b.in[0]);
  a.id = static_cast<const int32_t *>(b.in[1]);
  a.position = static_cast<const float *>(b.in[2]);
  a.scatter = static_cast<const float *>(b.in[3]);
  a.attenuation = static_cast<const float *>(b.in[4]);
  a.key = static_cast<const uint32_t *>(b.in[5]);
  a.throughput = static_cast<const float *>(b.in[6]);
  a.slot = static_cast<const uint32_t *>(b.in[7]);
  a.sums = static_cast<uint32_t *>(b.out[0]);
  a.origin = static_cast<float *>(b.out[1]);
  a.direction = static_cast<float *>(b.out[2]);
  a.from = static_cast<int32_t *>(b.out[3]);
  a.okey = static_cast<uint32_t *>(b.out[4]);
  a.othroughput = static_cast<float *>(b.out[5]);
  a.oslot = static_cast<uint32_t *>(b.out[6]);
  a.count = static_cast<uint32_t *>(b.out[7]);
  a.tile = static_cast<uint32_t *>(scratch);
  a.n = (uint32_t)b.n;
  a.n_slots = (uint32_t)b.n_slots;
  a.n_tiles = (uint32_t)tiles_of(b.n);
  a.scale = (float)(1u << b.shift);
  const bool sums = a.sums != nullptr && a.n_slots > 0;
  if (sums && kDepositInCount)
    rtk::count_kernel<true><<<a.n_tiles, rtk::kPathsBlock, 0, st>>>(a);
  else
    rtk::count_kernel<false><<<a.n_tiles, rtk::kPathsBlock, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  rtk::scan_kernel<<<1, rtk::kPathsScanBlock, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  if (sums && !kDepositInCount)
    rtk::scatter_kernel<true><<<a.n_tiles, rtk::kPathsBlock, 0, st>>>(a);
  else
    rtk::scatter_kernel<false><<<a.n_tiles, rtk::kPathsBlock, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  return RT_OK;
}

int frame_check(const rt_context *c, const uint32_t *sums, uint64_t n_slots, int32_t shift, const float *frame) {
  if (!c || n_slots > kMaxSlots || !shift_ok(shift)) return RT_ERR_INVALID;
  if (n_slots > 0 && (!sums || !frame)) return RT_ERR_INVALID;
  if (rtk::overlap(sums, (size_t)(12 * n_slots), frame, (size_t)(12 * n_slots))) return RT_ERR_INVALID;
  return RT_OK;
}

int frame_enqueue(const uint32_t *sums, uint64_t n_slots, int32_t shift, float *frame, hipStream_t st) {
  rtk::frame_params a;
  a.sums = sums;
  a.frame = frame;
  a.n = (uint32_t)(3 * n_slots);
  a.inv = 1.0f / (float)(1u << shift);
  rtk::frame_kernel<<<(unsigned)(((uint64_t)a.n + 255u) / 256u), 256, 0, st>>>(a);
  RT_HIP(hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_paths_version(void) { return RT_PATHS_VERSION; }
int rt_paths_tile(void) { return rtk::kPathsTile; }
int rt_paths_scan_block(void) { return rtk::kPathsScanBlock; }

int rt_paths_shift(int32_t spp) {
  if (spp < 1 || spp >= 4096) return -1;
  int log2 = 0;
  while ((spp >> (log2 + 1)) != 0) ++log2;
  return 31 - log2;
}

size_t rt_paths_scratch_bytes(uint64_t n) {
  if (n > kMaxRays) return 0;
  return (size_t)((4 * tiles_of(n) + 15) / 16 * 16 + (n == 0 ? 16 : 0));
}

int rt_paths_step_check(const rt_paths_in *in, const rt_paths_out *out) {
  paths_batch b;
  return step_check(in, out, b);
}

int rt_paths_step_async(rt_context *c, const rt_paths_in *dev, const rt_paths_out *out, void *scratch, void *stream) {
  paths_batch b;
  if (!c || step_check(dev, out, b) != RT_OK) return RT_ERR_INVALID;
  if (b.n > 0 && (!scratch || ((uintptr_t)scratch & 15))) return RT_ERR_INVALID;
  rt_pass_scope ps(c, nullptr, nullptr, stream);
  if (ps.status != RT_OK) return ps.end(ps.status);
  if (b.n == 0) {
    const hipError_t e = hipMemsetAsync(b.out[kOut - 1], 0, 4, ps.fs.stream);
    return ps.end(e == hipSuccess ? (int)RT_OK : hip_fail(e));
  }
  return ps.end(step_enqueue(b, scratch, ps.fs.stream));
}

int rt_paths_step(rt_context *c, const rt_paths_in *host, const rt_paths_out *out, double *kernel_ms) {
  paths_batch b;
  if (!c || step_check(host, out, b) != RT_OK) return RT_ERR_INVALID;
  if (kernel_ms) *kernel_ms = 0.0;
  if (b.n == 0) {
    *out->count = 0u;
    return RT_OK;
  }
  // the inputs go up; the sums and the next batch go up and come down (beyond *count the host arrays keep their
  // contents); the count comes down; the scratch stays
  rt_sync_part parts[kIn + kOut + 1];
  for (int k = 0; k < kIn + kOut; ++k) {
    const bool have = b.part(k) != nullptr;
    parts[k] = {have ? (size_t)b.bytes(k) : 0, k == kCount ? nullptr : b.part(k), k < kIn ? nullptr : b.out[k - kIn]};
  }
  parts[kIn + kOut] = {rt_paths_scratch_bytes(b.n), nullptr, nullptr};
  return rt_sync_pass(c, nullptr, nullptr, parts, kernel_ms, [&](void *const *dev, const rt_frame_setup &fs) {
    paths_batch d = b;
    for (int k = 0; k < kIn; ++k) d.in[k] = dev[k];
    for (int k = 0; k < kOut; ++k) d.out[k] = dev[kIn + k];
    return step_enqueue(d, dev[kIn + kOut], fs.stream);
  });
}

int rt_paths_frame_async(rt_context *c, const uint32_t *sums, uint64_t n_slots, int32_t shift, float *frame,
                         void *stream) {
  const int r = frame_check(c, sums, n_slots, shift, frame);
  if (r != RT_OK || n_slots == 0) return r;
  rt_pass_scope ps(c, nullptr, nullptr, stream);
  return ps.end(ps.status == RT_OK ? frame_enqueue(sums, n_slots, shift, frame, ps.fs.stream) : ps.status);
}

int rt_paths_frame(rt_context *c, const uint32_t *sums, uint64_t n_slots, int32_t shift, float *frame,
                   double *kernel_ms) {
  const int r = frame_check(c, sums, n_slots, shift, frame);
  if (r != RT_OK) return r;
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_slots == 0) return RT_OK;
  const size_t bytes = (size_t)(12 * n_slots);
  const rt_sync_part parts[2] = {{bytes, sums, nullptr}, {bytes, nullptr, frame}};
  return rt_sync_pass(c, nullptr, nullptr, parts, kernel_ms, [&](void *const *dev, const rt_frame_setup &fs) {
    return frame_enqueue(static_cast<const uint32_t *>(dev[0]), n_slots, shift, static_cast<float *>(dev[1]), fs.stream);
  });
}

}  // extern "C"
