// rt_kernel.hip -- the MI355X (gfx950) render kernel (the device half of the
// C ABI in include/rt.h; the host half is rt_api.cpp, the
// acceleration-structure builder rt_accel.cpp, the layout they share
// rt_layout.h).  Its device helpers -- RNG, camera ray, candidate rule, the
// walks behind closest_hit<>, refine_root -- live in rt_device.h, which the
// first-hit feature pass (rt_aov.hip) compiles too.
//
// Replaces render<<<>>> (src/gpu/camera.h:169-195) and, inside it, get_ray
// (camera.h:153-167 / src/cpu/camera.h:28-34), ray_color (src/cpu/main.cc:12-30,
// iterative as in src/gpu/camera.h:112-138), hittable_list::hit / sphere::hit
// (src/cpu/hittable_list.h:28-43, src/cpu/sphere.h:24-51) and the three
// material::scatter functions (src/cpu/material.h:15-88).
//
// Design:
//  * one wave64 per 8x8 pixel tile, 4 waves per block; the wave owns a pool of
//    its tile's (pixel, sample) items and a lane whose path ends takes the
//    next one ("path regeneration"), so no lane idles while the tile has
//    samples left; the wave exits on __ballot(alive) == 0;
//  * pixel sums are exact fixed-point integers (LDS atomics), so any split of
//    the samples over lanes, waves, launches or GPUs gives the same bits;
//  * closest hit: a per-lane DDA over a layer grid (the default for layer
//    scenes, 3.3), a wave-uniform stackless BVH walk (3.1-3.2) or the
//    brute-force scan; sphere and node records are scalar (SMEM) loads into
//    SGPRs, the grid lives in LDS when it fits;
//  * 8 waves per SIMD: kernel parameters are re-read from the kernarg segment
//    where they are used and per-lane coordinates recomputed, so nothing
//    rarely used stays in registers across the bounce loop;
//  * counter-based RNG (pcg4d keyed by pixel, sample, bounce slot, seed):
//    no per-pixel state, results independent of launch geometry and of the
//    number of GPUs;
//  * fp32 with explicit fmaf and -ffp-contract=off: the kernel is bit-exact
//    with the CPU restatement in oracle/rt_oracle.cc (kernel mode).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "rt_internal.h"
#include "rt_layout.h"
#include "rt_turn_table.h"
#include "rt_device.h"

namespace rtk {


// 8 waves per SIMD (<= 64 VGPRs; the layer-grid build uses 61 VGPRs and 72
// SGPRs, and 6 or 7 waves with more registers ran 2 % slower).  The walk is a serial latency
// chain per wave (scalar node load -> slab test -> ballot -> branch), so more
// resident waves keep the VALU busier: 312 vs 322 ms at 7 waves, although the
// 8-wave budget spills a few values (none inside the walk; the pool's
// per-step ones are pinned to VGPRs, see take below).  That
// became possible once the scene pointers and parameters were re-read from
// the kernarg segment where they are used (kernargs(), as_const()) instead of
// being held in SGPRs for the whole kernel: 94 SGPRs + 21 spilled -> 69 at 7
// waves.
// WIDE (scenes with an albedo above 1, rt_scene_upload): 64-bit pixel sums
//  and the radiance clamps below; the default build's
// code and registers are untouched.
// FOLD (grid builds; 0 elsewhere): the class of the scene's first extras group
// (kFold*, chosen by the host), i.e. which terms of its test scan_extras drops.
template <bool OPEN, bool METAL_UNIT, bool BVH, bool STATS, bool GRID, int GP, bool WIDE, int FOLD>
__global__ __launch_bounds__(kBlock, 8) void render_kernel(const kparams p) {
  typedef typename std::conditional<WIDE, unsigned long long, uint32_t>::type sum_t;
  // Per-lane values that the bounce loop rarely needs are not kept live (VGPR
  // pressure at 8 waves): the wave keeps its tile origin (col0, lrow0, SGPRs),
  // the lane its current pixel slot, sample and global pixel index; column and
  // row are recomputed where they are used.
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
  const unsigned entry = blockIdx.x * (unsigned)p.block_stride + (unsigned)p.block_base;
  const unsigned bid = p.block_order ? as_const(p.block_order)[entry] : entry;
  const int unit = (int)(bid % (unsigned)p.units);
  const int tile = (int)(bid / (unsigned)p.units) * kWavesPerBlock + wave;
  const int col0 = (tile % p.tiles_x) * kTile, lrow0 = (tile / p.tiles_x) * kTile;
  // this wave's samples: an even share of the launch's [s_lo, s_lo + s_cnt)
  const uint32_t s_begin = (uint32_t)p.s_lo + (uint32_t)((uint64_t)unit * (uint32_t)p.s_cnt / (uint32_t)p.units);
  const uint32_t s_end = (uint32_t)p.s_lo + (uint32_t)((uint64_t)(unit + 1) * (uint32_t)p.s_cnt / (uint32_t)p.units);
  // The wave's work pool: item k of [0, kend) is sample
  // s_begin + k / 64 of the tile's pixel slot k % 64 (x = slot % 8, y = slot /
  // 8).  A lane whose path ends takes the next item, so no lane idles while
  // the tile has samples left; a pixel's sum is an exact integer, whichever
  // lanes traced its samples in whatever order.
  const uint32_t kend = (s_end > s_begin ? s_end - s_begin : 0u) << 6;
  __shared__ sum_t s_sum[3][kBlock];                    // the tiles' fixed-point pixel sums
  // per tile row: the global pixel index of (x = 0, y) and how many of the
  // row's 8 slots are in the frame (0 for a row outside it): one ds_read_b64
  // per pool take gives both
  typedef uint32_t u2v __attribute__((ext_vector_type(2)));
  __shared__ u2v s_rowpix[kWavesPerBlock][kTile];
  {
    const int lane = lane_now();
    const int col = col0 + (lane & (kTile - 1));
    const int lrow = lrow0 + (lane >> 3);
    const int band = lrow / p.row_block;
    const int grow = (band * p.band_stride + p.band_offset) * p.row_block + (lrow - band * p.row_block);
    (void)col;
    if ((lane & (kTile - 1)) == 0) {
      const bool row_in = lrow < p.local_rows && grow < p.height;
      const uint32_t ncols = row_in ? (uint32_t)min(kTile, p.width - col0) : 0u;
      s_rowpix[wave][lane >> 3] = u2v{(uint32_t)grow * (uint32_t)p.width + (uint32_t)col0, ncols};
    }
  }
  s_sum[0][threadIdx.x] = s_sum[1][threadIdx.x] = s_sum[2][threadIdx.x] = 0u;
#ifdef RT_LANE_PROFILE
  if ((threadIdx.x & 63) < kLpRegions * 3) (&s_lane_prof[threadIdx.x >> 6][0][0])[threadIdx.x & 63] = 0u;
#endif
  if (GP == kGridLds) {  // the block's copy of the layer grid (kparams grid_n_items)
    const RT_GLOBAL f4 *gi = as_global(p.grid_items);
    for (int i = (int)threadIdx.x; i < p.grid_n_items; i += kBlock) s_grid_dyn[i] = gi[i];
    uint16_t *sc = reinterpret_cast<uint16_t *>(s_grid_dyn + p.grid_n_items);
    const RT_GLOBAL uint32_t *gc = as_global(p.grid_cells);
    // cell i's items are [start_i, start_{i+1}) (the builder numbers every
    // cell's first item by the running count, ring cells included): the LDS
    // holds each start's LDS byte address, plus the end of the last cell
    const uint32_t base = (uint32_t)(uintptr_t)(lds_f4 *)s_grid_dyn;
    for (int i = (int)threadIdx.x; i <= p.grid_n_cells; i += kBlock)
      sc[i] = (uint16_t)(base + ((i < p.grid_n_cells ? gc[i] >> 4 : (uint32_t)p.grid_n_items) << 4));
    __syncthreads();
  } else if (GP == kGridCells) {  // the cell starts only, as item indices (< 2^16)
    uint16_t *sc = reinterpret_cast<uint16_t *>(s_grid_dyn);
    const RT_GLOBAL uint32_t *gc = as_global(p.grid_cells);
    for (int i = (int)threadIdx.x; i <= p.grid_n_cells; i += kBlock)
      sc[i] = (uint16_t)(i < p.grid_n_cells ? gc[i] >> 4 : (uint32_t)p.grid_n_items);
    __syncthreads();
  }
  float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 1.f, dz = 0.f;
  float tmin = 0.001f;  // the ray's t_min (normalize3: 0.001 |d| of its unnormalised direction)
  float thr = 1.f, thg = 1.f, thb = 1.f;
  int depth = 0;
  uint32_t slot = 0, sample = 0, pix = 0;
  int origin_sphere = -1;  // the sphere the ray starts on (-1: a camera ray)
  uint32_t segs = 0, steps = 0;
  work_ctr wc;  // executed work, STATS builds only
  // take pool item k: slot, sample and pixel; false if the slot is outside the
  // frame (the lane then stays alive without tracing and takes another item)
  // wave-uniform values the pool reads once per step, held in VGPRs: as SGPRs
  // they were spilled to VGPR lanes at 8 waves (v_readlane per step)
  uint32_t s_begin_v = s_begin;
  uint32_t rowpix_v = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) u2v *)&s_rowpix[wave][0];
  asm volatile("" : "+v"(s_begin_v), "+v"(rowpix_v));
  auto take = [&](uint32_t k) -> bool {
    slot = k & 63u;
    sample = s_begin_v + (k >> 6);
    const u2v e = ((const __attribute__((address_space(3))) u2v *)(uintptr_t)rowpix_v)[slot >> 3];
    pix = e.x + (slot & (kTile - 1));
    return (slot & (kTile - 1)) < e.y;
  };
  // (col, global row) of the lane's pixel: col from the tile origin, row by
  // exact division (pix - col) / W
  auto pixel_cr = [&](const kparams &k, int &col, int &grow) {
    col = col0 + (int)(slot & (kTile - 1));
    grow = (int)(((pix - (uint32_t)col) >> k.wshift) * k.winv);
  };
  uint32_t knext = 64;  // the pool's next item (wave-uniform); lane l starts with item l
  bool alive = kend != 0 && p.max_depth > 0;  // depth 0: black, no hit test
  bool tracing = false;
  if (alive) {
    tracing = take((uint32_t)lane_now());
    if (tracing) {
      int col, grow;
      pixel_cr(p, col, grow);
      tmin = camera_ray(p, pcg4d(pix, sample, 0u, p.seed32), col, grow, ox, oy, oz, dx, dy, dz);
    }
  }

  // a divergent loop: a lane leaves it when its wave's pool has no item left
  // for it (the step body then runs under the alive lanes' mask, with no
  // wave-level any-alive ballot per step)
  while (alive) {
    LP(kLpStep, tracing);
    hit_state hs = no_hit();
    if (tracing) hs = closest_hit<OPEN, BVH, STATS, GRID, GP, FOLD>(ox, oy, oz, dx, dy, dz, tmin, wc);
    ++steps;
    const int best = best_of<OPEN>(hs);
    // lanes that end their path here (a miss) or hold a slot outside the frame
    // take their next items now: the step's one hash then draws the new camera ray
    const bool miss = !tracing || best < 0;
    uint32_t kn;
    {
      const uint64_t need = __builtin_amdgcn_ballot_w64(miss);
      kn = knext + __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
      knext += (uint32_t)__builtin_popcountll(need);
    }
    bool path_done = false;  // absorbed, or the bounce limit: the lane parks for a step
    bool skipped = false;    // a spurious root: same ray from further along, same t_min
    {
      const kparams q = kernargs();  // shading's parameters, re-read per step
      if (tracing) ++segs;
      if (tracing && best < 0) {
        LP(kLpSky, true);
        // miss: sky gradient, src/cpu/main.cc:27-29; the sample's radiance
        // goes into its pixel's fixed-point sum
        const float a = 0.5f * (dy + 1.0f);
        const float s0 = 1.0f - a;
        const int i = wave * 64 + (int)slot;
        float xr = thr * fmaf(a, 0.5f, s0), xg = thg * fmaf(a, 0.7f, s0), xb = thb * (s0 + a);
        if (WIDE) {  // radiance above the format's bound is clamped (v <= vcap, rt_api.cpp sum_format)
          xr = fminf(xr, q.vcap);
          xg = fminf(xg, q.vcap);
          xb = fminf(xb, q.vcap);
        }
        xr *= q.qscale;
        xg *= q.qscale;
        xb *= q.qscale;
        sum_t nr = (sum_t)xr, ng = (sum_t)xg, nb = (sum_t)xb;
        if (q.dither) {  // spp >= 4096: stochastic rounding
          const float u = dither_u(pix, sample, q.seed32);
          nr += __builtin_amdgcn_fractf(xr) > u ? 1u : 0u;
          ng += __builtin_amdgcn_fractf(xg) > u ? 1u : 0u;
          nb += __builtin_amdgcn_fractf(xb) > u ? 1u : 0u;
        }
        atomicAdd(&s_sum[0][i], nr);
        atomicAdd(&s_sum[1][i], ng);
        atomicAdd(&s_sum[2][i], nb);
      }
      if (miss) {
        if (kn < kend) {
          tracing = take(kn);
        } else {
          alive = tracing = false;
        }
      }
      // One hash per lane and step: a hit draws its bounce, pcg4d(pix, sample,
      // depth + 1); a lane that took a new item draws its camera ray, pcg4d(pix,
      // sample, 0) (only absorbed paths need a second hash below)
      const uint4 r = pcg4d(pix, sample, miss ? 0u : (uint32_t)(depth + 1), q.seed32);
      // one polar draw per lane and step: a hit's unit vector (oracle unit_vec:
      // z = 1 - 2 u1), a new camera ray's lens sample
      const float uz = fmaf(-2.0f, unif(r.x), 1.0f);
      float ux, uy;
      polar(miss ? unif(r.z) : fmaf(-uz, uz, 1.0f), unif(miss ? r.w : r.y), ux, uy);

      if (!miss) {
        LP(kLpHit, true);
        const float o2 = dot3(ox, oy, oz, ox, oy, oz);
        const float ox2 = -2.0f * ox, oy2 = -2.0f * oy, oz2 = -2.0f * oz;
        const float tmax = hs.tmax;
        const bool near = near_of(hs) != 0;
        // a 32-bit byte offset from the records' base (saddr addressing)
        static_assert(sizeof(shade_rec) == 64, "best << 6");
        const shade_rec sr = cload_g((const RT_GLOBAL shade_rec *)((const RT_GLOBAL char *)as_global(q.shade) +
                                                                   ((uint32_t)best << 6)));
        float b;
        const float t = refine_root(sr, tmax, near, ox, oy, oz, dx, dy, dz, o2, ox2, oy2, oz2, b);
        // A refined root before t_min on a sphere the ray moves away from
        // (b > 0): the ray starts on that sphere and leaves its ball, which it
        // cannot meet again; the expanded quadratic's root was an fp32 artefact
        // (DESIGN.md 2, step 3).  So is the exiting root of the very sphere
        // the ray starts on when it moves away from its centre: in exact
        // arithmetic that root is t = 0 (the origin is on the surface), but an
        // fp32 hit point can sit inside the ball by an ulp, which a bounce
        // with a tiny t_min (lambertian n + u with u ~ -n) then "exits" --
        // 6x as many paths entered sealed balls as in the reference's fp64
        // (DESIGN.md 2, step 4).  Not a segment: the ray walks again, same
        // direction -- in the first case from the scan's root point (>= t_min
        // further), in the second from the same origin with t_min raised just
        // past the scan's root, so that root cannot be taken again (moving the
        // origin instead can take ~t_exit / t_min re-walks, unbounded as
        // |n + u| -> 0).
        if (b > 0.0f && (t < tmin || (best == origin_sphere && !near))) {
          if (t < tmin) {
            ox = fmaf(tmax, dx, ox);
            oy = fmaf(tmax, dy, oy);
            oz = fmaf(tmax, dz, oz);
          } else {
            tmin = __uint_as_float(__float_as_uint(tmax) + 1u);  // nextafter(tmax, +inf), tmax > 0 finite
          }
          LP(kLpSkip, true);
          skipped = true;
          --segs;
        } else {
        const float px = fmaf(t, dx, ox), py = fmaf(t, dy, oy), pz = fmaf(t, dz, oz);
        // set_face_normal (hittable.h:16-19): dot(d, outward) < 0 is, in exact
        // arithmetic, "the entering root was taken" (outward flips for r < 0);
        // the root form cannot flip sign at grazing incidence in fp32.  The
        // flip is folded into the 1/r factor: (p - c) (-1/r) = -((p - c) / r)
        // exactly, one select instead of three negations
        const bool front = near != (sr.inv_r < 0.0f);
        const float fir = front ? sr.inv_r : -sr.inv_r;
        const float nx = (px - sr.cx) * fir, ny = (py - sr.cy) * fir, nz = (pz - sr.cz) * fir;
        // shared by the material branches (computed once: lanes of one wave
        // usually hit several materials, so the branches all execute)
        const float dn = dot3(dx, dy, dz, nx, ny, nz);
        float rx, ry, rz;
        reflect3(dx, dy, dz, nx, ny, nz, dn, rx, ry, rz);
        // three independent material blocks, each under its own lane mask (an
        // if / else-if chain compiles to a structurised exec-mask cascade of
        // ~35 scalar instructions; kinds are 0..2, rt_scene_upload checks)
        float sx = rx, sy = ry, sz = rz;
        bool scattered = true;
        const uint32_t kind = sr.kind;
        if (kind == RT_LAMBERTIAN) {
          LP(kLpLamb, true);
          // The opaque-inside rule: a sealed lambertian
          // sphere (no other ball overlaps its ball, rt_accel.cpp
          // sealed_spheres) hit at its exiting root -- the ray started inside
          // its ball, having got in past the surface within t_min of a contact
          // point (a glass sphere resting on the ground) -- ends the path black.
          // In the reference's arithmetic such a path hits the same sphere at
          // t = |r| after every scatter (its chords are n + u long) until the
          // depth cap; here it ends at once, without segments of up to 2000
          // units from origins beyond the grid's padding bound (C4's rank share
          // 408 -> 143 ms at 100 spp, profiles/r03d_c4_ab.log).  Keyed on the
          // root (near), not the face: a negative radius flips the face only.
          scattered = near || !sr.sealed;
          // material.h:19-30
          sx = nx + ux;
          sy = ny + uy;
          sz = nz + uz;
          const float e = 1e-8f;
          if (fabsf(sx) < e && fabsf(sy) < e && fabsf(sz) < e) {
            sx = nx;
            sy = ny;
            sz = nz;
          }
        }
        if (kind == RT_METAL) {
          LP(kLpMetal, true);
          // material.h:40-46
          float fz = sr.param;
          if (!METAL_UNIT) fz *= ball_radius(r);  // random_in_unit_sphere
          sx = fmaf(fz, ux, rx);
          sy = fmaf(fz, uy, ry);
          sz = fmaf(fz, uz, rz);
          scattered = dot3(sx, sy, sz, nx, ny, nz) > 0.0f;
        }
        if (kind >= RT_DIELECTRIC) {
          LP(kLpDiel, true);
          // dielectric, material.h:57-87 (r0 is the same for ior and 1/ior)
          const float ratio = front ? sr.inv_param : sr.param;
          const float cos_t = fminf(-dn, 1.0f);
          // ratio sin > 1 (material.h:64), squared: no square root
          const bool cannot = (ratio * ratio) * fmaf(-cos_t, cos_t, 1.0f) > 1.0f;
          // (s = the reflection, set above, unless it refracts)
          if (!(cannot || schlick(cos_t, sr.r0) > unif(r.x))) refract3(dx, dy, dz, nx, ny, nz, cos_t, ratio, sx, sy, sz);
        }
        // attenuation = albedo (dielectrics store 1,1,1: the product is exact)
        thr *= sr.ar;
        thg *= sr.ag;
        thb *= sr.ab;
        if (WIDE) {  // albedos above 1: the throughput stays finite (inf x 0 would be NaN)
          thr = fminf(thr, 0x1p100f);
          thg = fminf(thg, 0x1p100f);
          thb = fminf(thb, 0x1p100f);
        }
        ++depth;
        if (!scattered || depth >= q.max_depth) {
          path_done = true;  // absorbed, or bounce limit (main.cc:16-17): black
        } else {
          ox = px;
          oy = py;
          oz = pz;
          dx = sx;  // normalised below, with the new camera rays
          dy = sy;
          dz = sz;
          origin_sphere = best;
        }
        }
      } else if (tracing) {
        LP(kLpCamera, true);
        // a new item: its camera ray, with the lens sample drawn above
        int col, grow;
        pixel_cr(q, col, grow);
        camera_dir(q, r, ux, uy, col, grow, ox, oy, oz, dx, dy, dz);
        depth = 0;
        origin_sphere = -1;
        thr = thg = thb = 1.0f;
      }
    }
    // an absorbed path, or one at the bounce limit, parks its lane for a
    // step: the lane takes its next item with the misses of the next step
    // (one camera-ray path per step, with the step's one hash)
    if (path_done) tracing = false;
    LP(kLpTail, true);
    // one normalize3 per lane and step: the bounce direction or the new
    // camera ray's (a finished lane's is unused), and with it the ray's t_min
    // (a skipped ray keeps its own)
    const float tmin_new = normalize3(dx, dy, dz);
    tmin = skipped ? tmin : tmin_new;
  }

  const int lane = lane_now();
  {
    const kparams q = kernargs();
    const int col = col0 + (lane & (kTile - 1)), lrow = lrow0 + (lane >> 3);
    if (col < q.width && lrow < q.local_rows) {  // padding pixels (row >= height) write zeros
      const size_t o = 3 * ((size_t)lrow * q.width + col);
      const int i = wave * 64 + lane;
      if (!q.sum_atomic) {
        RT_GLOBAL float *out = as_global(q.out) + o;
        out[0] = (float)s_sum[0][i] * q.qinv;
        out[1] = (float)s_sum[1][i] * q.qinv;
        out[2] = (float)s_sum[2][i] * q.qinv;
      } else {  // the tile's units / launches add their integer sums (finish_sums converts)
        // (global, not generic, atomics: the product's device code holds no
        // flat memory instruction, DESIGN.md 8 "the v7 fault")
        RT_GLOBAL sum_t *acc = reinterpret_cast<RT_GLOBAL sum_t *>(as_global(q.out)) + o;  // WIDE: the 64-bit scratch frame
        __hip_atomic_fetch_add(acc + 0, s_sum[0][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(acc + 1, s_sum[1][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(acc + 2, s_sum[2][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
#ifdef RT_LANE_PROFILE
  if (lane < kLpRegions * 3)
    atomicAdd(&g_lane_prof[lane], (unsigned long long)(&s_lane_prof[wave][0][0])[lane]);
#endif
  // one atomic per wave for the counters
  uint32_t s = segs;
  // wave-steps: the most any lane of the wave looped
  uint32_t ws = steps;
  uint64_t lt = wc.tests, lb = wc.boxes, lh = wc.box_hits, lr = wc.roots;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off);
    ws = max(ws, (uint32_t)__shfl_xor(ws, off));
    if (STATS) {
      lt += __shfl_xor(lt, off);
      lb += __shfl_xor(lb, off);
      lh += __shfl_xor(lh, off);
      lr += __shfl_xor(lr, off);
    }
  }
  if (lane == 0) {
    if (STATS) {  // pilot renders (units = 1, launch order): segments per tile
      const kparams k = kernargs();
      if (k.tile_cost) {
        // and nothing else: 6 same-address atomics from each of ~10^5 short
        // waves serialise (the 4-spp pilot took 9.5 ms instead of ~1.2)
        as_global(k.tile_cost)[(int)blockIdx.x * kWavesPerBlock + wave] = s;
        return;
      }
    }
    RT_GLOBAL unsigned long long *counters = as_global(kernargs().counters) + 8 * (blockIdx.x & (kCounterSlots - 1));
    auto add = [](RT_GLOBAL unsigned long long *a, unsigned long long v) {
      __hip_atomic_fetch_add(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    add(&counters[0], s);
    add(&counters[1], ws);
    if (STATS) {
      add(&counters[2], lt);
      add(&counters[3], lb);
      add(&counters[4], lh);
      add(&counters[5], lr);
    }
  }
}

// Several waves per tile (rt_params.units > 1): they added their integer pixel
// sums into the frame (zeroed first), which holds uint32 sums until this pass
// converts them in place, sum * 2^-F.  Memory-bound and tiny.
__global__ __launch_bounds__(256) void finish_sums(uint32_t *__restrict__ frame, uint64_t n, float qinv) {
  // every access goes through the uint32 view: the float result is stored as its bits
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u)
    frame[j] = __float_as_uint((float)frame[j] * qinv);
}

// The same for WIDE renders: the 64-bit sums live in the context's scratch
// frame (the caller's fp32 frame has 4 bytes per channel), converted into it.
__global__ __launch_bounds__(256) void finish_sums_wide(const uint64_t *__restrict__ sums, float *__restrict__ frame,
                                                        uint64_t n, float qinv) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256u)
    frame[j] = (float)sums[j] * qinv;
}

// Known-answer evaluation of the render kernel's own device arithmetic
// (rt_device_kat; tests/test_parity_gpu.py checks it against the reference's
// vectors in tests/golden/kat.jsonl).  Case layout: 10 doubles in, 9 out.
//   RT_KAT_SPHERE_HIT  in  o[3] d[3] c[3] r      (sphere::hit, src/cpu/sphere.h:24-51,
//                                                  t_min 0.001 in units of d, t_max inf)
//                      out hit, t (in units of the given d), p[3], normal[3], front_face
//                      -- the scan's candidate test, refine_root, the shading normal
//                      and set_face_normal, exactly as render_kernel runs them on a
//                      direction normalised by normalize3
//   RT_KAT_REFLECT     in  v[3] n[3]             out reflect3(v, n)
//   RT_KAT_REFRACT     in  v[3] n[3] eta         out refract3(v, n, eta)
//   RT_KAT_REFLECTANCE in  cosine ref_idx        out schlick(cosine, r0(ref_idx))
__global__ __launch_bounds__(64) void kat_kernel(int kind, const double *__restrict__ in, int n,
                                                 double *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double *a = in + 10 * (size_t)i;
  double *o = out + 9 * (size_t)i;
  for (int k = 0; k < 9; ++k) o[k] = 0.0;
  if (kind == RT_KAT_SPHERE_HIT) {
    const float ox = (float)a[0], oy = (float)a[1], oz = (float)a[2];
    float dx = (float)a[3], dy = (float)a[4], dz = (float)a[5];
    const double len = sqrt(a[3] * a[3] + a[4] * a[4] + a[5] * a[5]);
    const float tmin = normalize3(dx, dy, dz);
    shade_rec sr;
    sr.cx = (float)a[6];
    sr.cy = (float)a[7];
    sr.cz = (float)a[8];
    sr.radius = (float)a[9];
    sr.inv_r = 1.0f / sr.radius;
    const double cx = sr.cx, cy = sr.cy, cz = sr.cz, rr = sr.radius;
    sr.ks = (float)(cx * cx + cy * cy + cz * cz - rr * rr);  // as rt_scene_upload
    const float nk1 = -dot3(ox, oy, oz, dx, dy, dz);
    const float o2 = dot3(ox, oy, oz, ox, oy, oz);
    const float ox2 = -2.0f * ox, oy2 = -2.0f * oy, oz2 = -2.0f * oz;
    const float h = fmaf(sr.cz, dz, fmaf(sr.cx, dx, fmaf(sr.cy, dy, nk1)));
    const float g = fmaf(sr.cz, oz2, fmaf(sr.cx, ox2, fmaf(sr.cy, oy2, o2)));
    const float e = fmaf(h, h, -g);
    hit_state hs = no_hit();
    candidate<false>(e >= sr.ks, h, e - sr.ks, tie2_of<false>(0u), tmin, hs);
    if (best_of<false>(hs) < 0) return;
    float b_unused;
    const float t = refine_root(sr, hs.tmax, near_of(hs) != 0, ox, oy, oz, dx, dy, dz, o2, ox2, oy2, oz2, b_unused);
    const float px = fmaf(t, dx, ox), py = fmaf(t, dy, oy), pz = fmaf(t, dz, oz);
    float nx = (px - sr.cx) * sr.inv_r, ny = (py - sr.cy) * sr.inv_r, nz = (pz - sr.cz) * sr.inv_r;
    const bool front = (near_of(hs) != 0) != (sr.inv_r < 0.0f);
    if (!front) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
    o[0] = 1.0;
    o[1] = (double)t / len;
    o[2] = px;
    o[3] = py;
    o[4] = pz;
    o[5] = nx;
    o[6] = ny;
    o[7] = nz;
    o[8] = front ? 1.0 : 0.0;
  } else if (kind == RT_KAT_REFLECT || kind == RT_KAT_REFRACT) {
    const float vx = (float)a[0], vy = (float)a[1], vz = (float)a[2];
    const float nx = (float)a[3], ny = (float)a[4], nz = (float)a[5];
    float x, y, z;
    if (kind == RT_KAT_REFLECT) {
      reflect3(vx, vy, vz, nx, ny, nz, dot3(vx, vy, vz, nx, ny, nz), x, y, z);
    } else {
      const float cos_t = fminf(-dot3(vx, vy, vz, nx, ny, nz), 1.0f);
      refract3(vx, vy, vz, nx, ny, nz, cos_t, (float)a[6], x, y, z);
    }
    o[0] = x;
    o[1] = y;
    o[2] = z;
  } else if (kind == RT_KAT_REFLECTANCE) {
    const double r0 = (1.0 - a[1]) / (1.0 + a[1]);  // as rt_scene_upload's shade_rec.r0
    o[0] = schlick((float)a[0], (float)(r0 * r0));
  }
}

// write_color on the device (rt_tonemap_async): the level of a channel is
// (int)(256 * clamp(sqrt(sum * scale), 0, 0.999)) in fp64 with scale = 1.0 / spp
// (src/cpu/color.h:8-23), or in fp32 with scale = 1.0f / spp
// (src/gpu/color.h:16-38).  sqrt is monotone, so the level is the number of
// thresholds T[k] = min{q : sqrt_rn(q) >= k / 256}, k = 1..255, that q = sum *
// scale reaches (tonemap_thresholds, on the host with its correctly rounded
// sqrt).  The device estimates the level with its own sqrt and corrects it by
// one step against T: the result does not depend on how the device rounds
// sqrt.  NaN sums map to 0 (rt_tonemap_u8 does the same).  Four channels per
// lane: one 16-B load, one 4-B store (HBM-bound, 15 B per pixel).
template <bool FP32, typename T>
__device__ __forceinline__ uint32_t tone_level(float s, T scale, const T *__restrict__ thr) {
  const T q = (T)s * scale;
  const T y = (T)256 * (FP32 ? (T)sqrtf((float)q) : (T)sqrt((double)q));
  int l = y >= (T)255 ? 255 : (y > (T)0 ? (int)y : 0);
  if (l < 255 && q >= thr[l + 1]) ++l;
  else if (l > 0 && q < thr[l]) --l;
  return (uint32_t)l;
}

template <bool FP32, typename T>
__global__ __launch_bounds__(256) void tonemap_kernel(const float *__restrict__ sums, uint64_t n, T scale,
                                                      const T *__restrict__ thr_g, uint8_t *__restrict__ out) {
  __shared__ T thr[256];
  thr[threadIdx.x] = thr_g[threadIdx.x];
  __syncthreads();
  const uint64_t n4 = n / 4;
  const bool vec = ((uintptr_t)sums % 16 == 0) && ((uintptr_t)out % 4 == 0);
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  if (vec) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n4; i += stride) {
      const f4 v = reinterpret_cast<const f4 *>(sums)[i];
      reinterpret_cast<uint32_t *>(out)[i] =
          tone_level<FP32, T>(v.x, scale, thr) | tone_level<FP32, T>(v.y, scale, thr) << 8 |
          tone_level<FP32, T>(v.z, scale, thr) << 16 | tone_level<FP32, T>(v.w, scale, thr) << 24;
    }
  }
  for (uint64_t i = (vec ? 4 * n4 : 0) + (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride)
    out[i] = (uint8_t)tone_level<FP32, T>(sums[i], scale, thr);
}

// ------------------------------------------------------------ launches ----
// render_kernel variant V (rt_layout.h kVar*): the grid bits count only with
// the BVH flag on a layer scene (without it they select the scan), and the
// placement only with the grid walk.
template <int V>
void launch_variant(unsigned blocks, size_t lds, hipStream_t st, const kparams &kp) {
  constexpr bool O = V & kVarOpen, U = V & kVarMetalUnit, B = V & kVarBvh, S = V & kVarStats;
  constexpr bool G = B && (V & kVarGrid), W = V & kVarWide;
  constexpr int P = G ? ((V >> kVarPlaceShift) & 3) % 3 : kGridGlobal;
  // the first extras group's class: a build of its own for the grid walk
  // only (the scan and BVH builds are one kernel each whatever the bits say)
  constexpr int F = G ? (V >> kVarFoldShift) & 3 : 0;
  render_kernel<O, U, B, S, G, P, W, F><<<blocks, kBlock, G ? lds : 0, st>>>(kp);
}
using launch_fn = void (*)(unsigned, size_t, hipStream_t, const kparams &);
template <int... V>
constexpr auto launch_table(std::integer_sequence<int, V...>) {
  return std::array<launch_fn, sizeof...(V)>{&launch_variant<V>...};
}
constexpr auto kLaunch = launch_table(std::make_integer_sequence<int, kVarCount>{});

hipError_t launch_render(int variant, unsigned blocks, size_t lds_bytes, hipStream_t st, const kparams &kp) {
  if (variant < 0 || variant >= (int)kLaunch.size()) return hipErrorInvalidValue;
  kLaunch[variant](blocks, lds_bytes, st, kp);
  return hipGetLastError();
}

hipError_t launch_finish_sums(uint32_t *frame, uint64_t n, float qinv, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 256u * 64u);
  finish_sums<<<grid, 256, 0, st>>>(frame, n, qinv);
  return hipGetLastError();
}

hipError_t launch_finish_sums_wide(const uint64_t *sums, float *frame, uint64_t n, float qinv, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 256u * 64u);
  finish_sums_wide<<<grid, 256, 0, st>>>(sums, frame, n, qinv);
  return hipGetLastError();
}

hipError_t launch_tonemap(bool fp32, const float *sums, uint64_t n, int spp, const void *thresholds,
                          uint8_t *out, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<uint64_t>((n / 4 + 255) / 256 + 1, 256u * 32u);
  if (!fp32)
    tonemap_kernel<false, double><<<grid, 256, 0, st>>>(sums, n, 1.0 / spp, (const double *)thresholds, out);
  else
    tonemap_kernel<true, float><<<grid, 256, 0, st>>>(sums, n, 1.0f / (float)spp, (const float *)thresholds, out);
  return hipGetLastError();
}

hipError_t launch_kat(int kind, const double *in, int n, double *out) {
  kat_kernel<<<(unsigned)((n + 63) / 64), 64>>>(kind, in, n, out);
  return hipGetLastError();
}

hipError_t upload_turn_table() {
  float tab[2 * RT_TURN_TABLE];
  rt_turn_table(tab);
  return hipMemcpyToSymbol(HIP_SYMBOL(g_turn_tab), tab, sizeof tab);
}

}  // namespace rtk

#ifdef RT_LANE_PROFILE
// the measurement variant's counters (tools/lane_profile.py): read (and, with
// reset != 0, zero) the kLpRegions x (waves, exec lanes, useful lanes) sums
extern "C" int rt_lane_profile_read(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rtk::g_lane_prof), sizeof(rtk::g_lane_prof)) != hipSuccess) return -2;
  if (reset) {
    static const unsigned long long zero[rtk::kLpRegions * 3] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_lane_prof), zero, sizeof(zero)) != hipSuccess) return -2;
  }
  return rtk::kLpRegions;
}
#endif
