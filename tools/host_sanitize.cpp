// tools/host_sanitize.cpp -- drives the library's host code under ASan + UBSan
// on the CPU (no device): the scene builders, both cameras, the BVH / layer-grid
// builder (rt_internal_accel_info) and its grid fitter (csrc/rt_accel.h, linked
// directly), both tonemaps and the P3 / P6 writers, on the reference scenes
// and on ragged / degenerate inputs, and the argument rules the image-space
// passes share (csrc/rt_post.h, csrc/rt_reproject.h: inline, no device), and the
// traced passes' sample cut (csrc/rt_frame.h).  Built and run by
// tools/host_sanitize.sh; exits non-zero on any failed check (the sanitizers
// abort on their own findings).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <fcntl.h>
#include <unistd.h>
#include <vector>

#include "rt_internal.h"
#include "rt_accel.h"
#include "rt_frame.h"
#include "rt_reproject.h"

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      std::fprintf(stderr, "check failed: %s (line %d)\n", #x, __LINE__); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

struct scene {
  std::vector<float> cx, cy, cz, r, alb, par;
  std::vector<uint32_t> kind;
  rt_scene_buf buf(uint32_t cap) {
    cx.resize(cap), cy.resize(cap), cz.resize(cap), r.resize(cap), par.resize(cap);
    alb.resize(3 * (size_t)cap), kind.resize(cap);
    return rt_scene_buf{cap, 0, cx.data(), cy.data(), cz.data(), r.data(), kind.data(), alb.data(), par.data()};
  }
  rt_scene_view view(uint32_t n) const {
    return rt_scene_view{n, cx.data(), cy.data(), cz.data(), r.data(), kind.data(), alb.data(), par.data()};
  }
};

static void accel(const rt_scene_view &v, bool expect_layer) {
  // every grid placement (auto, LDS, cells in LDS, global) and a few cell scales
  for (int place = 0; place <= 3; ++place)
    for (double scale : {0.0, 0.5, 1.3}) {
      uint64_t info[RT_ACCEL_INFO_N];
      CHECK(rt_internal_accel_info(&v, place, scale, info, RT_ACCEL_INFO_N) == RT_OK);
      CHECK((info[2] != 0) == expect_layer);
      if (info[7]) CHECK(info[11] == 1 && info[12] == 1 && info[10] <= 15 && info[16] >= 1);
      // values 36..42: the grid's geometry as float32 bits, zeros without a grid
      for (int k = 36; k < RT_ACCEL_INFO_N; ++k) CHECK(info[k] <= 0xffffffffull && (info[7] || info[k] == 0));
      CHECK((info[38] != 0) == (info[5] != 0));  // a cell side iff stored cells
    }
  uint64_t two[2];
  CHECK(rt_internal_accel_info(&v, 0, 0.0, two, 2) == RT_OK);  // a short buffer is filled, no more
  CHECK(rt_internal_accel_info(&v, 4, 0.0, two, 2) != RT_OK);
}

// what rt_internal_accel_info checks of a built grid: nx x nz stored cells,
// whole items, running item starts, an empty ring
static void grid_ok(const rtk::grid_geom &g) {
  CHECK(g.nx >= 3 && g.nz >= 3 && g.cells.size() == (size_t)g.nx * (size_t)g.nz);
  CHECK(g.items.size() % 4 == 0);
  const size_t items = g.items.size() / 4;
  for (size_t i = 0; i < g.cells.size(); ++i) {
    const uint32_t first = g.cells[i] >> 4, cnt = g.cells[i] & 15u;
    CHECK(first + cnt == (i + 1 < g.cells.size() ? g.cells[i + 1] >> 4 : items));
    const int x = (int)(i % g.nx), z = (int)(i / g.nx);
    if (x == 0 || z == 0 || x == g.nx - 1 || z == g.nz - 1) CHECK(cnt == 0);
  }
}

// The grid fitter behind RT_OPT_GRID_FIT, for every requested placement that
// can have one: each candidate scale that choose() reports for a camera builds
// a sound grid, and build() at the builder's own scale reproduces the grid
// build_accel returned (one rtk::grid_geom from the builder to the refit).
static void fitter(const rt_scene_view &v, const rt_camera (&cams)[2]) {
  for (int place : {-1, (int)rtk::kGridLds, (int)rtk::kGridCells}) {
    rtk::accel_options o;
    o.grid_placement = place;
    rtk::accel_build a;
    rtk::grid_fitter *f = nullptr;
    rtk::build_accel(&v, o, a, &f);
    CHECK(!a.grid.cells.empty());
    grid_ok(a.grid);
    CHECK((f != nullptr) == (a.grid_placement != rtk::kGridGlobal));
    if (!f) continue;  // (10 000 spheres do not fit kGridLds: global memory, no fitter)
    rtk::grid_geom g;
    CHECK(f->build(a.grid.scale, g));
    CHECK(g == a.grid);
    for (const rt_camera &cam : cams) {
      std::vector<std::pair<double, double>> cs;
      const double best = f->choose(cam, 640, 360, &cs);
      CHECK(!cs.empty() && cs.size() <= (size_t)rtk::kFitSteps + 1);
      bool seen = false;
      for (const std::pair<double, double> &c : cs) {
        CHECK(f->build(c.first, g));
        CHECK(g.scale == c.first);
        grid_ok(g);
        seen = seen || c.first == best;
      }
      CHECK(seen);
    }
    delete f;
  }
}

int main() {
  // the final scene at several sizes (half extent 11: 486 spheres; 50: 10k)
  for (int he : {0, 1, 3, 11, 50}) {
    scene s;
    const uint32_t cap = (uint32_t)(4 * he * he + 8);
    rt_scene_buf b = s.buf(cap);
    double next = 0;
    CHECK(rt_scene_final(he, &b, &next) == RT_OK);
    CHECK(b.n <= cap);
    accel(s.view(b.n), he >= 11);
    // the grid fitter (RT_OPT_GRID_FIT's host model) for two frame geometries
    if (he == 11 || he == 50) {
      rt_camera cam;
      const double from[3] = {13, 2, 3}, at[3] = {0, 0, 0}, up[3] = {0, 1, 0};
      CHECK(rt_camera_cpu(from, at, up, 20.0, 16.0 / 9.0, 0.1, 10.0, &cam) == RT_OK);
      const rt_scene_view v = s.view(b.n);
      double scale = -1, costs[2 * 40];
      size_t n = 0;
      CHECK(rt_internal_grid_fit(&v, &cam, 3840, 2160, &scale, costs, 40, &n) == RT_OK);
      CHECK(scale > 0 && n >= 1 && n <= 31);
      CHECK(rt_internal_grid_fit(&v, &cam, 64, 64, &scale, nullptr, 0, &n) == RT_OK);
      rt_camera cams[2] = {cam, cam};
      const double from2[3] = {-3, 6, 12};
      CHECK(rt_camera_cpu(from2, at, up, 40.0, 1.0, 0.0, 10.0, &cams[1]) == RT_OK);
      fitter(v, cams);
    }
  }
  {  // too small a buffer is refused
    scene s;
    rt_scene_buf b = s.buf(3);
    CHECK(rt_scene_final(11, &b, nullptr) != RT_OK);
  }
  {  // the five-sphere scene (no layer), and an empty scene
    scene s;
    rt_scene_buf b = s.buf(8);
    CHECK(rt_scene_five(&b) == RT_OK);
    accel(s.view(b.n), false);
    accel(s.view(0), false);
  }
  {  // a dense layer: 300 overlapping spheres in 1.5 x 1.5 (the builder shrinks cells or gives up)
    scene s;
    s.buf(300);
    for (int i = 0; i < 300; ++i) {
      s.cx[i] = 1.5f * (float)((i * 37) % 100) / 100.0f;
      s.cz[i] = 1.5f * (float)((i * 61) % 100) / 100.0f;
      s.cy[i] = 0.2f;
      s.r[i] = 0.2f;
      s.kind[i] = RT_LAMBERTIAN;
      s.alb[3 * i] = s.alb[3 * i + 1] = s.alb[3 * i + 2] = 0.5f;
    }
    uint64_t info[RT_ACCEL_INFO_N];
    const rt_scene_view v = s.view(300);
    CHECK(rt_internal_accel_info(&v, 0, 0.0, info, RT_ACCEL_INFO_N) == RT_OK);
    if (info[7]) CHECK(info[11] == 1 && info[12] == 1 && info[10] <= 15);
  }
  // cameras (both models, with and without a lens)
  rt_camera cam;
  const double from[3] = {13, 2, 3}, at[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  CHECK(rt_camera_cpu(from, at, up, 20.0, 16.0 / 9.0, 0.1, 10.0, &cam) == RT_OK);
  CHECK(rt_camera_gpu(from, at, up, 20.0, 1920, 1080, 0.6, 10.0, &cam) == RT_OK);
  // tonemaps (both modes) and the writers, on ragged sizes
  for (int w : {1, 7, 333}) {
    const int h = 5;
    std::vector<float> sums(3 * (size_t)w * h);
    for (size_t i = 0; i < sums.size(); ++i) sums[i] = (float)(i % 97) * 0.37f;
    std::vector<uint8_t> rgb(sums.size());
    for (int spp : {1, 10, 500}) {
      CHECK(rt_tonemap_u8_mode(sums.data(), (size_t)w * h, spp, RT_TONEMAP_CPU, rgb.data()) == RT_OK);
      CHECK(rt_tonemap_u8_mode(sums.data(), (size_t)w * h, spp, RT_TONEMAP_GPU, rgb.data()) == RT_OK);
    }
    const int fd = open("/dev/null", O_WRONLY);
    CHECK(fd >= 0);
    CHECK(rt_write_ppm(fd, rgb.data(), w, h, 0) == RT_OK);
    CHECK(rt_write_ppm(fd, rgb.data(), w, h, 1) == RT_OK);
    close(fd);
  }
  // launch plans (rt_internal_launch_plan): frames from one pixel to C4's,
  // spp up to the ABI's maximum, budgets from 1 sample to 2^40
  for (int w : {1, 9, 3840, 16384}) {
    for (int spp : {0, 1, 16, 2000, (1 << 24) - 1}) {
      for (double budget : {0.0, 1.0, 1e6, 4294967296.0, 1099511627776.0}) {
        rt_params p;
        std::memset(&p, 0, sizeof p);
        p.width = w;
        p.height = w;
        p.spp = spp;
        p.max_depth = 50;
        p.row_block = w;
        p.band_stride = 1;
        p.local_rows = w;
        p.flags = RT_FLAG_ACCEL_BVH | RT_FLAG_PILOT_SCHEDULE;
        uint64_t plan[RT_LAUNCH_PLAN_N];
        CHECK(rt_internal_launch_plan(&p, budget, plan, RT_LAUNCH_PLAN_N) == RT_OK);
        CHECK(plan[0] >= 1 && plan[1] >= 1 && plan[2] >= 1 && plan[4] == plan[0] * plan[1] && plan[4] <= 65536);
        CHECK(plan[0] <= plan[3] && (spp == 0 || plan[1] <= (uint64_t)spp));
      }
    }
  }
  // the passes' shared argument rules (csrc/rt_post.h, csrc/rt_reproject.h)
  {
    char buf[64];
    CHECK(rtk::overlap(buf, 16, buf + 15, 16) && rtk::overlap(buf + 15, 16, buf, 16) && rtk::overlap(buf, 64, buf, 1));
    CHECK(!rtk::overlap(buf, 16, buf + 16, 16) && !rtk::overlap(buf + 16, 16, buf, 16));
    CHECK(!rtk::overlap(nullptr, 16, buf, 16) && !rtk::overlap(buf, 16, nullptr, 16));
    CHECK(rtk::post_aligned16(nullptr) && rtk::post_aligned16((void *)(uintptr_t)32) &&
          !rtk::post_aligned16((void *)(uintptr_t)40));
    int n = -1;
    CHECK(rtk::post_option(0, 2, 1, true, 1024, n) && n == 2);
    CHECK(rtk::post_option(1024, 2, 1, true, 1024, n) && n == 1024);
    CHECK(!rtk::post_option(1025, 2, 1, true, 1024, n) && !rtk::post_option(-1, 2, 1, true, 1024, n));
    float v = -1.0f;
    CHECK(rtk::post_option(0.0f, 0.5f, 0.0f, false, INFINITY, v) && v == 0.5f);
    CHECK(rtk::post_option(-0.0f, 0.5f, 0.0f, false, INFINITY, v) && v == 0.5f);
    CHECK(rtk::post_option(INFINITY, 0.5f, 0.0f, false, INFINITY, v) && std::isinf(v));
    CHECK(!rtk::post_option(-1e-30f, 0.5f, 0.0f, false, INFINITY, v) && !rtk::post_option(NAN, 0.5f, 0.0f, false, INFINITY, v));
    CHECK(rtk::post_option(-1.0f, 0.9f, -1.0f, true, 1.0f, v) && v == -1.0f);
    CHECK(!rtk::post_option(1.5f, 0.9f, -1.0f, true, 1.0f, v) && !rtk::post_option(NAN, 0.9f, -1.0f, true, 1.0f, v));
    CHECK(rtk::rp_camera_ok(&cam, 1, 1) && !rtk::rp_camera_ok(nullptr, 4, 4) && !rtk::rp_camera_ok(&cam, 0, 4) &&
          !rtk::rp_camera_ok(&cam, 4, 32769));
    rt_camera cpu_cam;
    CHECK(rt_camera_cpu(from, at, up, 20.0, 16.0 / 9.0, 0.1, 10.0, &cpu_cam) == RT_OK);
    CHECK(rtk::rp_camera_ok(&cpu_cam, 2, 2) && !rtk::rp_camera_ok(&cpu_cam, 1, 2) && !rtk::rp_camera_ok(&cpu_cam, 2, 1));
    cpu_cam.model = 77;
    CHECK(!rtk::rp_camera_ok(&cpu_cam, 4, 4));
  }
  // the traced feature passes' cut of a frame's samples into launches (csrc/rt_frame.h)
  {
    struct range {
      int lo, cnt;
    };
    const auto ranges = [](int spp, double frame_px, double launch_samples) {
      std::vector<range> r;
      const long long per = rt_samples_per_launch(spp, frame_px, launch_samples);
      CHECK(per >= 1);
      CHECK(rt_sample_ranges(spp, per, [&](int lo, int cnt) {
              r.push_back({lo, cnt});
              return (int)RT_OK;
            }) == RT_OK);
      return r;
    };
    std::vector<range> r = ranges(0, 64.0 * 64.0, 1e6);  // spp = 0: one launch that only initialises
    CHECK(r.size() == 1 && r[0].lo == 0 && r[0].cnt == 0);
    r = ranges(1, 64.0 * 64.0, 1e6);
    CHECK(r.size() == 1 && r[0].lo == 0 && r[0].cnt == 1);
    CHECK(rt_samples_per_launch(16, 3840.0 * 2160.0, 1e6) == 1);  // a frame larger than launch_samples
    CHECK(ranges(16, 3840.0 * 2160.0, 1e6).size() == 16);
    CHECK(rt_samples_per_launch(16, 64.0 * 64.0, 1e6) == 16 && rt_samples_per_launch(500, 64.0 * 64.0, 1e6) == 244);
    for (int spp : {1, 7, 500, 65536, 65537, 200000, (1 << 24) - 1})
      for (double frame_px : {1.0, 64.0 * 64.0, 16384.0 * 16384.0})
        for (double budget : {1.0, 1e6, 1099511627776.0}) {
          r = ranges(spp, frame_px, budget);
          CHECK(!r.empty() && r.size() <= (size_t)rtk::kMaxLaunches);
          long long next = 0;
          for (const range &x : r) {  // ascending, contiguous, none empty
            CHECK(x.lo == next && x.cnt >= 1);
            next += x.cnt;
          }
          CHECK(next == spp);
        }
    // a failing launch ends the ranges with its status
    int calls = 0;
    CHECK(rt_sample_ranges(8, 2, [&](int, int) { return ++calls == 2 ? (int)RT_ERR_HIP : (int)RT_OK; }) == RT_ERR_HIP &&
          calls == 2);
  }
  std::printf("host_sanitize: ok\n");
  return 0;
}
