"""The frames the pilot schedule is checked on (test infrastructure): shared by
test_sched_gpu.py, which compares the device's tile costs and block orders
with sched_ref's on them, and test_sched.py, which shows on the CPU, from the
oracle alone, that each of them can tell a right schedule from a wrong one
(its reference order is not launch order, and its blocks take many distinct
costs).  A case's reference tile costs are computed once per (case, pilot
samples, seed) and shared; nobody writes to them."""
import functools

import oracle_lib
import sched_ref

GRID = 1 << 9    # RT_FLAG_ACCEL_BVH: the layer grid on layer scenes, the BVH elsewhere
PILOT = 1 << 11  # RT_FLAG_PILOT_SCHEDULE
CAM_B = dict(lookfrom=(6, 1, 12))  # the refit tests' second camera (test_configs_gpu.py)

# name: (scene, camera, camera arguments, make_params arguments); every case
# renders with RT_FLAG_PILOT_SCHEDULE on top of its flags
CASES = {
    # the final scene through the layer grid, the reference's lens camera;
    # 67x37: partial tiles on both edges, 45 tiles in 12 blocks (3 padding tiles)
    "final_67x37": ("final", "cpu", {}, dict(width=67, height=37, spp=5, seed=11, flags=GRID)),
    "final_320x120": ("final", "cpu", {}, dict(width=320, height=120, spp=5, seed=12, flags=GRID)),
    # spp = 2: the pilot traces 2 samples, not 4
    "final_67x37_spp2": ("final", "cpu", {}, dict(width=67, height=37, spp=2, seed=13, flags=GRID)),
    "final_320x120_spp2": ("final", "cpu", {}, dict(width=320, height=120, spp=2, seed=14, flags=GRID)),
    # the five-sphere scene (no layer: the plain BVH), src/gpu's pinhole camera and semantics
    "five_64x36": ("five", "gpu", {}, dict(width=64, height=36, spp=4, seed=15, flags=GRID | 3)),
    # rank 1 of 3 in 8-row bands: local rows 0-7, 8-15, 16-23, 24-31 are the
    # frame's 8-15, 32-39, 56-63 and 80-87, the last three of them past row 84
    "band_131x85": ("final", "cpu", {}, dict(width=131, height=85, spp=5, seed=16, flags=GRID, world=3, rank=1,
                                             row_block=8)),
    # the cache: another camera, and another scene, at final_67x37's frame and block count
    "final_67x37_cam_b": ("final", "cpu", CAM_B, dict(width=67, height=37, spp=5, seed=11, flags=GRID)),
    "five_67x37": ("five", "cpu", {}, dict(width=67, height=37, spp=5, seed=11, flags=GRID)),
    # a render split into strided entry ranges (test_host.py test_launch_plan's row)
    "final_320x180": ("final", "cpu", {}, dict(width=320, height=180, spp=50, seed=17, flags=GRID, units=1)),
}
SPLIT_BUDGET = 320 * 180 * 10  # RT_OPT_LAUNCH_SAMPLES for final_320x180: 5 entry ranges


@functools.lru_cache(maxsize=None)
def scene(rtow, which):
    return rtow.final_scene() if which == "final" else rtow.five_scene()


def case(rtow, name, **override):
    """(scene, camera, params) of a case; override: make_params arguments (spp,
    seed, units, ...) that replace the case's.  The flags get PILOT."""
    which, model, cam_kw, kw = CASES[name]
    kw = dict(kw, **override)
    kw["flags"] = kw["flags"] | PILOT
    if model == "cpu":
        cam = rtow.camera_cpu(aspect=kw["width"] / kw["height"], **cam_kw)
    else:
        cam = rtow.camera_gpu(kw["width"], kw["height"], **cam_kw)
    return scene(rtow, which), cam, rtow.make_params(**kw)


@functools.lru_cache(maxsize=None)
def _costs(rtow, name, samples, seed):
    sc, cam, p = case(rtow, name, seed=seed)
    cost = sched_ref.tile_costs(oracle_lib.kernel_pixel_segments(sc, cam, p, samples=samples), p)
    cost.setflags(write=False)
    return cost


def ref_costs(rtow, name, **override):
    """The pilot's tile costs for the case (with the same overrides as case()),
    from the oracle: read-only uint32 [blocks * 4].  Only the seed and min(spp,
    4) of the parameters enter them."""
    _, _, p = case(rtow, name, **override)
    return _costs(rtow, name, min(p.spp, sched_ref.PILOT_SPP), int(p.seed))
