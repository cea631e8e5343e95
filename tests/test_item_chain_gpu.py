"""The layer-grid walk's item chain (csrc/rt_device.h grid_walk):
with the grid in LDS a cell's first K = 4 items (RT_ITEM_CHAIN) are tested in
straight-line stages on every walking lane, masked by the lane's item count,
and the rest by the pointer loop.  Every case is a small frame compared with
tobytes() against the oracle's kernel mode (a brute-force scan that knows no
grid), so a stage that let a lane past its cell's end win, or dropped an
item, shows as a differing float or segment count.
"""
import dataclasses

import numpy as np
import pytest

from oracle_lib import kernel_render
from ray_fans import crowd

pytestmark = pytest.mark.gpu

K = 4  # RT_ITEM_CHAIN of the product build (csrc/rt_layout.h)
MODES = ("lds", "cells", "global")
INTERVALS = {"closed": 0, "open": 1}  # RT_FLAG_OPEN_INTERVAL


# 80 spheres thrown into a square of half side `half`, and the cell scale at
# which the host's grid has exactly `most` items in its fullest cell.  The
# construction's own 1.5 x 1.5 square of r = 0.2 spheres builds no grid at any
# scale (a padded box is at least 0.18 wide: more than 15 meet in some cell),
# so the radius is 0.1 there and the sparser fixtures spread the spheres out.
DENSE = {K - 1: (8.0, 0.05, 0.5), K: (3.0, 0.05, 0.5), K + 1: (3.0, 0.05, 1.0), 15: (0.75, 0.1, 2.8)}


def dense(rtow, most):
    half, radius, scale = DENSE[most]
    rng = np.random.default_rng(80)
    cx, cz = rng.uniform(-half, half, 80), rng.uniform(-half, half, 80)
    cam = rtow.camera_cpu(lookfrom=(4.0 * half, 2.0 * half, 2.7 * half), lookat=(0.0, 0.1, 0.0), aspect=64 / 64)
    return crowd(rtow, cx, cz, radius, 81), scale, cam


def render_pair(rtow, ctx, scene, cam, p, mode, scale=None):
    """(sums, stats) of one placement; the context's grid options go back to their defaults."""
    ctx.upload(scene, grid_mode=mode, grid_scale=0.0 if scale is None else scale)
    try:
        got, st = ctx.render(cam, p)
    finally:
        ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, rtow.RT_GRID_AUTO)
        ctx.set_option(rtow.RT_OPT_GRID_SCALE, 0.0)
    return got, st


def same_bits(got, st, want, segs, what):
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))
    assert st.segments == segs, what


@pytest.mark.parametrize("interval", list(INTERVALS))
def test_final_scene_every_placement(rtow, gpu_ctx, interval):
    """The final scene (909 items, at most 5 per cell: the chain's four stages
    and one turn of the loop), 64x64 at 8 spp, in all three placements."""
    scene = rtow.final_scene()
    info = rtow.accel_info(scene, "lds")
    assert info["grid_placement"] == rtow.RT_GRID_LDS and info["max_items_per_cell"] == K + 1
    cam = rtow.camera_cpu(aspect=1.0)
    p = rtow.make_params(64, 64, 8, seed=71, flags=rtow.RT_FLAG_ACCEL_BVH | INTERVALS[interval])
    want, segs = kernel_render(scene, cam, p)
    for mode in MODES:
        got, st = render_pair(rtow, gpu_ctx, scene, cam, p, mode)
        same_bits(got, st, want, segs, mode)


@pytest.mark.parametrize("interval", list(INTERVALS))
@pytest.mark.parametrize("most", sorted(DENSE))
def test_dense_layers_fill_the_chain_and_the_loop(rtow, gpu_ctx, most, interval):
    """Crowded layers whose fullest cell holds exactly K - 1, K, K + 1 and 15
    items (asserted from the host's grid): the chain ends one stage early, on
    its last stage, hands one item to the pointer loop, and hands it eleven.
    The camera sees the whole crowd, 64x64 at 6 spp, in all three placements."""
    scene, scale, cam = dense(rtow, most)
    for mode, place in zip(MODES, (rtow.RT_GRID_LDS, rtow.RT_GRID_CELLS_LDS, rtow.RT_GRID_GLOBAL)):
        info = rtow.accel_info(scene, mode, scale)
        assert info["grid_placement"] == place and info["max_items_per_cell"] == most, (mode, info)
    p = rtow.make_params(64, 64, 6, seed=72, flags=rtow.RT_FLAG_ACCEL_BVH | INTERVALS[interval])
    want, segs = kernel_render(scene, cam, p)
    for mode in MODES:
        got, st = render_pair(rtow, gpu_ctx, scene, cam, p, mode, scale)
        same_bits(got, st, want, segs, (most, mode))


def corridor(rtow):
    """Two crowds either side of an empty strip |x| < 1.4, and a camera inside
    the layer's y-range looking straight down the strip (direction x nearly 0
    around the centre column; the pixel jitter keeps it from being exactly 0,
    which test_ray_fans_gpu.py's fans cover): its rays cross empty cells only
    (n = 0)."""
    rng = np.random.default_rng(7)
    side = rng.integers(0, 2, 80) * 2 - 1
    scene = crowd(rtow, side * rng.uniform(1.5, 3.0, 80), rng.uniform(-3.0, 3.0, 80), 0.1, 8)
    cam = rtow.camera_cpu(lookfrom=(0.0, 0.1, 6.0), lookat=(0.0, 0.1, -6.0), aspect=128 / 72, aperture=0.0)
    return scene, 0.5, cam


@pytest.mark.parametrize("interval", list(INTERVALS))
def test_empty_cells_along_an_axis_aligned_view(rtow, gpu_ctx, interval):
    scene, scale, cam = corridor(rtow)
    info = rtow.accel_info(scene, "lds", scale)
    assert info["grid_placement"] == rtow.RT_GRID_LDS
    # most listed cells are empty (the strip is 2.8 of the grid's ~6.2 width)
    assert 0 < info["listed_cells"] < (info["grid_nx"] - 2) * (info["grid_nz"] - 2) // 2, info
    p = rtow.make_params(128, 72, 4, seed=73, flags=rtow.RT_FLAG_ACCEL_BVH | INTERVALS[interval])
    want, segs = kernel_render(scene, cam, p)
    for mode in MODES:
        got, st = render_pair(rtow, gpu_ctx, scene, cam, p, mode, scale)
        same_bits(got, st, want, segs, mode)


# (sphere_tests, box_tests) of the renders below, recorded from the parent
# commit's build (the item loop before the chain) on an MI355X: a lane past
# its cell's end in a chain stage must not count as a test
PARENT_WORK = {
    ("final", "lds"): (660273, 122863),
    ("final", "cells"): (660273, 122863),
    ("final", "global"): (643933, 129602),
    ("dense15", "lds"): (1880711, 192409),
    ("dense3", "lds"): (278373, 44427),
}


def test_count_work_equals_the_parents(rtow, gpu_ctx):
    """RT_FLAG_COUNT_WORK: per-lane sphere tests and cell visits are what the
    item loop counted, and the counting build's image is still the oracle's."""
    flags = rtow.RT_FLAG_ACCEL_BVH | rtow.RT_FLAG_COUNT_WORK
    final = (rtow.final_scene(), None, rtow.camera_cpu(aspect=1.0))
    cases = [("final", m, final) for m in MODES] + [("dense15", "lds", dense(rtow, 15)),
                                                    ("dense3", "lds", dense(rtow, K - 1))]
    got_work = {}
    for name, mode, (scene, scale, cam) in cases:
        p = rtow.make_params(64, 64, 8, seed=74, flags=flags)
        got, st = render_pair(rtow, gpu_ctx, scene, cam, p, mode, scale)
        want, segs = kernel_render(scene, cam, p)
        same_bits(got, st, want, segs, (name, mode))
        got_work[(name, mode)] = (int(st.sphere_tests), int(st.box_tests))
    print("work counts:", got_work)
    assert got_work == PARENT_WORK


def test_wide_scene_keeps_its_cells_in_lds(rtow, gpu_ctx):
    """An albedo above 1 (64-bit sums: 3 KB more static LDS): the final scene's
    grid keeps only its cells in LDS, and the item loop reads global memory."""
    base = rtow.final_scene()
    alb = base.albedo.copy()
    alb[0] = (1.02, 1.02, 1.02)
    alb[int(np.nonzero(base.kind == rtow.RT_LAMBERTIAN)[0][5])] = (1.2, 1.5, 0.9)
    hot = dataclasses.replace(base, albedo=alb)
    assert rtow.accel_info(hot)["grid_placement"] == rtow.RT_GRID_CELLS_LDS
    cam = rtow.camera_cpu(aspect=1.0)
    for interval in INTERVALS.values():
        p = rtow.make_params(64, 64, 8, seed=75, flags=rtow.RT_FLAG_ACCEL_BVH | interval)
        want, segs = kernel_render(hot, cam, p)
        gpu_ctx.upload(hot)
        got, st = gpu_ctx.render(cam, p)
        same_bits(got, st, want, segs, interval)
