"""Every walk of all four tracing code objects on tests/ray_fans.py's cases:
exactly axis-parallel rays (the +-1e18 clamp of 1/d, the step direction from
the sign of a zero, the DDA's huge or residual boundary times, the layer's
y-slab with 1/dy clamped), eyes on cell borders and corners, in the grid's
ring and outside its box, and ray origins beyond oref (a wave scans when any
lane's origin is).  test_ray_fans.py shows on the CPU that the cases produce
those rays.  Every comparison is tobytes() equality with the oracle's kernel
mode (a brute-force scan that knows no walk) plus the segment count: no
tolerance, no masked pixel."""
import numpy as np
import pytest

import features_ref
import ray_fans as rf
import route_ref
from test_features_oracle_gpu import _check

pytestmark = pytest.mark.gpu

BVH, LAYER_BVH = 1 << 9, (1 << 9) | (1 << 12)  # RT_FLAG_ACCEL_BVH, + RT_FLAG_LAYER_BVH
INTERVALS = (0, 1)  # RT_FLAG_OPEN_INTERVAL off and on
# (name, accel flags, grid placement) per kind of scene
LAYER_WALKS = (("scan", 0, None), ("layer_bvh", LAYER_BVH, None), ("grid-lds", BVH, "lds"),
               ("grid-cells", BVH, "cells"), ("grid-global", BVH, "global"))
PLAIN_WALKS = (("scan", 0, None), ("bvh", BVH, None))
RENDERS = [(s, w) for s in rf.SCENES for w in (LAYER_WALKS if s in rf.LAYER_SCENES else PLAIN_WALKS)]


def _upload(rtow, ctx, scene_name, mode=None):
    ctx.upload(rf.scene_of(scene_name), grid_mode=mode)


def _defaults(rtow, ctx):
    ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, rtow.RT_GRID_AUTO)
    ctx.set_option(rtow.RT_OPT_GRID_SCALE, 0.0)


@pytest.mark.parametrize("scene_name,walk", RENDERS, ids=[f"{s}-{w[0]}" for s, w in RENDERS])
def test_render_is_the_oracles(rtow, gpu_ctx, scene_name, walk):
    """Every camera of every case of the scene, both intervals, in one walk."""
    _, accel, mode = walk
    if mode is not None:
        assert rtow.accel_info(rf.scene_of(scene_name), mode)["grid_placement"] == rtow.GRID_PLACEMENTS[mode]
    elif accel:
        assert rf.info_of(scene_name)["layer_mode"] == (1 if scene_name in rf.LAYER_SCENES else 0)
    n = 0
    try:
        _upload(rtow, gpu_ctx, scene_name, mode)
        for name, c in rf.cases_of(scene_name).items():
            for i, (label, cam) in enumerate(c["cams"]):
                for interval in INTERVALS:
                    want, segs = rf.want_of(name, i, interval)
                    got, st = gpu_ctx.render(cam, rf.params_of(c, interval, accel))
                    what = (name, label, interval, walk[0])
                    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))
                    assert st.segments == segs, what
                    n += 1
    finally:
        _defaults(rtow, gpu_ctx)
    assert n >= 40


PASSES = ("aov", "guides", "route")
ROUTE_ALL = features_ref.ROUTE + ("state",)


@pytest.mark.parametrize("which", PASSES)
@pytest.mark.parametrize("scene_name", rf.LAYER_SCENES)
def test_feature_passes_are_the_oracles(rtow, gpu_ctx, scene_name, which):
    """rt_aov, rt_guides and rt_route (each compiles closest_hit on its own)
    on the same cameras, the default layer-grid walk, at the default 8 bounces
    and at 2, against the sums, the route state and its finalize restated from
    the oracle's terminals."""
    gpu_ctx.upload(rf.scene_of(scene_name))
    for name, c in rf.cases_of(scene_name).items():
        p = rf.params_of(c, 0, BVH)
        for i, (label, cam) in enumerate(c["cams"]):
            what = "%s [%s] rt_%s" % (name, label, which)
            if which == "aov":
                term = rf.terminals_of(name, i, -1, keep_dir=True)
                _check(gpu_ctx.aov(cam, p), features_ref.sums(term), features_ref.AOV, term, what)
                continue
            for mb in (8, 2):
                term = rf.terminals_of(name, i, mb)
                opt = None if mb == 8 else mb
                if which == "guides":
                    _check(gpu_ctx.guides(cam, p, max_bounces=opt), features_ref.sums(term), features_ref.GUIDES, term,
                           "%s max_bounces %d" % (what, mb))
                else:
                    state = features_ref.route_state(term)
                    got = gpu_ctx.route(cam, p, which=ROUTE_ALL, max_bounces=opt)
                    assert got["state"].tobytes() == state.tobytes(), (what, mb)
                    _check(got, route_ref.finalize(state), features_ref.ROUTE, term, "%s max_bounces %d" % (what, mb),
                           features_ref.route_outputs)


def _n_pad(scene):
    return -(-scene.n // 8) * 8  # kSpherePad: the scan's slots, whole groups of 8


@pytest.mark.parametrize("scene_name", list(rf.SCENES))
def test_far_origins_scan(rtow, gpu_ctx, scene_name):
    """RT_FLAG_COUNT_WORK on the far cases.  A wave-step scans when any of its
    lanes starts beyond oref2, and the scan adds n_pad tests per segment.

    Whole-far cameras at max_depth 1 trace primary rays only, all from beyond
    oref: exactly the scan's work, sphere_tests == n_pad x segments and no box
    test.  (At depth 50 the bounces start inside oref and walk once a wave
    holds no camera ray, so the identity is the depth-1 render's; the depth-50
    image of the counting build is checked as well.)

    The mixed camera at depth 50: its camera rays start on both sides of oref2
    in every wave, so those wave-steps scan, and its bounce-only wave-steps
    walk: sphere_tests lies strictly between a render of the same camera moved
    to 0.5 oref (all walk) and n_pad x segments.  The counting build's image
    is still the oracle's."""
    scene = rf.scene_of(scene_name)
    n_pad = _n_pad(scene)
    flags = BVH | rtow.RT_FLAG_COUNT_WORK
    gpu_ctx.upload(scene)
    for name, c in rf.cases_of(scene_name).items():
        if "far" not in c:
            continue
        (label, cam), = c["cams"]
        want, segs = rf.want_of(name, 0, 0)
        got, st = gpu_ctx.render(cam, rf.params_of(c, 0, flags))
        print(f"{name}: depth 50: segments {st.segments}, sphere_tests {st.sphere_tests} "
              f"(n_pad x segments {n_pad * st.segments}), box_tests {st.box_tests}")
        assert got.tobytes() == want.tobytes() and st.segments == segs, name
        if c["far"] == "whole":
            _, st1 = gpu_ctx.render(cam, rf.params_of(c, 0, flags, max_depth=1))
            print(f"{name}: depth 1: segments {st1.segments}, sphere_tests {st1.sphere_tests}, box_tests {st1.box_tests}")
            w, h = c["frame"]
            assert st1.segments == w * h * c["spp"], name
            assert st1.sphere_tests == n_pad * st1.segments and st1.box_tests == 0, name
            assert st.sphere_tests <= n_pad * st.segments, name
        elif n_pad >= 64:  # (the five-sphere scene's walk is no cheaper than its scan of 8 slots: image only)
            near = rf.mixed_camera(scene_name, 0.5, c["look"])
            _, stn = gpu_ctx.render(near, rf.params_of(c, 0, flags))
            print(f"{name}: at 0.5 oref: segments {stn.segments}, sphere_tests {stn.sphere_tests}")
            assert stn.sphere_tests < st.sphere_tests < n_pad * st.segments, name
