"""The case lists of rt_bounce's tests (test infrastructure), shared by
test_bounce.py, which shows on the CPU oracle that the lists meet every
situation the checks are there for, and test_bounce_gpu.py, which runs the
pass on them.  The scenes, cameras and frames are tests/features_cases.py's;
this module adds the render's depth caps, the walks of a scene, and the two
numpy loops over Context.bounce that the judges compare: rtow.path_trace's
render (in rtow.py, the worked example) and the specular chain below."""
import copy

import numpy as np

import features_cases as fc
import oracle_lib

# the render judge: every case with narrow pixel sums.  An albedo above 1 makes a render's sums wide (64-bit, a
# clamped sample radiance), which rtow.path_trace does not restate: clamp's mirrors (3.0) and the hot scene's (1.3)
WIDE_CASES = ("clamp", "hot", "hot-gpusem")
RENDER_CASES = tuple(c for c in fc.CASES if c not in WIDE_CASES)
DEPTHS = (50, 3)
# the chain judge: clamp and glassground bring the 2^100 clamp and both skip arms inside a chain
CHAIN_CASES = tuple(fc.CASES)
CHAIN_BOUNCES = (-1, 1, 2, 8)
CLAMP_BOUNCES = 64  # the clamp case once more: 3.0^64 > 2^100 needs a chain this long to reach the clamp
CHAIN_FUZZ = (0.0, 0.3)
# camera rays: the lens model, the pinhole model, a banded frame
CAMERA_CASES = ("final-lens", "five-pinhole", "final-bands", "mirror")

BVH, LAYER_BVH = 1 << 9, (1 << 9) | (1 << 12)
LAYER_WALKS = (("scan", 0, None), ("layer_bvh", LAYER_BVH, None), ("grid-lds", BVH, "lds"),
               ("grid-cells", BVH, "cells"), ("grid-global", BVH, "global"))
PLAIN_WALKS = (("scan", 0, None), ("bvh", BVH, None))
WALK_BITS = BVH | LAYER_BVH


def is_layer_scene(rtow, case):
    return rtow.accel_info(fc.scene_of(rtow, case))["layer_mode"] != 0


def walks_of(rtow, case):
    """(name, acceleration flags, grid placement or None) of every walk the case's scene has."""
    return LAYER_WALKS if is_layer_scene(rtow, case) else PLAIN_WALKS


def params_of(rtow, case, frame, max_depth=50, accel=None):
    """features_cases' params with a depth cap and, when given, another walk's flags."""
    p = copy.copy(fc.params_of(rtow, case, frame))
    p.max_depth = max_depth
    if accel is not None:
        p.flags = (p.flags & ~WALK_BITS) | accel
    return p


def chain(rtow, ctx, cam, p, max_bounces, max_fuzz):
    """rt_guides' specular chain as a loop over Context.bounce -> records of
    oracle_lib.TERMINAL (events left 0): follow a dielectric, and a scattered
    metal whose fuzz is <= max_fuzz, for at most max_bounces bounces;
    total += t and thr = fmin(thr * attenuation, 2^100) in float32 per counted
    hit."""
    f32 = np.float32
    scene = ctx.scene
    n = p.local_rows * p.width * p.spp
    rec = np.zeros(n, oracle_lib.TERMINAL)
    rec["sphere"] = -1
    if n == 0:
        return rec.reshape(p.local_rows, p.width, p.spp)
    o, d, key = ctx.camera_rays(cam, p)
    live = np.nonzero(np.repeat(rtow.local_to_global_rows(p) < p.height, p.width * p.spp))[0]
    o, d, key, frm = o[live], d[live], key[live], np.full(live.size, -1, np.int32)
    thr, total, nb = np.ones((live.size, 3), f32), np.zeros(live.size, f32), np.zeros(live.size, np.uint32)
    fuzz = np.minimum(scene.param.astype(f32), f32(1.0))
    while live.size:
        got = ctx.bounce(o, d, key, p.seed, frm, flags=p.flags)
        assert not (got["status"] == rtow.BOUNCE_INVALID).any()
        hit = got["id"] >= 0
        rec["escaped"][live[~hit]] = frm[~hit] >= 0  # left the scene: the terminal is the last counted hit
        thr = np.minimum(thr * got["attenuation"], f32(2.0 ** 100))
        total = total + np.where(hit, got["t"], f32(0.0))
        h = live[hit]
        rec["sphere"][h], rec["depth"][h], rec["P"][h], rec["N"][h] = got["id"][hit], total[hit], got["position"][hit], got["normal"][hit]
        rec["thr"][h], rec["bounces"][h] = thr[hit], nb[hit]
        kind = scene.kind[np.maximum(got["id"], 0)]
        cont = hit & ((kind >= 2) | ((kind == 1) & (got["status"] == rtow.BOUNCE_SCATTERED) &
                                     (fuzz[np.maximum(got["id"], 0)] <= f32(max_fuzz))))
        on = cont & (nb < max(max_bounces, 0))
        assert (got["status"][on] == rtow.BOUNCE_SCATTERED).all()
        rec["bounces"][live[on]] = nb[on] + np.uint32(1)  # a bounce followed counts whether or not it hits again
        key = key[on] + np.array([0, 0, 1], np.uint32)
        live, o, d, frm = live[on], got["position"][on], got["scatter"][on], got["id"][on]
        thr, total, nb = thr[on], total[on], nb[on] + np.uint32(1)
    return rec.reshape(p.local_rows, p.width, p.spp)


CHAIN_FIELDS = ("sphere", "depth", "P", "N", "thr", "bounces", "escaped")
