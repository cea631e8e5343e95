"""Scenes for the extras-fold tests (test infrastructure): the final scene
with its first extras group (the ground and the three big spheres) edited so
that one part of the group falls out of its class, and scenes from
random_scenes.py that have extras."""
import dataclasses

import numpy as np

import random_scenes

AXIAL, COAXIAL = 1, 2  # rtow.RT_EXTRAS_*


def _edit(scene, field, index, value):
    a = getattr(scene, field).copy()
    a[index] = value
    return dataclasses.replace(scene, **{field: a})


def hand_made(rtow):
    """name -> (scene, expected class bits).  The final scene's ground is
    sphere 0, its big spheres are the last three (centres (0, 1, 0), (-4, 1,
    0), (4, 1, 0))."""
    base = rtow.final_scene()
    n = base.n
    f32 = np.float32
    return {
        # a big sphere off the x axis: the ground stays axial
        "big_cz_quarter": (_edit(base, "cz", n - 2, f32(0.25)), AXIAL),
        # a big sphere whose centre y is the next float32 above 1
        "big_cy_one_ulp": (_edit(base, "cy", n - 1, np.nextafter(f32(1.0), f32(2.0))), AXIAL),
        # only +0 is zero: -0 and 1e-30 take the general form; the big spheres stay coaxial
        "lead_cx_minus_zero": (_edit(base, "cx", 0, f32(-0.0)), COAXIAL),
        "lead_cx_tiny": (_edit(base, "cx", 0, f32(1e-30)), COAXIAL),
    }


def random_with_extras(rtow):
    """Two scenes of random_scenes.py that have extras.  Its only layer scene
    with extras is final_prefix_65 (the ground alone: three padding slots);
    the second is free_scene(3)'s spheres (overlapping, negative radii, a
    second ground) appended to the final scene, where they are extras."""
    out = {"final_prefix_65": random_scenes.degenerate_scenes(rtow)["final_prefix_65"]}
    base, free = rtow.final_scene(), random_scenes.free_scene(rtow, 3)
    keep = np.arange(min(free.n, 10))
    out["final_plus_free_3"] = rtow.Scene(*(np.concatenate([getattr(base, f), getattr(free, f)[keep]])
                                            for f in ("cx", "cy", "cz", "radius", "kind", "albedo", "param")))
    return out
