"""The class of a layer scene's first extras group (CPU, through
rt_internal_extras_info): which scenes take the folded forms of the grid
build's scan_extras, and that classifying moves no sphere.

-0 does not count as zero.  The bit argument in rt_device.h would cover it
(the dropped product is then -+0 instead of +-0, and a zero's sign reaches
neither e nor a root), but the class is one exact bit pattern per coordinate:
a centre spelt -0, like one of 1e-30, takes the general form.
"""
import numpy as np
import pytest

import extras_scenes
from extras_scenes import AXIAL, COAXIAL


def parent_order(scene, slots):
    """The extras as the builder has always laid them out: the spheres off the
    layer (here: the given ones), largest |radius| first, ties in index
    order, padded with -1 to a multiple of four."""
    idx = sorted(int(i) for i in slots if i >= 0)
    idx.sort(key=lambda i: -abs(float(scene.radius[i])))  # stable
    return idx + [-1] * (-len(idx) % 4)


def off_layer(scene):
    """Indices of the spheres that do not share the most common (cy, |r|)."""
    keys = list(zip(scene.cy.tolist(), np.abs(scene.radius).tolist()))
    best = max(set(keys), key=lambda k: (keys.count(k), ))
    return [i for i, k in enumerate(keys) if k != best]


@pytest.mark.parametrize("half_extent", [11, 50])
def test_final_scene_is_axial_and_coaxial(rtow, half_extent):
    scene = rtow.final_scene(half_extent=half_extent)
    fold, cy, slots = rtow.extras_info(scene)
    assert fold == AXIAL | COAXIAL
    assert cy.tobytes() == np.float32(1.0).tobytes()
    n = scene.n
    assert slots.tolist() == [0, n - 3, n - 2, n - 1] == parent_order(scene, off_layer(scene))
    assert rtow.RT_EXTRAS_AXIAL == AXIAL and rtow.RT_EXTRAS_COAXIAL == COAXIAL


def test_five_scene_has_no_class(rtow):
    fold, cy, slots = rtow.extras_info(rtow.five_scene())
    assert fold == 0 and cy.tobytes() == np.float32(0.0).tobytes() and slots.size == 0


@pytest.mark.parametrize("name", ["big_cz_quarter", "big_cy_one_ulp", "lead_cx_minus_zero", "lead_cx_tiny"])
def test_hand_made_scenes_lose_exactly_the_edited_part(rtow, name):
    """The edited part of the group takes the general form (its class bit is
    clear), the other part keeps its class, and the spheres stay where the
    unclassified builder put them (slot = tie key)."""
    scene, want = extras_scenes.hand_made(rtow)[name]
    fold, cy, slots = rtow.extras_info(scene)
    assert fold == want
    assert cy.tobytes() == np.float32(1.0 if want & COAXIAL else 0.0).tobytes()
    n = scene.n
    assert slots.tolist() == [0, n - 3, n - 2, n - 1] == parent_order(scene, off_layer(scene))


def test_minus_zero_is_not_zero_anywhere(rtow):
    """-0 in any coordinate the class reads as zero declines that part."""
    import dataclasses
    base = rtow.final_scene()
    for field, index, lost in (("cz", 0, AXIAL), ("cz", base.n - 1, COAXIAL), ("cz", base.n - 3, COAXIAL)):
        a = getattr(base, field).copy()
        a[index] = np.float32(-0.0)
        fold, _, _ = rtow.extras_info(dataclasses.replace(base, **{field: a}))
        assert fold == (AXIAL | COAXIAL) & ~lost, (field, index)
    # the big spheres' cx is free: -0 there changes nothing
    a = base.cx.copy()
    a[base.n - 3] = np.float32(-0.0)
    assert rtow.extras_info(dataclasses.replace(base, cx=a))[0] == AXIAL | COAXIAL


def test_random_scenes_with_extras(rtow):
    """final_prefix_65: the ground alone (axial; no other sphere to be
    coaxial with).  The final scene plus random spheres: three groups, the
    ground first; the random spheres next to it are not coaxial."""
    scenes = extras_scenes.random_with_extras(rtow)
    fold, _, slots = rtow.extras_info(scenes["final_prefix_65"])
    assert fold == AXIAL and slots.tolist() == [0, -1, -1, -1]
    scene = scenes["final_plus_free_3"]
    fold, _, slots = rtow.extras_info(scene)
    assert slots.size > 4 and slots.size % 4 == 0 and slots[0] == 0
    assert slots.tolist() == parent_order(scene, off_layer(scene))
    assert fold == AXIAL
    # the general render path's view of the same layout
    info = rtow.accel_info(scene)
    assert info["layer_mode"] == 1 and 2 * info["n_extra_pairs"] == slots.size
