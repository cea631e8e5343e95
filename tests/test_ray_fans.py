"""The coverage conditions of tests/ray_fans.py's case list, on the CPU oracle
(no GPU): that the hand-built cameras produce the rays they are there for.
These are conditions on the inputs, met by choosing eyes and fans, not
tolerances: test_ray_fans_gpu.py then checks every walk on the same list.

A hit sample's P is fma(t, d, o) per axis, so P[k] == eye[k] exactly iff
d[k] is +-0 (t > 0, d finite): kernel_terminals with keep_dir, which keeps a
camera ray's direction bits, shows the exact zeros on the first hits."""
import numpy as np
import pytest

import oracle_lib
import ray_fans as rf


def _first_hits(name, i):
    return rf.terminals_of(name, i, -1, keep_dir=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_list_has_every_kind_of_case(rtow):
    cases = rf.cases()
    for scene in rf.SCENES:
        assert rf.cases_of(scene), scene
    for scene in rf.LAYER_SCENES:
        info = rf.info_of(scene)
        assert info["layer_mode"] == 1 and info["grid_items"] > 0 and info["grid_ring_empty"] == 1, info
        own = rf.cases_of(scene)
        for key in ("border", "diagonal", "ring", "on_xi", "outside", "far", "layer", "neg"):
            assert any(c.get(key) for c in own.values()), (scene, key)
        zeros = {c["zero"] for c in own.values() if "zero" in c}
        assert zeros >= {(0,), (1,), (2,), (0, 2), (1, 2), (0, 1)}, zeros
    # the crowd's fullest cell goes past the item chain's four stages; the other two scenes walk the plain BVH
    assert rf.info_of("crowd")["max_items_per_cell"] > 4
    assert rf.info_of("final")["max_items_per_cell"] > 4
    for scene in ("final17", "five"):
        assert rf.info_of(scene)["layer_mode"] == 0, scene
    assert any(c["model"] == rf.GPU and len(c.get("zero", ())) == 1 for c in cases.values())
    for name, c in cases.items():
        w, h = c["frame"]
        assert (w, h) in ((32, 16), (8, 8)) and 2 <= c["spp"] <= 4 and c["cams"], name


def test_accel_info_gives_the_kernels_grid_geometry(rtow):
    """The new trailing values: the inner box lies inside the stored cells by
    one ring cell, borders 1 and n - 1 are its corners up to float32 rounding,
    and a scene without a grid reports zeros."""
    for scene in rf.LAYER_SCENES:
        info = rf.info_of(scene)
        g = info["grid_g"]
        assert g > 0 and info["grid_x0"] < info["grid_xi"] < info["grid_x1"]
        assert info["grid_z0"] < info["grid_zi"] < info["grid_z1"]
        for axis, lo, hi, n in ((0, "grid_xi", "grid_x1", "grid_nx"), (2, "grid_zi", "grid_z1", "grid_nz")):
            assert abs(float(rf.border(info, axis, 1)) - float(info[lo])) <= 4e-6 * abs(float(info[lo]))
            assert abs(float(rf.border(info, axis, info[n] - 1)) - float(info[hi])) <= 4e-6 * abs(float(info[hi]))
    five = rf.info_of("five")
    assert all(five[k] == 0 for k in rtow.ACCEL_INFO_GRID_KEYS)


def test_zero_component_fans_are_exactly_axis_parallel(rtow):
    """Every hit sample of a zero-component case has P[k] == eye[k] bit for
    bit on the case's zero axes; a -0 case's corner - eye has its sign bit set
    there on the host; and each such camera hits something."""
    n_cases = n_samples = 0
    some_neg = set()
    for name, c in rf.cases().items():
        if "zero" not in c:
            continue
        for i, (label, cam) in enumerate(c["cams"]):
            t = _first_hits(name, i)
            hit = t["sphere"] >= 0
            assert hit.any() or c.get("may_miss"), (name, label)
            for k in c["zero"]:
                eye = np.float32(cam.eye[k])
                assert (_bits(t["P"][..., k])[hit] == _bits(eye)).all(), (name, label, k)
                d = rf.direction_of(cam)[k]
                assert d == 0.0, (name, label, k, d)
                if c.get("neg") == "some":
                    some_neg.add((name, k) if np.signbit(d) else None)
                else:
                    assert bool(np.signbit(d)) == bool(c.get("neg")), (name, label, k, d)
            n_samples += int(hit.sum())
        if c.get("neg") == "some":
            assert any((name, k) in some_neg for k in c["zero"]), (name, some_neg)
        n_cases += 1
    print(f"zero-component cases: {n_cases}, hit samples with an exact zero: {n_samples}")
    assert n_cases >= 40


def test_layer_fans_walk_the_layer(rtow):
    """Per camera of a fan meant to walk the layer: at least 10 % of the
    samples first-hit a layer sphere, and at least 8 distinct ones appear."""
    seen = 0
    for name, c in rf.cases().items():
        if not c.get("layer"):
            continue
        lay = set(rf.layer_spheres(rf.scene_of(c["scene"])).tolist())
        for i, (label, cam) in enumerate(c["cams"]):
            first = _first_hits(name, i)["sphere"]
            on_layer = np.isin(first, list(lay))
            share, distinct = on_layer.mean(), len(set(first[on_layer].tolist()))
            print(f"{name} [{label}]: {share:.1%} of {first.size} samples on {distinct} layer spheres")
            assert share >= 0.10 and distinct >= 8, (name, label, share, distinct)
            seen += 1
    assert seen >= 20


def test_border_eyes_sit_on_the_walks_borders(rtow):
    """The eye's coordinate equals fmaf(k, g, x0) bit for bit, k interior; the
    on-xi eye equals grid_xi; the diagonal rays have |dx| == |dz| exactly and
    start on a cell corner; ring eyes lie in the ring and outside eyes outside
    the stored cells, their centre ray through an inner-box corner."""
    for name, c in rf.cases().items():
        info = rf.info_of(c["scene"])
        g = float(info["grid_g"])
        lo = (float(info["grid_x0"]), 0.0, float(info["grid_z0"]))
        inner = ((float(info["grid_xi"]), float(info["grid_x1"])), None, (float(info["grid_zi"]), float(info["grid_z1"])))
        n = (info["grid_nx"], 0, info["grid_nz"])
        if "border" in c:
            axis, ks = c["border"]
            assert len(ks) == len(c["cams"]) and len(set(ks)) == 3
            for k, (label, cam) in zip(ks, c["cams"]):
                assert 2 <= k <= n[axis] - 2
                assert _bits(np.float32(cam.eye[axis])) == _bits(rf.border(info, axis, k)), (name, label)
            other = 2 if axis == 0 else 0
            # the eye looks back over the scene from either end: both signs of the other horizontal component
            assert {float(np.sign(cam.eye[other])) for _, cam in c["cams"]} == {-1.0, 1.0}
        if c.get("on_xi"):
            for label, cam in c["cams"]:
                assert _bits(np.float32(cam.eye[0])) == _bits(info["grid_xi"]), (name, label)
        if c.get("diagonal"):
            signs = set()
            for label, cam in c["cams"]:
                d = rf.direction_of(cam)
                assert abs(d[0]) == abs(d[2]) and d[0] != 0, (name, label, d)
                signs.add((float(np.sign(d[0])), float(np.sign(d[2]))))
                assert _bits(np.float32(cam.eye[0])) == _bits(rf.border(info, 0, n[0] // 2))
                assert _bits(np.float32(cam.eye[2])) == _bits(rf.border(info, 2, n[2] // 2))
            assert len(signs) == 4
        if c.get("ring"):
            for i, (label, cam) in enumerate(c["cams"]):
                out = [k for k in (0, 2) if not inner[k][0] <= cam.eye[k] <= inner[k][1]]
                assert len(out) == 1, (name, label)
                k = out[0]
                assert lo[k] < cam.eye[k] < lo[k] + n[k] * g and min(abs(cam.eye[k] - inner[k][0]),
                                                                     abs(cam.eye[k] - inner[k][1])) < g, (name, label)
                assert (_first_hits(name, i)["sphere"] > 0).mean() > 0.1, (name, label)  # it looks in, at the layer
        if c.get("outside"):
            for label, cam in c["cams"]:
                assert all(not lo[k] <= cam.eye[k] <= lo[k] + n[k] * g for k in (0, 2)), (name, label)
                # the centre ray (fs = ft = 0.5) crosses x = corner x and z = corner z at one parameter
                eye = np.array(cam.eye[:], np.float64)
                d = (np.array(cam.corner[:], np.float64) + 0.5 * np.array(cam.horiz[:], np.float64) +
                     0.5 * np.array(cam.vert[:], np.float64)) - eye
                hits = [(cx, cz) for cx in inner[0] for cz in inner[2]
                        if abs((cx - eye[0]) / d[0] - (cz - eye[2]) / d[2]) < 1e-5 and (cx - eye[0]) / d[0] > 0]
                assert hits, (name, label)


def test_far_cases_lie_beyond_oref(rtow):
    """Whole-far cases: every sample's origin has |O|^2 > oref2, computed in
    float32 as the kernel does.  The mixed case: in every 8x8 tile at least one
    sample lies on each side of oref2 (the float32 the host uploads), with the
    origins taken from the oracle's own camera_ray."""
    n_whole = n_mixed = 0
    for name, c in rf.cases().items():
        if "far" not in c:
            continue
        oref2 = rf.oref2_of(c["scene"])
        (label, cam), = c["cams"]
        o = oracle_lib.camera_origins(cam, rf.params_of(c))
        f = np.float32
        # dot3 as the kernel's: fma(z, z, fma(y, y, x x)) in float32 (float64 products of float32 are exact;
        # each sum is rounded once)
        o64 = o.astype(np.float64)
        o2 = f(f(o64[..., 0] * o64[..., 0]))
        o2 = (o64[..., 1] * o64[..., 1] + o2.astype(np.float64)).astype(f)
        o2 = (o64[..., 2] * o64[..., 2] + o2.astype(np.float64)).astype(f)
        beyond = o2 > oref2
        if c["far"] == "whole":
            assert beyond.all() and np.isfinite(o2).all(), (name, float(o2.min()), float(oref2))
            assert (o == np.array(cam.eye[:], np.float32)).all()
            assert (_first_hits(name, 0)["sphere"] >= 0).mean() > 0.5, name  # it looks at the scene
            n_whole += 1
        else:
            h, w = beyond.shape[:2]
            tiles = beyond.reshape(h // 8, 8, w // 8, 8, -1).transpose(0, 2, 1, 3, 4).reshape(h // 8 * (w // 8), -1)
            share = tiles.mean(1)
            print(f"{name}: share of origins beyond oref2 per 8x8 tile {share.min():.2f} .. {share.max():.2f}")
            assert (tiles.any(1) & ~tiles.all(1)).all(), name
            # margins an ulp of the dot product cannot close: the test's own float32 restatement is not at issue
            assert (np.abs(o2 - oref2) > 1e-3).mean() > 0.99
            n_mixed += 1
    assert n_whole >= 8 and n_mixed >= 4
