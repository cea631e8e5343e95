"""Feature buffers that follow mirror and glass paths, on the GPU
(include/rt_guides.h, rt_guides / Context.guides): with nothing followed the
pass is rt_aov, byte for byte; its routing through specular surfaces is the
render's (exact, against renders of a scene whose rough surfaces are black);
the throughput is the product of the albedos on the path (exact); a one-bounce
mirror image agrees with an fp64 solution within a tolerance derived from the
kernel's own sphere arithmetic; one answer from every walk, placement, launch
split and band partition; and the denoiser takes the buffers as they are."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
from mirror_room import A_MIRROR, left_out64, mirror_room, mirror_room_camera, roots64, second_hop64
from oracle_lib import read_ppm_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ray-tracing-in-one-weekend_amd", "bin")
FRAMES = ((67, 37), (5, 3), (1, 1))
AOV = ("hits", "id", "depth", "position", "normal", "albedo")
NAMES = AOV + ("bounces", "escaped")
FIVE_VIEW = dict(lookfrom=(-2.0, 0.5, 2.0), lookat=(0.0, 0.0, -1.0), vfov=40.0, focus_dist=3.4)


def _scene(rtow, name):
    return rtow.final_scene() if name == "final" else rtow.five_scene()


def _camera(rtow, scene_name, model, w, h):
    view = FIVE_VIEW if scene_name == "five" else dict(focus_dist=10.0)
    if model == "cpu_lens":
        return rtow.camera_cpu(aspect=w / h, aperture=0.1, **view)
    return rtow.camera_gpu(w, h, defocus_angle=0.0, **view)


def _same(a, b, names=NAMES):
    return all(a[n].tobytes() == b[n].tobytes() for n in names)


def _copy(rtow, s, **changes):
    d = dict(cx=s.cx.copy(), cy=s.cy.copy(), cz=s.cz.copy(), radius=s.radius.copy(), kind=s.kind.copy(),
             albedo=s.albedo.copy(), param=s.param.copy())
    d.update(changes)
    return rtow.Scene(**d)


def _continues(rtow, scene, max_fuzz):
    """Spheres that can continue a chain: dielectrics, and metals with clamped fuzz <= max_fuzz."""
    return (scene.kind == rtow.RT_DIELECTRIC) | ((scene.kind == rtow.RT_METAL) &
                                                  (np.minimum(scene.param, np.float32(1.0)) <= np.float32(max_fuzz)))


@pytest.fixture
def ctx(rtow, gpu_ctx):
    """The session's context with its options at their defaults afterwards."""
    yield gpu_ctx
    gpu_ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_SCALE, 0)


# ---- 1. nothing followed: rt_aov ------------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("model", ["cpu_lens", "gpu_pinhole"])
@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_guides_without_bounces_are_rt_aov(rtow, ctx, scene_name, model, flags):
    """max_bounces = 0 (the struct's -1): rt_aov's six buffers byte for byte,
    bounces = escaped = 0.  At every max_bounces, hits is rt_aov's hits."""
    ctx.upload(_scene(rtow, scene_name))
    for w, h in FRAMES:
        cam = _camera(rtow, scene_name, model, w, h)
        p = rtow.make_params(w, h, 5, seed=11, flags=flags | rtow.RT_FLAG_ACCEL_BVH)
        if model == "cpu_lens" and min(w, h) < 2:  # that camera model needs two pixels each way: rt_aov's check
            for call in (ctx.aov, ctx.guides):
                with pytest.raises(rtow.RTError) as e:
                    call(cam, p)
                assert e.value.status == rtow.RT_ERR_INVALID
            continue
        want = ctx.aov(cam, p)
        got = ctx.guides(cam, p, max_bounces=0)
        assert sorted(got) == sorted(NAMES + ("kernel_ms",))
        assert _same(want, got, AOV), (w, h)
        assert not got["bounces"].any() and not got["escaped"].any()
        followed = 0
        for mb in (1, 2, None, 64):
            g = ctx.guides(cam, p, max_bounces=mb)
            assert g["hits"].tobytes() == want["hits"].tobytes(), (w, h, mb)
            assert np.all(g["escaped"] <= g["hits"]) and np.all(g["bounces"] <= g["hits"] * (mb or 8))
            assert np.all(g["bounces"] >= g["escaped"])
            followed += int(g["bounces"].sum())
        if (w, h) == FRAMES[0]:
            assert followed > 0  # both scenes show glass or a mirror


_BOTH_LIBRARIES_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import rtow
rtow.aov_lib(), rtow.guides_lib()  # both loaded before either pass runs
AOV = ("hits", "id", "depth", "position", "normal", "albedo")
view = dict(lookfrom=(-2.0, 0.5, 2.0), lookat=(0.0, 0.0, -1.0), vfov=40.0, focus_dist=3.4)
p = rtow.make_params(16, 16, 2, seed=11, flags=rtow.RT_FLAG_ACCEL_BVH)
lens, pinhole = (rtow.camera_cpu(aspect=1.0, aperture=a, **view) for a in (0.1, 0.0))
with rtow.Context(0) as ctx:
    ctx.upload(rtow.five_scene())
    calls = {"aov": ctx.aov, "guides": lambda cam, p: ctx.guides(cam, p, max_bounces=0)}
    got = {name: calls[name](lens, p) for name in sys.argv[2:]}  # in the order under test
    for n in AOV:
        assert got["aov"][n].tobytes() == got["guides"][n].tobytes(), n
    for name in got:
        sharp = calls[name](pinhole, p)
        assert (got[name]["hits"] > 0).any()
        assert got[name]["position"].tobytes() != sharp["position"].tobytes(), name
print("ok")
"""


@pytest.mark.parametrize("order", [("guides", "aov"), ("aov", "guides")])
def test_both_libraries_in_one_process_upload_their_own_lens_table(order):
    """librtow_aov.so and librtow_guides.so each hold a lens table of their own
    (g_turn_tab, one per code object) and upload it on their first pass from the
    one ensure_turn_table of csrc/rt_trace_pass.h.  Were its "done" state shared
    between the libraries, the one called second would trace lens samples from
    a table of zeros.  A fresh process per order, both libraries loaded, the
    five-sphere scene through a lens camera (aperture 0.1), 16x16, 2 spp, BVH
    flag: rt_guides with nothing followed (Context.guides(max_bounces=0), the
    struct's -1) and rt_aov give the same bytes in all six shared buffers, and
    each pass's positions differ from the same call with aperture 0."""
    pkg = os.path.join(ROOT, "ray-tracing-in-one-weekend_amd")
    r = subprocess.run([sys.executable, "-c", _BOTH_LIBRARIES_CHILD, pkg, *order], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


# ---- 2. a scene with nothing to follow ------------------------------------
def test_guides_of_a_rough_scene_are_rt_aov(rtow, ctx):
    """The final scene with its dielectrics made lambertian and every metal's
    fuzz raised to at least 0.1: at the defaults nothing continues a chain."""
    s = rtow.final_scene()
    diel = s.kind == rtow.RT_DIELECTRIC
    kind = np.where(diel, rtow.RT_LAMBERTIAN, s.kind).astype(np.uint32)
    param = np.where(diel, 0.0, np.where(s.kind == rtow.RT_METAL, np.maximum(s.param, 0.1), s.param)).astype(np.float32)
    rough = _copy(rtow, s, kind=kind, param=param)
    assert diel.any() and ((s.kind == rtow.RT_METAL) & (s.param == 0)).any()
    assert not _continues(rtow, rough, 0.0).any()
    ctx.upload(rough)
    w, h = FRAMES[0]
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    p = rtow.make_params(w, h, 5, seed=4, flags=rtow.RT_FLAG_ACCEL_BVH)
    want, got = ctx.aov(cam, p), ctx.guides(cam, p)
    assert _same(want, got, AOV) and (want["hits"] > 0).any()
    assert not got["bounces"].any() and not got["escaped"].any()


# ---- 3. routing is the render's -------------------------------------------
def _routing(rtow, ctx, scene_name, seeds, bounces, max_fuzz, flags):
    scene = _scene(rtow, scene_name)
    go_on = _continues(rtow, scene, max_fuzz)
    assert go_on.any() and (~go_on).any()
    twin = _copy(rtow, scene, albedo=np.where(go_on[:, None], scene.albedo, np.float32(0.0)).astype(np.float32))
    # the darkest escaping sample: the smallest tint on the chain, B times, under the darkest sky (0.5)
    tint = float(np.where((scene.kind == rtow.RT_DIELECTRIC)[:, None], 1.0, scene.albedo)[go_on].min())
    assert tint ** max(bounces) * 0.5 > 1024 * 2.0 ** -31
    if scene_name == "final" and max_fuzz == 0.0:
        m = go_on & (scene.kind == rtow.RT_METAL)
        assert m.sum() == 1 and np.array_equal(scene.albedo[m][0], np.array(A_MIRROR, np.float32))
    w, h = FRAMES[0]
    cam = _camera(rtow, scene_name, "cpu_lens", w, h)
    for seed in seeds:
        for B in bounces:
            p = rtow.make_params(w, h, 1, max_depth=B + 1, seed=seed, flags=flags | rtow.RT_FLAG_ACCEL_BVH)
            ctx.upload(scene)
            g = ctx.guides(cam, p, max_bounces=B, max_fuzz=max_fuzz)
            ctx.upload(twin)
            img, _ = ctx.render(cam, p)
            ref, _ = oracle_lib.kernel_render(twin, cam, p)
            assert np.array_equal(img, ref), (seed, B)
            lit = (img > 0).all(-1)
            assert np.array_equal(lit, (img > 0).any(-1))
            want = (g["hits"] == 0) | (g["escaped"] == 1)
            assert np.array_equal(lit, want), (scene_name, seed, B, int((lit != want).sum()))
            assert np.all(g["escaped"] <= g["hits"]) and np.all(g["bounces"] <= B)
            if B == 0:
                assert not g["escaped"].any()
            elif B >= 2:
                assert (g["escaped"] == 1).any() and (g["bounces"] >= 2).any()


@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_guides_routing_is_the_renders(rtow, ctx, scene_name):
    """The black-terminal twin of a scene: every sphere that cannot continue a
    chain (lambertians, metals with fuzz > max_fuzz) gets albedo 0; geometry,
    kinds and params stay.  A sample's radiance in a render of the twin at
    max_depth = B + 1 is then > 0 exactly when its chain leaves the scene within
    B bounces: at spp 1, (render > 0) == (hits == 0) | (escaped == 1) for every
    pixel, with the product's render, which the oracle's equals."""
    _routing(rtow, ctx, scene_name, (1, 2, 3), (0, 1, 2, 5), 0.0, 0)


def test_guides_routing_with_fuzzy_metals_and_gpu_semantics(rtow, ctx):
    """Once more with max_fuzz = 0.3 (fuzzy metals continue the chain: the
    metal block's unit vector, ball radius and absorption test are on the path)
    and RT_FLAG_GPU_SEMANTICS (open interval, RT_FLAG_METAL_UNIT_VECTOR)."""
    s = rtow.final_scene()
    fuzzy = (s.kind == rtow.RT_METAL) & (s.param > 0) & (s.param <= np.float32(0.3))
    assert fuzzy.any()
    _routing(rtow, ctx, "final", (1,), (1, 2, 5), 0.3, rtow.RT_FLAG_GPU_SEMANTICS)
    _routing(rtow, ctx, "final", (2,), (2,), 0.3, 0)


# ---- 4. / 5. the mirror room ----------------------------------------------
def _mirror_room_pass(rtow, ctx):
    w, h = FRAMES[0]
    scene = mirror_room(rtow)
    ctx.upload(scene)
    cam = mirror_room_camera(rtow, w, h)
    p = rtow.make_params(w, h, 1, seed=3, flags=rtow.RT_FLAG_ACCEL_BVH)
    return scene, cam, ctx.aov(cam, p), ctx.guides(cam, p)


def test_guides_throughput_is_exact(rtow, ctx):
    """Mirror room, spp 1: a pixel with one bounce that ended on a surface has
    albedo f32(f32(1 a_mirror) a_id) componentwise; one whose chain escaped has
    a_mirror and the mirror's id, position and normal."""
    scene, cam, aov, g = _mirror_room_pass(rtow, ctx)
    assert np.array_equal(g["hits"], aov["hits"])
    one = (g["bounces"] == 1) & (g["escaped"] == 0)
    esc = g["escaped"] == 1
    assert one.sum() >= 40 and esc.sum() >= 10 and g["bounces"].max() == 1
    am = np.array(A_MIRROR, np.float32) * np.float32(1.0)
    ids = g["id"][one]
    assert (ids > 0).all() and len(np.unique(ids)) >= 3
    assert np.array_equal(g["albedo"][one], am[None, :] * scene.albedo[ids])
    assert np.all(g["albedo"][esc] == am) and np.all(g["id"][esc] == 0)
    for n in ("position", "normal", "depth"):
        assert g[n][esc].tobytes() == aov[n][esc].tobytes(), n
    # only the mirror's pixels bounced (all but at most a few at its limb, where
    # the reflection may round into the surface: absorbed); the others are rt_aov's
    assert not g["bounces"][aov["id"] != 0].any()
    assert (g["bounces"] == 1).sum() >= 0.97 * (aov["id"] == 0).sum()
    rest = g["bounces"] == 0
    for n in AOV:
        assert g[n][rest].tobytes() == aov[n][rest].tobytes(), n


def test_guides_one_bounce_geometry_against_fp64(rtow, ctx):
    """Mirror room, spp 1, a pinhole camera.  rt_aov gives each mirror pixel's
    first hit M and normal N_M for the same ray; in fp64, d = normalize(M -
    eye), r = d - 2 (d.N) N, and the nearest root past t_min over all spheres
    is the expected id, P, N and depth = |M - eye| + t.

    tol, as in test_aov_geometry_against_fp64: the largest deviation of
    rt_device_kat(RT_KAT_SPHERE_HIT) from fp64 on both hops' cases, times 8,
    times the growth of a direction error over the second hop, 1 + 2 t /
    |r_mirror|, floored at 4 ulp32 of the largest coordinate; the one bound
    holds for P, N and depth.  Rays with
    two offers within tol or passing a limb within tol are left out: at most
    1 % of the one-bounce pixels (on the CPU, with pixel-centre rays, the fp64
    side leaves out 0 of 110 at this frame size).  Measured on the MI355X: 112
    pixels, none left out, KAT deviation 4.17e-6, tol 2.44e-4 .. 1.63e-3, the
    largest deviation 0.026 of its bound."""
    scene, cam, aov, g = _mirror_room_pass(rtow, ctx)
    f8 = np.float64
    one = (g["bounces"] == 1) & (g["escaped"] == 0) & (aov["id"] == 0)
    assert one.sum() >= 40
    eye = np.array(cam.eye[:], f8)
    C = np.stack([scene.cx, scene.cy, scene.cz], -1).astype(f8)
    R = scene.radius.astype(f8)
    M, NM = aov["position"][one].astype(f8), aov["normal"][one].astype(f8)
    offer, r, limb = second_hop64(eye, M, NM, C, R)
    want_id = np.argmin(offer, -1)
    t64 = offer.min(-1)
    ok = np.isfinite(t64)
    tq = np.where(ok, t64, 0.0)
    P64 = M + tq[:, None] * r
    c, rad = C[want_id], R[want_id]
    N64 = (P64 - c) / rad[:, None]
    N64 *= np.where((N64 * r).sum(-1) > 0, -1.0, 1.0)[:, None]
    first = np.linalg.norm(M - eye, axis=-1)
    d1 = (M - eye) / first[:, None]

    # the tolerance, from the kernel's own arithmetic on both hops' cases
    def kat_dev(o, d, cc, rr):
        cases = np.concatenate([o, d, cc, rr[:, None]], -1)
        kat = rtow.device_kat(rtow.RT_KAT_SPHERE_HIT, cases)
        t0, t1 = roots64(o, d, cc, rr)
        good = (kat[:, 0] == 1.0) & np.isfinite(t0)
        assert good.mean() >= 0.99
        near = np.abs(kat[:, 1] - t0) <= np.abs(kat[:, 1] - t1)
        t = np.where(near, t0, t1)
        p = o + t[:, None] * d
        n = (p - cc) / rr[:, None]
        n *= np.where((n * d).sum(-1) > 0, -1.0, 1.0)[:, None]
        return max(np.abs(kat[good, 1] - t[good]).max(), np.abs(kat[good, 2:5] - p[good]).max(),
                   np.abs(kat[good, 5:8] - n[good]).max())

    dev = max(kat_dev(np.broadcast_to(eye, d1.shape), d1, np.broadcast_to(C[0], d1.shape), np.full(len(d1), R[0])),
              kat_dev(M[ok], r[ok], c[ok], rad[ok]))
    biggest = max(np.abs(C).max(), np.abs(R).max(), np.abs(eye).max(), np.abs(g["position"][one]).max())
    ulp = float(np.spacing(np.float32(biggest)))
    tol = np.maximum(8.0 * dev * (1.0 + 2.0 * tq / abs(R[0])), 4.0 * ulp)
    out = left_out64(offer, limb, tol)
    print("mirror room: %d one-bounce pixels, %d left out; KAT deviation %.3e, 4 ulp32(%.4g) = %.3e, tol %.3e .. %.3e" %
          (len(tq), int(out.sum()), dev, biggest, 4 * ulp, tol.min(), tol.max()))
    assert out.mean() <= 0.01
    k = ~out
    P, N, dep = g["position"][one].astype(f8), g["normal"][one].astype(f8), g["depth"][one].astype(f8)
    ep = np.abs(P - P64).max(-1)
    en = np.abs(N - N64).max(-1)
    ed = np.abs(dep - (first + tq))
    print("mirror room: measured deviation P %.3e, N %.3e, depth %.3e (largest ratio to its bound %.3f)" %
          (ep[k].max(), en[k].max(), ed[k].max(),
           max((ep[k] / tol[k]).max(), (ed[k] / tol[k]).max(), (en[k] / tol[k]).max())))
    assert np.array_equal(g["id"][one][k], want_id[k])
    assert np.all(ep[k] <= tol[k]) and np.all(ed[k] <= tol[k])
    assert np.all(en[k] <= tol[k])
    # N is the normal of the stored P, facing the reflected ray
    gn = (P - c) / rad[:, None]
    assert np.all(np.abs(N - gn).max(-1)[k] <= tol[k]) and np.all((N * r).sum(-1)[k] < 0)


# ---- 6. glass --------------------------------------------------------------
def test_guides_glass_sanity_on_the_five_sphere_scene(rtow, ctx):
    """Hollow glass (a negative radius inside a positive one), spp 1: every
    pixel whose chain bounced and ended on a surface has P on sphere id, a unit
    N that is +-(P - C) / R, and depth >= rt_aov's first-hit depth.  tol: the
    KAT's deviation from fp64 on the first-hit cases times 8, floored at 4
    ulp32 of the largest coordinate (test_aov_geometry_against_fp64's)."""
    w, h = FRAMES[0]
    scene = rtow.five_scene()
    ctx.upload(scene)
    cam = _camera(rtow, "five", "gpu_pinhole", w, h)
    p = rtow.make_params(w, h, 1, seed=3, flags=rtow.RT_FLAG_ACCEL_BVH)
    aov, g = ctx.aov(cam, p), ctx.guides(cam, p)
    f8 = np.float64
    C = np.stack([scene.cx, scene.cy, scene.cz], -1).astype(f8)
    R = scene.radius.astype(f8)
    eye = np.array(cam.eye[:], f8)
    hit = aov["id"] >= 0
    v = aov["position"][hit].astype(f8) - eye
    d = v / np.linalg.norm(v, axis=-1, keepdims=True)
    ids0 = aov["id"][hit]
    kat = rtow.device_kat(rtow.RT_KAT_SPHERE_HIT,
                          np.concatenate([np.broadcast_to(eye, d.shape), d, C[ids0], R[ids0][:, None]], -1))
    t0, t1 = roots64(eye, d, C[ids0], R[ids0])
    good = (kat[:, 0] == 1.0) & np.isfinite(t0)
    t = np.where(np.abs(kat[:, 1] - t0) <= np.abs(kat[:, 1] - t1), t0, t1)
    dev = max(np.abs(kat[good, 1] - t[good]).max(), np.abs(kat[good, 2:5] - (eye + t[:, None] * d)[good]).max())
    biggest = max(np.abs(C).max(), np.abs(R).max(), np.abs(eye).max(), np.abs(g["position"]).max())
    tol = max(8.0 * dev, 4.0 * float(np.spacing(np.float32(biggest))))
    m = (g["bounces"] > 0) & (g["escaped"] == 0)
    glass = scene.kind[np.maximum(aov["id"], 0)] == rtow.RT_DIELECTRIC
    assert m.sum() >= 40 and (m & glass & hit).sum() >= 20 and (g["bounces"] >= 2).any()
    ids = g["id"][m]
    assert (ids >= 0).all()
    P, N = g["position"][m].astype(f8), g["normal"][m].astype(f8)
    res = np.abs(np.linalg.norm(P - C[ids], axis=-1) - np.abs(R[ids]))
    gn = (P - C[ids]) / R[ids][:, None]
    en = np.minimum(np.abs(N - gn).max(-1), np.abs(N + gn).max(-1))
    print("five: %d chained pixels, tol %.3e; |P - C| - |R| %.3e, N vs +-(P - C) / R %.3e, ||N| - 1| %.3e" %
          (int(m.sum()), tol, res.max(), en.max(), np.abs(np.linalg.norm(N, axis=-1) - 1).max()))
    assert res.max() <= tol and en.max() <= tol
    assert np.abs(np.linalg.norm(N, axis=-1) - 1.0).max() <= tol
    assert np.all(g["depth"][m] >= aov["depth"][m])
    assert np.all(g["depth"][g["bounces"] == 0] == aov["depth"][g["bounces"] == 0])


# ---- 7. determinism --------------------------------------------------------
def test_guides_every_walk_gives_the_same_bytes(rtow, ctx):
    bvh = rtow.RT_FLAG_ACCEL_BVH
    w, h = FRAMES[0]
    scene = rtow.final_scene()
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    ctx.upload(scene)
    want = ctx.guides(cam, rtow.make_params(w, h, 5, seed=5, flags=0))  # the scan
    assert (want["bounces"] > 0).any() and (want["escaped"] > 0).any()
    got = ctx.guides(cam, rtow.make_params(w, h, 5, seed=5, flags=bvh | rtow.RT_FLAG_LAYER_BVH))
    assert _same(want, got), "layer BVH"
    for mode in ("lds", "cells", "global"):
        ctx.upload(scene, grid_mode=mode)
        assert rtow.accel_info(scene, grid_mode=mode)["grid_placement"] == rtow.GRID_PLACEMENTS[mode]
        assert _same(want, ctx.guides(cam, rtow.make_params(w, h, 5, seed=5, flags=bvh))), mode
    ctx.upload(scene, grid_mode="auto", grid_scale=0.7)  # another cell size
    assert _same(want, ctx.guides(cam, rtow.make_params(w, h, 5, seed=5, flags=bvh)))
    ctx.upload(scene, grid_mode="auto", grid_scale=0)
    a = ctx.guides(cam, rtow.make_params(w, h, 5, seed=5, flags=3), max_fuzz=0.3)
    b = ctx.guides(cam, rtow.make_params(w, h, 5, seed=5, flags=3 | bvh), max_fuzz=0.3)
    assert _same(a, b)
    five = rtow.five_scene()
    ctx.upload(five)
    cam5 = _camera(rtow, "five", "cpu_lens", w, h)
    a = ctx.guides(cam5, rtow.make_params(w, h, 5, seed=5, flags=0))
    b = ctx.guides(cam5, rtow.make_params(w, h, 5, seed=5, flags=bvh))  # the plain BVH
    assert _same(a, b) and (a["bounces"] > 0).any()


def test_guides_launch_split_and_bands_give_the_same_bytes(rtow, ctx):
    """spp 8 as 1, 2 and 8 launches (the later ones continue the stored sums);
    a subset of the buffers; three interleaved bands with padding rows."""
    w, h = FRAMES[0]
    ctx.upload(rtow.final_scene())
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    flags = rtow.RT_FLAG_ACCEL_BVH
    p = rtow.make_params(w, h, 8, seed=9, flags=flags)
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, w * h * 8)
    want = ctx.guides(cam, p)
    assert (want["bounces"] > 8).any()
    for per in (4, 1):
        ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, w * h * per)
        assert _same(want, ctx.guides(cam, p)), per
    part = ctx.guides(cam, p, which=("normal", "id", "escaped"))
    assert sorted(part) == ["escaped", "id", "kernel_ms", "normal"]
    assert all(part[n].tobytes() == want[n].tobytes() for n in ("normal", "id", "escaped"))
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    assert _same(want, ctx.guides(cam, p))
    seen = np.zeros(h, int)
    for rank in range(3):
        pb = rtow.make_params(w, h, 8, seed=9, flags=flags, rank=rank, world=3, row_block=8)
        got = ctx.guides(cam, pb)
        rows = rtow.local_to_global_rows(pb)
        inside = rows < h
        assert inside.any() and (rank < 2 or (~inside).any())
        for n in NAMES:
            assert got[n][inside].tobytes() == want[n][rows[inside]].tobytes(), (rank, n)
            assert np.all(got[n][~inside] == (-1 if n == "id" else 0)), (rank, n)
        seen[rows[inside]] += 1
    assert np.all(seen == 1)


def test_guides_between_renders_leaves_them_alone(rtow, ctx):
    scene = rtow.final_scene()
    ctx.upload(scene)
    cam = rtow.camera_cpu(aspect=64 / 36)
    p = rtow.make_params(64, 36, 5, seed=2024, flags=rtow.RT_FLAG_ACCEL_BVH)
    a, sa = ctx.render(cam, p)
    w, h = FRAMES[0]
    ctx.guides(_camera(rtow, "final", "cpu_lens", w, h), rtow.make_params(w, h, 5, seed=1, flags=rtow.RT_FLAG_ACCEL_BVH))
    ctx.guides(cam, p)
    b, sb = ctx.render(cam, p)
    want, segs = oracle_lib.kernel_render(scene, cam, p)
    assert np.array_equal(a, b) and np.array_equal(a, want)
    assert sa.segments == sb.segments == segs


def test_guides_async_into_device_pointers(rtow, ctx):
    """rt_guides_async into caller-owned device memory on a caller's stream
    gives rt_guides' bytes."""
    import torch
    w, h = FRAMES[0]
    ctx.upload(rtow.final_scene())
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    p = rtow.make_params(w, h, 5, seed=9, flags=rtow.RT_FLAG_ACCEL_BVH)
    names = ("hits", "depth", "normal", "bounces", "escaped")
    want = ctx.guides(cam, p, which=names, max_bounces=3)
    dev = torch.device("cuda:0")
    t = {n: torch.full((h, w, 3) if n == "normal" else (h, w), 7, device=dev,
                       dtype=torch.float32 if n in ("depth", "normal") else torch.int32) for n in names}
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ctx.guides_async(cam, p, {n: t[n].data_ptr() for n in names}, stream=stream.cuda_stream, max_bounces=3)
    stream.synchronize()
    for n in names:
        assert t[n].cpu().numpy().tobytes() == want[n].tobytes(), n


# ---- 8. error paths --------------------------------------------------------
def test_guides_error_paths_on_the_device(rtow):
    L = rtow.guides_lib()
    cam = rtow.camera_cpu(aspect=64 / 36)
    with rtow.Context(0) as c:
        p = rtow.make_params(64, 36, 1)
        with pytest.raises(rtow.RTError) as e:
            c.guides(cam, p)
        assert e.value.status == -6  # RT_ERR_NO_SCENE
        c.upload(rtow.five_scene())
        bufs = rtow.GuidesBuffers()  # every pointer NULL: RT_OK, nothing launched
        args = (c._h, ctypes.byref(cam), ctypes.byref(p), None, ctypes.byref(bufs))
        assert L.rt_guides(*args, None) == 0 and L.rt_guides_async(*args, None) == 0
        bad = rtow.make_params(64, 36, 1)
        bad.band_offset = 1  # >= band_stride
        assert L.rt_guides(c._h, ctypes.byref(cam), ctypes.byref(bad), None, ctypes.byref(bufs), None) == \
            rtow.RT_ERR_INVALID
        out = c.guides(cam, rtow.make_params(67, 37, 0))  # spp = 0: zeroed buffers, id = -1
        for n in NAMES:
            assert np.all(out[n] == (-1 if n == "id" else 0)), n


# ---- 9. the consumers take the buffers -------------------------------------
def _mse(sums, spp, truth, mask=None):
    x = np.clip(np.sqrt(sums.astype(np.float64) / spp), 0.0, 1.0)
    e = (x - truth) ** 2
    return float(e.mean() if mask is None else e[mask].mean())


@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_denoise_with_chain_guides(rtow, gpu_ctx, scene_name):
    """DESIGN.md 10's protocol at 128x72: 16 spp (seed 5) denoised at the
    defaults with rt_aov's guides and with rt_guides', against the product's
    4096-spp render (seed 99); MSE on sqrt(mean) clamped to [0, 1], over the
    pixels whose first hit is a dielectric or a fuzz-0 metal and over the frame.
    On the final scene's masked pixels the chain guides give the lower error:
    what the pass exists for.  Measured on the MI355X, masked: final 8.38e-4
    -> 7.31e-4; five 8.66e-4 -> 2.76e-3, where it does not hold (the hollow
    shell's samples end on several surfaces) and is printed only."""
    w, h = 128, 72
    scene = _scene(rtow, scene_name)
    view = FIVE_VIEW if scene_name == "five" else dict(focus_dist=10.0)
    cam = rtow.camera_cpu(aspect=w / h, aperture=0.1, **view)
    gpu_ctx.upload(scene)
    flags = rtow.RT_FLAG_ACCEL_BVH
    truth = gpu_ctx.render(cam, rtow.make_params(w, h, 4096, seed=99, flags=flags))[0]
    truth = np.clip(np.sqrt(truth.astype(np.float64) / 4096), 0.0, 1.0)
    p16 = rtow.make_params(w, h, 16, seed=5, flags=flags)
    noisy = gpu_ctx.render(cam, p16)[0]
    first, chain = gpu_ctx.aov(cam, p16), gpu_ctx.guides(cam, p16)
    spec = _continues(rtow, scene, 0.0)
    mask = (first["id"] >= 0) & spec[np.maximum(first["id"], 0)]
    assert mask.mean() >= 0.03
    den_first, den_chain = gpu_ctx.denoise(noisy, first, 16), gpu_ctx.denoise(noisy, chain, 16)
    e = {k: (_mse(v, 16, truth, mask), _mse(v, 16, truth)) for k, v in
         (("noisy", noisy), ("first", den_first), ("chain", den_chain))}
    hit_samples = max(int(chain["hits"].sum()), 1)
    print("guides quality %s: masked pixels %.3f of the frame; mse masked / frame: 16 spp %.4e / %.4e, "
          "first-hit guides %.4e / %.4e, chain guides %.4e / %.4e; mean bounces per hit sample %.3f" %
          (scene_name, mask.mean(), *e["noisy"], *e["first"], *e["chain"], chain["bounces"].sum() / hit_samples))
    if scene_name == "final":
        assert e["chain"][0] < e["first"][0]


def _cli(extra):
    w, h, spp, seed = 64, 36, 8, 11
    args = [os.path.join(BIN, "gpu_ray_tracer"), "--width", str(w), "--height", str(h), "--spp", str(spp),
            "--seed", str(seed), "--quiet"] + extra
    return subprocess.run(args, capture_output=True, timeout=120)


def test_cli_denoise_guides_switch(rtow, gpu_ctx):
    """gpu_ray_tracer --denoise --denoise-guides=chain writes the bytes the
    Python path gives with rt_guides at its defaults; =first writes those of
    --denoise alone; the switch is refused without --denoise, with an unknown
    value, and wherever --denoise is."""
    w, h, spp, seed = 64, 36, 8, 11
    gpu_ctx.upload(rtow.final_scene())
    cam = rtow.camera_gpu(w, h, defocus_angle=0.6, focus_dist=10.0)
    p = rtow.make_params(w, h, spp, max_depth=50, seed=seed,
                         flags=rtow.RT_FLAG_GPU_SEMANTICS | rtow.RT_FLAG_ACCEL_BVH)
    sums = gpu_ctx.render(cam, p)[0]
    first = gpu_ctx.denoise(sums, gpu_ctx.aov(cam, p), spp)
    chain = gpu_ctx.denoise(sums, gpu_ctx.guides(cam, p), spp)
    tone = lambda x: rtow.tonemap(x, spp, rtow.RT_TONEMAP_GPU)  # noqa: E731
    assert not np.array_equal(tone(first), tone(chain))
    for extra, want in ((["--denoise"], first), (["--denoise", "--denoise-guides=first"], first),
                        (["--denoise-guides=chain", "--denoise"], chain)):
        r = _cli(extra)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert np.array_equal(read_ppm_bytes(r.stdout), tone(want)), extra
    for extra in (["--denoise-guides=chain"], ["--denoise", "--denoise-guides=all"], ["--denoise", "--denoise-guides"],
                  ["--denoise", "--denoise-guides=chain", "--gpus", "2", "--devices", "0,0"]):
        r = _cli(extra)
        assert r.returncode != 0 and r.stdout == b"", extra
