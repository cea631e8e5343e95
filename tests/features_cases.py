"""The case list of the bit-for-bit checks of rt_aov, rt_guides and rt_route
against the chain oracle (test infrastructure): shared by
test_features_oracle_gpu.py, which runs the passes on it, and
test_features_oracle.py, which shows on the CPU that the list meets every
situation the checks are there for (the coverage conditions).  The oracle's
records are computed once per (case, frame, max_bounces, max_fuzz, keep_dir)
and shared by the passes' tests of that case; they are dropped when another
case asks."""
import numpy as np

import fixture_scenes
import oracle_lib
import random_scenes
from mirror_room import mirror_room

FRAMES = ((67, 37), (5, 3), (1, 1))
FIVE_VIEW = dict(lookfrom=(-2.0, 0.5, 2.0), lookat=(0.0, 0.0, -1.0), vfov=40.0, focus_dist=3.4)
MIRROR_VIEW = dict(lookfrom=(0.0, 0.5, 6.0), lookat=(0.0, 0.0, 0.0), vfov=40.0, focus_dist=6.0)
CLAMP_VIEW = dict(lookfrom=(0.0, 0.0, 3.0), lookat=(0.0, 0.0, 0.0), vfov=60.0, focus_dist=3.0)
CLAMP_ALBEDO = 3.0
DEFAULT_BOUNCES = 8                     # rt_guides_options / rt_route_options max_bounces = 0
GUIDES_BOUNCES = (-1, 1, 2, DEFAULT_BOUNCES, 64)
GUIDES_FUZZ = (0.0, 0.3, 1.0)
ROUTE_BOUNCES = (DEFAULT_BOUNCES, 2)


def _spheres(rtow, rows):
    """A Scene of rows (cx, cy, cz, radius, kind, albedo rgb, param)."""
    f32 = np.float32
    geom = np.array([r[:4] for r in rows], np.float64).astype(f32)
    return rtow.Scene(geom[:, 0].copy(), geom[:, 1].copy(), geom[:, 2].copy(), geom[:, 3].copy(),
                      np.array([r[4] for r in rows], np.uint32), np.array([r[5] for r in rows], f32),
                      np.array([r[6] for r in rows], f32))


def clamp_scene(rtow):
    """Synthetic, for the 2^100 throughput clamp: two mirrors (fuzz-0 metals)
    of albedo 3.0 facing each other -- a hollow one of radius 8 around the
    camera and a ball of radius 1 at its centre -- and a small lambertian ball.
    A chain of at most 64 bounces has at most 65 counted hits, and 2.9^65 <
    2^100: with albedos up to 2.9 the clamp is unreachable within 64 bounces.
    3.0^64 > 2^100 reaches it at the 64th hit of a chain between the mirrors.
    Such an albedo is for this scene only."""
    a = CLAMP_ALBEDO
    rows = [(0.0, 0.0, 0.0, 8.0, 1, (a, a, a), 0.0), (0.0, 0.0, 0.0, 1.0, 1, (a, a, a), 0.0),
            (2.5, 0.5, 0.0, 0.5, 0, (0.6, 0.5, 0.4), 0.0)]
    return _spheres(rtow, rows)


def glass_ground_scene(rtow):
    """Synthetic, for the spurious-root rule inside a chain: the r = 1000 ground
    made of glass under a lambertian, a glass and a mirror ball, all inside a
    lambertian dome of radius 3000.  A ray that leaves the ground's surface
    (reflected off it, or refracted into it) starts on a sphere whose expanded
    fp32 quadratic is noisy at that size, so both arms of the rule occur a few
    hundred times per frame; the dome gives every such ray a counted hit after
    the skip, so that the distance a first-arm skip walked enters a depth."""
    rows = [(0.0, -1000.0, 0.0, 1000.0, 2, (1.0, 1.0, 1.0), 1.5), (0.0, 1.0, 0.0, 1.0, 0, (0.7, 0.6, 0.5), 0.0),
            (2.0, 0.5, 2.0, 0.5, 2, (1.0, 1.0, 1.0), 1.5), (3.0, 0.4, -1.5, 0.4, 1, (0.9, 0.9, 0.9), 0.0),
            (0.0, 0.0, 0.0, 3000.0, 0, (0.5, 0.6, 0.8), 0.0)]
    return _spheres(rtow, rows)


SCENES = {
    "final": lambda rtow: rtow.final_scene(),
    "five": lambda rtow: rtow.five_scene(),
    "mirror": mirror_room,
    "embed": fixture_scenes.embedded_glass_scene,
    "negop": fixture_scenes.negative_opaque_scene,
    "hot": fixture_scenes.hot_scene,
    "contact": fixture_scenes.contact_scene,
    "clamp": clamp_scene,
    "glassground": glass_ground_scene,
    "free3": lambda rtow: random_scenes.free_scene(rtow, 3),
    "free12": lambda rtow: random_scenes.free_scene(rtow, 12),
}
VIEWS = {"five": FIVE_VIEW, "mirror": MIRROR_VIEW, "clamp": CLAMP_VIEW}

# name: scene, camera model, flags (RT_FLAG_GPU_SEMANTICS or 0), spp, seed, and
#   walk:   "bvh" = RT_FLAG_ACCEL_BVH (the layer grid on the final scene: the default walk), "scan" = without it
#   frames: FRAMES unless given (1x1 is skipped for the lens camera, which needs two pixels each way)
#   bands:  (world, rank, row_block) of a banded case
#   launch: samples per pixel and launch of a case that sets RT_OPT_LAUNCH_SAMPLES
_BIG = (FRAMES[0],)
CASES = {
    "final-lens": dict(scene="final", model="cpu_lens", flags=0, spp=5, seed=11),
    "final-pinhole-gpusem": dict(scene="final", model="gpu_pinhole", flags=3, spp=16, seed=12),
    "final-scan": dict(scene="final", model="cpu_lens", flags=3, spp=5, seed=13, walk="scan", frames=_BIG),
    "final-spp0": dict(scene="final", model="cpu_lens", flags=0, spp=0, seed=14, frames=_BIG),
    "final-bands": dict(scene="final", model="cpu_lens", flags=0, spp=5, seed=15, frames=_BIG, bands=(2, 1, 8)),
    "five-pinhole": dict(scene="five", model="gpu_pinhole", flags=0, spp=16, seed=21),
    "five-lens-gpusem": dict(scene="five", model="cpu_lens", flags=3, spp=5, seed=22),
    "five-spp1": dict(scene="five", model="gpu_pinhole", flags=3, spp=1, seed=23),
    "five-launches": dict(scene="five", model="cpu_lens", flags=0, spp=16, seed=24, frames=_BIG, launch=4),
    "mirror": dict(scene="mirror", model="gpu_pinhole", flags=0, spp=1, seed=3),
    "mirror-lens-gpusem": dict(scene="mirror", model="cpu_lens", flags=3, spp=5, seed=31, frames=_BIG),
    "embed-lens": dict(scene="embed", model="cpu_lens", flags=0, spp=5, seed=41, frames=_BIG),
    "embed-pinhole-gpusem": dict(scene="embed", model="gpu_pinhole", flags=3, spp=16, seed=42, frames=_BIG),
    "negop": dict(scene="negop", model="cpu_lens", flags=3, spp=5, seed=51, frames=_BIG),
    "hot": dict(scene="hot", model="cpu_lens", flags=0, spp=5, seed=61, frames=_BIG),
    "hot-gpusem": dict(scene="hot", model="gpu_pinhole", flags=3, spp=16, seed=62, frames=_BIG),
    "contact": dict(scene="contact", model="cpu_lens", flags=0, spp=16, seed=71, frames=_BIG),
    "contact-gpusem": dict(scene="contact", model="gpu_pinhole", flags=3, spp=5, seed=72, frames=_BIG),
    "clamp": dict(scene="clamp", model="gpu_pinhole", flags=0, spp=5, seed=81, frames=_BIG),
    "glassground": dict(scene="glassground", model="cpu_lens", flags=0, spp=5, seed=7, frames=_BIG),
    "glassground-gpusem": dict(scene="glassground", model="gpu_pinhole", flags=3, spp=16, seed=8, frames=_BIG),
    "free3": dict(scene="free3", model="cpu_lens", flags=0, spp=5, seed=91, frames=_BIG),
    "free12-gpusem": dict(scene="free12", model="gpu_pinhole", flags=3, spp=16, seed=92, frames=_BIG),
}

_SCENES, _TERMS = {}, {}  # _TERMS holds one case's records at a time


def scene_of(rtow, case):
    name = CASES[case]["scene"]
    if name not in _SCENES:
        _SCENES[name] = SCENES[name](rtow)
    return _SCENES[name]


def frames_of(case):
    c = CASES[case]
    return [f for f in c.get("frames", FRAMES) if not (c["model"] == "cpu_lens" and min(f) < 2)]


def camera_of(rtow, case, frame):
    c = CASES[case]
    w, h = frame
    view = VIEWS.get(c["scene"], dict(focus_dist=10.0))
    if c["model"] == "cpu_lens":
        return rtow.camera_cpu(aspect=w / h, aperture=0.1, **view)
    return rtow.camera_gpu(w, h, defocus_angle=0.0, **view)


def params_of(rtow, case, frame):
    c = CASES[case]
    w, h = frame
    world, rank, row_block = c.get("bands", (1, 0, 8))
    flags = c["flags"] | (0 if c.get("walk") == "scan" else rtow.RT_FLAG_ACCEL_BVH)
    return rtow.make_params(w, h, c["spp"], seed=c["seed"], flags=flags, rank=rank, world=world, row_block=row_block)


def terminals(rtow, case, frame, max_bounces, max_fuzz=0.0, keep_dir=False):
    """The oracle's records of a case, computed once and shared, read-only, by
    the tests of that case (which run next to each other, parametrised by case
    or looping over the cases); another case's records are dropped first."""
    if _TERMS and next(iter(_TERMS))[0] != case:
        _TERMS.clear()
    key = (case, frame, int(max_bounces), float(np.float32(max_fuzz)), bool(keep_dir))
    if key not in _TERMS:
        t = oracle_lib.kernel_terminals(scene_of(rtow, case), camera_of(rtow, case, frame),
                                        params_of(rtow, case, frame), max_bounces, max_fuzz, keep_dir)
        t.setflags(write=False)
        _TERMS[key] = t
    return _TERMS[key]
