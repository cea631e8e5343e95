"""First-hit feature buffers on the GPU (include/rt_aov.h, rt_aov / Context.aov):
the pass traces the render's own primary rays (exact, against depth-1 renders
of the product and of the oracle), gives one answer from every walk, grid
placement, launch split and band partition (byte equality), stays serialised
with the context's renders, and its geometry agrees with an fp64 solution
within a tolerance derived from the render kernel's own sphere arithmetic
(rt_device_kat)."""
import ctypes

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

FRAMES = ((67, 37), (64, 36))  # partial tiles on both edges and an odd width (wshift = 0); whole tiles
NAMES = ("hits", "id", "depth", "position", "normal", "albedo")
# the five-sphere scene seen from low enough to show sky (from (-2, 2, 1) at
# vfov 20, test_parity_gpu's view, every primary ray hits the ground)
FIVE_VIEW = dict(lookfrom=(-2.0, 0.5, 2.0), lookat=(0.0, 0.0, -1.0), vfov=40.0, focus_dist=3.4)


def _scene(rtow, name):
    return rtow.final_scene() if name == "final" else rtow.five_scene()


def _camera(rtow, scene_name, model, w, h):
    view = FIVE_VIEW if scene_name == "five" else dict(focus_dist=10.0)
    if model == "cpu_lens":
        return rtow.camera_cpu(aspect=w / h, aperture=0.1, **view)
    return rtow.camera_gpu(w, h, defocus_angle=0.0, **view)


def _same(a, b):
    return all(a[n].tobytes() == b[n].tobytes() for n in NAMES)


@pytest.fixture
def ctx(rtow, gpu_ctx):
    """The session's context with its options at their defaults afterwards."""
    yield gpu_ctx
    gpu_ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, 0)


# ---- a. the render's primary rays ----------------------------------------
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("model", ["cpu_lens", "gpu_pinhole"])
@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_aov_hits_are_the_renders_primary_hits(rtow, ctx, scene_name, model, flags):
    """At max_depth = 1 a render's hit sample adds exactly 0 and a miss adds
    q(sky) > 0 per channel.  So hits == spp <=> the pixel's three sums are 0,
    and at spp = 1 hits == 0 <=> the sum is > 0: for every pixel, against the
    product's render and the oracle's.  Each frame must have >= 5 % all-hit and
    >= 5 % all-miss pixels, and at spp = 5 a pixel with 0 < hits < spp."""
    scene = _scene(rtow, scene_name)
    ctx.upload(scene)
    for w, h in FRAMES:
        cam = _camera(rtow, scene_name, model, w, h)
        for spp in (1, 5):
            p = rtow.make_params(w, h, spp, max_depth=1, seed=11, flags=flags | rtow.RT_FLAG_ACCEL_BVH)
            hits = ctx.aov(cam, p, which=("hits",))["hits"]
            gpu, _ = ctx.render(cam, p)
            cpu, _ = oracle_lib.kernel_render(scene, cam, p)
            assert hits.shape == (h, w) and hits.max() <= spp
            all_hit, all_miss = hits == spp, hits == 0
            print(scene_name, model, flags, (w, h), spp, "all-hit %.3f all-miss %.3f partial %d" %
                  (all_hit.mean(), all_miss.mean(), int((~all_hit & ~all_miss).sum())))
            for img in (gpu, cpu):
                black = (img == 0).all(-1)
                assert np.array_equal(all_hit, black)
                if spp == 1:
                    assert np.array_equal(all_miss, (img > 0).all(-1))
                # a pixel with a miss among its samples is lit in every channel
                assert np.array_equal(~all_hit, (img > 0).all(-1))
            assert all_hit.mean() >= 0.05 and all_miss.mean() >= 0.05
            if spp == 5:
                assert (~all_hit & ~all_miss).any()


# ---- b. one answer from every walk ---------------------------------------
def test_aov_every_walk_gives_the_same_bytes(rtow, ctx):
    bvh = rtow.RT_FLAG_ACCEL_BVH
    w, h = FRAMES[0]
    scene = rtow.final_scene()
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    ctx.upload(scene)
    want = ctx.aov(cam, rtow.make_params(w, h, 5, seed=5, flags=0))  # the scan
    assert 0 < (want["hits"] == 5).sum() < w * h and (want["id"] >= 0).any()
    got = ctx.aov(cam, rtow.make_params(w, h, 5, seed=5, flags=bvh | rtow.RT_FLAG_LAYER_BVH))
    assert _same(want, got), "layer BVH"
    for mode in ("lds", "cells", "global"):
        ctx.upload(scene, grid_mode=mode)
        assert rtow.accel_info(scene, grid_mode=mode)["grid_placement"] == rtow.GRID_PLACEMENTS[mode]
        got = ctx.aov(cam, rtow.make_params(w, h, 5, seed=5, flags=bvh))
        assert _same(want, got), mode
    ctx.upload(scene, grid_mode="auto")
    # open interval: its own answer, again the same from scan and grid
    a = ctx.aov(cam, rtow.make_params(w, h, 5, seed=5, flags=1))
    b = ctx.aov(cam, rtow.make_params(w, h, 5, seed=5, flags=1 | bvh))
    assert _same(a, b)
    five = rtow.five_scene()
    ctx.upload(five)
    cam5 = _camera(rtow, "five", "cpu_lens", w, h)
    a = ctx.aov(cam5, rtow.make_params(w, h, 5, seed=5, flags=0))
    b = ctx.aov(cam5, rtow.make_params(w, h, 5, seed=5, flags=bvh))
    assert _same(a, b) and 0 < (a["hits"] == 5).sum() < w * h


# ---- c. launch split, bands, interleaving --------------------------------
def test_aov_launch_split_gives_the_same_bytes(rtow, ctx):
    """RT_OPT_LAUNCH_SAMPLES = 2 W H at spp 5: three launches over samples
    [0, 2), [2, 4), [4, 5), the later ones continuing the stored sums."""
    w, h = FRAMES[0]
    ctx.upload(rtow.final_scene())
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    p = rtow.make_params(w, h, 5, seed=9, flags=rtow.RT_FLAG_ACCEL_BVH)
    want = ctx.aov(cam, p)
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, w * h * 2)
    got = ctx.aov(cam, p)
    assert _same(want, got)
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 1)  # one sample per pixel and launch
    assert _same(want, ctx.aov(cam, p))
    # a subset of the buffers is the same bytes as in the full set
    part = ctx.aov(cam, p, which=("normal", "id"))
    assert sorted(part) == ["id", "kernel_ms", "normal"]
    assert part["normal"].tobytes() == want["normal"].tobytes() and np.array_equal(part["id"], want["id"])


def test_aov_band_partition_gives_the_same_bytes(rtow, ctx):
    w, h = FRAMES[0]
    ctx.upload(rtow.final_scene())
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    flags = rtow.RT_FLAG_ACCEL_BVH
    want = ctx.aov(cam, rtow.make_params(w, h, 5, seed=9, flags=flags))
    seen = np.zeros(h, int)
    for rank in range(3):
        p = rtow.make_params(w, h, 5, seed=9, flags=flags, rank=rank, world=3, row_block=8)
        got = ctx.aov(cam, p)
        rows = rtow.local_to_global_rows(p)
        inside = rows < h
        assert inside.any() and (rank < 2 or (~inside).any())  # the last rank holds padding rows
        for n in NAMES:
            assert got[n][inside].tobytes() == want[n][rows[inside]].tobytes(), (rank, n)
            pad = got[n][~inside]
            assert np.all(pad == (-1 if n == "id" else 0)), (rank, n)
        seen[rows[inside]] += 1
    assert np.all(seen == 1)


def test_aov_between_renders_leaves_them_alone(rtow, ctx):
    """The pass shares the context's serialisation and grid: a render before
    and a render after an rt_aov are bit-identical to each other and to the
    oracle (another frame size in between, so the grid is refitted)."""
    scene = rtow.final_scene()
    ctx.upload(scene)
    cam = rtow.camera_cpu(aspect=64 / 36)
    p = rtow.make_params(64, 36, 5, seed=2024, flags=rtow.RT_FLAG_ACCEL_BVH)
    a, sa = ctx.render(cam, p)
    w, h = FRAMES[0]
    ctx.aov(_camera(rtow, "final", "cpu_lens", w, h), rtow.make_params(w, h, 5, seed=1, flags=rtow.RT_FLAG_ACCEL_BVH))
    ctx.aov(cam, p)
    b, sb = ctx.render(cam, p)
    want, segs = oracle_lib.kernel_render(scene, cam, p)
    assert np.array_equal(a, b) and np.array_equal(a, want)
    assert sa.segments == sb.segments == segs


# ---- d. geometry against fp64 --------------------------------------------
def _roots64(o, d, c, r):
    """fp64 roots (t0 <= t1, NaN where the line misses) of |o + t d - c| = |r|, |d| = 1."""
    oc = o - c
    b = (oc * d).sum(-1)
    cc = (oc * oc).sum(-1) - r * r
    disc = b * b - cc
    sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
    q = -(b + np.where(b < 0, -sq, sq))  # no cancellation
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = q, np.where(q != 0, cc / q, np.nan)
    return np.minimum(ta, tb), np.maximum(ta, tb)


@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_aov_geometry_against_fp64(rtow, ctx, scene_name):
    """spp 1, a pinhole camera (every ray starts at the eye): per hit pixel the
    buffers describe one point of sphere `id` inside the pixel's footprint,
    with nothing in front of it.

    tol comes from the render kernel's present sphere arithmetic: the same
    (eye, normalised P - eye, C, r) cases through rt_device_kat(RT_KAT_SPHERE_HIT),
    its largest deviation of t, P, N from the fp64 solution over the frame,
    times 8 (2x: the reconstructed direction carries one more rounding; 4x:
    the KAT has no form selection of refine_root's for the r = 1000 ground),
    floored at 4 ulp32 of the largest coordinate magnitude involved.  The
    occlusion check uses the same tolerance in relative form, eps = tol / t."""
    w, h = FRAMES[0]
    scene = _scene(rtow, scene_name)
    ctx.upload(scene)
    cam = _camera(rtow, scene_name, "gpu_pinhole", w, h)
    p = rtow.make_params(w, h, 1, seed=3, flags=rtow.RT_FLAG_ACCEL_BVH)
    out = ctx.aov(cam, p)
    hit = out["id"] >= 0
    assert np.array_equal(hit, out["hits"] == 1) and 0.05 <= hit.mean() <= 0.95
    rows, cols = np.nonzero(hit)
    ids = out["id"][hit]
    f8 = np.float64
    eye = np.array(cam.eye[:], f8)
    C = np.stack([scene.cx, scene.cy, scene.cz], -1).astype(f8)
    R = scene.radius.astype(f8)
    P, N, t = out["position"][hit].astype(f8), out["normal"][hit].astype(f8), out["depth"][hit].astype(f8)
    c, r = C[ids], R[ids]
    v = P - eye
    dist = np.linalg.norm(v, axis=-1)
    d = v / dist[:, None]

    # the tolerance, from the kernel's own arithmetic on the same cases
    cases = np.concatenate([np.broadcast_to(eye, d.shape), d, c, r[:, None]], -1)
    kat = rtow.device_kat(rtow.RT_KAT_SPHERE_HIT, cases)
    t0, t1 = _roots64(eye, d, c, r)
    # (a line through a point an ulp outside the sphere at its very limb may miss it)
    ok = (kat[:, 0] == 1.0) & np.isfinite(t0)
    assert ok.mean() >= 0.99
    near = np.abs(kat[:, 1] - t0) <= np.abs(kat[:, 1] - t1)
    t64 = np.where(near, t0, t1)
    p64 = eye + t64[:, None] * d
    n64 = (p64 - c) / r[:, None]
    n64 *= np.where((n64 * d).sum(-1) > 0, -1.0, 1.0)[:, None]  # set_face_normal
    dev = max(np.abs(kat[ok, 1] - t64[ok]).max(), np.abs(kat[ok, 2:5] - p64[ok]).max(),
              np.abs(kat[ok, 5:8] - n64[ok]).max())
    biggest = max(np.abs(C[np.unique(ids)]).max(), np.abs(R[np.unique(ids)]).max(), np.abs(eye).max(), np.abs(P).max())
    ulp = float(np.spacing(np.float32(biggest)))
    tol = max(8.0 * dev, 4.0 * ulp)
    print("%s: KAT deviation from fp64 %.3e, 4 ulp32(%.4g) = %.3e, tol = %.3e" % (scene_name, dev, biggest, 4 * ulp, tol))

    # albedo: the hit sphere's shading albedo, exactly
    want_alb = np.where((scene.kind[ids] == rtow.RT_DIELECTRIC)[:, None], np.float32(1.0), scene.albedo[ids])
    assert np.array_equal(out["albedo"][hit], want_alb.astype(np.float32))
    assert np.all(out["albedo"][~hit] == 0) and np.all(out["depth"][~hit] == 0)
    assert np.all(out["position"][~hit] == 0) and np.all(out["normal"][~hit] == 0)
    # depth, the point on the sphere, the normal
    assert np.abs(t - dist).max() <= tol
    assert np.abs(np.linalg.norm(P - c, axis=-1) - np.abs(r)).max() <= tol
    g = (P - c) / r[:, None]
    assert np.minimum(np.abs(N - g).max(-1), np.abs(N + g).max(-1)).max() <= tol
    assert np.all((N * v).sum(-1) < 0)
    # the direction lies in the pixel's footprint: P - eye = lam (corner - eye + fs horiz + ft vert)
    hz, vt = np.array(cam.horiz[:], f8), np.array(cam.vert[:], f8)
    basis = np.stack([np.array(cam.corner[:], f8) - eye, hz, vt], -1)
    x = np.linalg.solve(basis, v.T).T
    lam, fs, ft = x[:, 0], x[:, 1] / x[:, 0], x[:, 2] / x[:, 0]
    assert np.all(lam > 0)
    tol_s, tol_t = tol / (lam * np.linalg.norm(hz)), tol / (lam * np.linalg.norm(vt))  # tol in pixels at P
    assert np.all(np.abs(fs - cols) <= 0.5 + tol_s) and np.all(np.abs(ft - rows) <= 0.5 + tol_t)
    # nothing in front: over all spheres, the root each offers (the entering
    # one if past t_min, else the exiting one) is not before t (1 - eps)
    tmin = 0.001 * dist / lam  # 0.001 |unnormalised direction|
    a0, a1 = _roots64(eye[None, None, :], d[:, None, :], C[None, :, :], R[None, :])
    with np.errstate(invalid="ignore"):
        offer = np.where(a0 > tmin[:, None], a0, a1)
        offer = np.where(np.isnan(offer) | (offer <= tmin[:, None]), np.inf, offer)
    srt = np.sort(offer, axis=-1)
    assert np.all(np.isfinite(srt[:, 0]))
    eps = tol / dist
    ambiguous = (srt[:, 1] - srt[:, 0]) < eps * srt[:, 0]
    print("%s: %d hit pixels, %d with two roots within eps left out" % (scene_name, len(ids), int(ambiguous.sum())))
    assert ambiguous.mean() <= 0.01
    clear = ~ambiguous
    assert np.all(srt[clear, 0] >= dist[clear] * (1 - eps[clear]))
    assert np.array_equal(np.argmin(offer, axis=-1)[clear], ids[clear])


# ---- e. error paths -------------------------------------------------------
def test_aov_error_paths_on_the_device(rtow):
    L = rtow.aov_lib()
    cam = rtow.camera_cpu(aspect=64 / 36)
    with rtow.Context(0) as c:
        p = rtow.make_params(64, 36, 1)
        with pytest.raises(rtow.RTError) as e:
            c.aov(cam, p)
        assert e.value.status == -6  # RT_ERR_NO_SCENE
        c.upload(rtow.five_scene())
        # every pointer NULL: RT_OK, nothing launched
        bufs = rtow.AovBuffers()
        assert L.rt_aov(c._h, ctypes.byref(cam), ctypes.byref(p), ctypes.byref(bufs), None) == 0
        assert L.rt_aov_async(c._h, ctypes.byref(cam), ctypes.byref(p), ctypes.byref(bufs), None) == 0
        bad = rtow.make_params(64, 36, 1)
        bad.band_offset = 1  # >= band_stride
        assert L.rt_aov(c._h, ctypes.byref(cam), ctypes.byref(bad), ctypes.byref(bufs), None) == rtow.RT_ERR_INVALID
        # spp = 0: zeroed buffers, id = -1
        out = c.aov(cam, rtow.make_params(67, 37, 0))
        for n in NAMES:
            assert np.all(out[n] == (-1 if n == "id" else 0)), n


def test_aov_async_into_device_pointers(rtow, ctx):
    """rt_aov_async into caller-owned device memory on a caller's stream gives
    rt_aov's bytes."""
    import torch
    w, h = FRAMES[0]
    ctx.upload(rtow.final_scene())
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    p = rtow.make_params(w, h, 5, seed=9, flags=rtow.RT_FLAG_ACCEL_BVH)
    want = ctx.aov(cam, p, which=("hits", "depth", "normal"))
    dev = torch.device("cuda:0")
    hits = torch.full((h, w), 77, dtype=torch.int32, device=dev)
    depth = torch.full((h, w), 7.0, dtype=torch.float32, device=dev)
    normal = torch.full((h, w, 3), 7.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ctx.aov_async(cam, p, {"hits": hits.data_ptr(), "depth": depth.data_ptr(), "normal": normal.data_ptr()},
                  stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(hits.cpu().numpy().astype(np.uint32), want["hits"])
    assert depth.cpu().numpy().tobytes() == want["depth"].tobytes()
    assert normal.cpu().numpy().tobytes() == want["normal"].tobytes()
