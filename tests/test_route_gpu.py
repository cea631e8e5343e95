"""Guide buffers of each pixel's dominant specular route, on the GPU
(include/rt_route.h, rt_route / Context.route): with nothing followed the pass
is rt_aov, where nothing can be followed it is rt_guides, byte for byte; the
vote is the restatement's (tests/route_ref.py) on every sample's route as
rt_guides' prefix differences give it, exactly; the sums are those samples'
features within a rounding bound; finalize is the restatement's, bit for bit;
one answer from every walk, placement, launch split and band partition; and the
denoiser takes the buffers as they are."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import route_ref
from oracle_lib import read_ppm_bytes
from test_guides_gpu import (AOV, FIVE_VIEW, FRAMES, _camera, _cli, _continues, _copy, _mse, _scene, mirror_room,
                             mirror_room_camera)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = AOV + ("route", "matched")
ALL = NAMES + ("state",)
FEATURES = ("depth", "position", "normal", "albedo")
SPP = 16


def _same(a, b, names=NAMES):
    return all(a[n].tobytes() == b[n].tobytes() for n in names)


@pytest.fixture
def ctx(rtow, gpu_ctx):
    """The session's context with its options at their defaults afterwards."""
    yield gpu_ctx
    gpu_ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_SCALE, 0)


# ---- 1. equality with the existing passes ----------------------------------
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("model", ["cpu_lens", "gpu_pinhole"])
@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_route_without_bounces_is_rt_aov(rtow, ctx, scene_name, model, flags):
    """max_bounces = 0 (the struct's -1): every key is 1, so the six shared
    buffers are rt_aov's byte for byte, route = 0 on every hit pixel and
    matched = hits.  At max_bounces 0, 1, 2 and 8, hits is rt_aov's hits."""
    ctx.upload(_scene(rtow, scene_name))
    for w, h in FRAMES:
        cam = _camera(rtow, scene_name, model, w, h)
        p = rtow.make_params(w, h, 5, seed=11, flags=flags | rtow.RT_FLAG_ACCEL_BVH)
        if model == "cpu_lens" and min(w, h) < 2:  # that camera model needs two pixels each way: rt_aov's check
            with pytest.raises(rtow.RTError) as e:
                ctx.route(cam, p)
            assert e.value.status == rtow.RT_ERR_INVALID
            continue
        want = ctx.aov(cam, p)
        got = ctx.route(cam, p, max_bounces=0)
        assert sorted(got) == sorted(NAMES + ("kernel_ms",))
        assert _same(want, got, AOV), (w, h)
        assert np.array_equal(got["matched"], got["hits"])
        assert np.array_equal(got["route"], np.where(got["hits"] > 0, 0, rtow.ROUTE_NO_HIT).astype(np.uint32))
        for mb in (1, 2, 8):
            g = ctx.route(cam, p, which=("hits", "matched"), max_bounces=mb)
            assert g["hits"].tobytes() == want["hits"].tobytes(), (w, h, mb)
            assert np.all(g["matched"] <= g["hits"]) and np.all((g["matched"] > 0) == (g["hits"] > 0))


def test_route_of_a_rough_scene_is_rt_guides(rtow, ctx):
    """test_guides_of_a_rough_scene_are_rt_aov's scene: at the defaults nothing
    continues a chain, every sample's key is 1: rt_guides' bytes, matched ==
    hits everywhere."""
    s = rtow.final_scene()
    diel = s.kind == rtow.RT_DIELECTRIC
    kind = np.where(diel, rtow.RT_LAMBERTIAN, s.kind).astype(np.uint32)
    param = np.where(diel, 0.0, np.where(s.kind == rtow.RT_METAL, np.maximum(s.param, 0.1), s.param)).astype(np.float32)
    rough = _copy(rtow, s, kind=kind, param=param)
    assert not _continues(rtow, rough, 0.0).any()
    ctx.upload(rough)
    w, h = FRAMES[0]
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    p = rtow.make_params(w, h, 5, seed=4, flags=rtow.RT_FLAG_ACCEL_BVH)
    want, got = ctx.guides(cam, p), ctx.route(cam, p)
    assert _same(want, got, AOV) and (want["hits"] > 0).any()
    assert np.array_equal(got["matched"], got["hits"])
    assert np.all(got["route"][got["hits"] > 0] == 0)


# ---- 2. the selection and the sums -----------------------------------------
_PREFIX = {}


def _prefix(rtow, ctx, scene_name):
    """rt_guides at spp = 1 .. 16 (one seed, 67x37) and rt_route at 16 spp with
    its state; computed once per scene and shared, unchanged, by the tests
    below.  The integer prefix differences of hits, bounces and escaped give
    every sample's hit, b_s and e_s."""
    if scene_name not in _PREFIX:
        w, h = FRAMES[0]
        if scene_name == "mirror":
            ctx.upload(mirror_room(rtow))
            cam = mirror_room_camera(rtow, w, h)
        else:
            ctx.upload(_scene(rtow, scene_name))
            cam = _camera(rtow, scene_name, "cpu_lens", w, h)
        params = [rtow.make_params(w, h, k, seed=7, flags=rtow.RT_FLAG_ACCEL_BVH) for k in range(SPP + 1)]
        g = [ctx.guides(cam, q) for q in params]
        assert not g[0]["hits"].any()
        route = ctx.route(cam, params[SPP], which=ALL)
        i64 = {n: np.stack([x[n].astype(np.int64) for x in g]) for n in ("hits", "bounces", "escaped")}
        hit, b, e = (np.diff(i64[n], axis=0) for n in ("hits", "bounces", "escaped"))
        assert set(np.unique(hit)) <= {0, 1} and set(np.unique(e)) <= {0, 1} and b.min() >= 0 and b.max() <= 8
        assert not (b[hit == 0].any() or e[hit == 0].any())
        sel = route_ref.select(route_ref.route_key(b, e), hit == 1)
        _PREFIX[scene_name] = dict(g=g, route=route, hit=hit == 1, b=b, e=e, sel=sel)
    return _PREFIX[scene_name]


@pytest.mark.parametrize("scene_name", ["five", "mirror", "final"])
def test_route_selection_is_the_restatements(rtow, ctx, scene_name):
    """route_ref.select on every sample's (hit, b_s, e_s) equals the state's
    (key, votes, n, hits) and the route / matched outputs, as integers.
    Wherever the adoption index is the first hit sample and n == hits (the
    candidate never changed and every hit sample matched), and where nothing
    hit, the six shared buffers are rt_guides' bytes."""
    d = _prefix(rtow, ctx, scene_name)
    sel, route, full = d["sel"], d["route"], d["g"][SPP]
    st = route_ref.split_state(route["state"])
    for n in ("key", "votes", "n", "hits"):
        assert np.array_equal(st[n], sel[n]), n
    assert not st["pad"].any()
    assert np.array_equal(route["matched"], sel["n"]) and np.array_equal(route["hits"], full["hits"])
    assert np.array_equal(route["route"], sel["key"] - np.uint32(1))
    assert np.array_equal(route["id"], full["id"]) and np.array_equal(st["id"], full["id"])
    hits = sel["hits"]
    first_hit = np.where(hits > 0, np.argmax(d["hit"], axis=0), -1)
    plain = (sel["adopted"] == first_hit) & (sel["n"] == hits)
    assert plain[hits == 0].all() and (plain & (hits > 0)).any()
    for n in AOV:
        assert route[n][plain].tobytes() == full[n][plain].tobytes(), n


@pytest.mark.parametrize("scene_name", ["five", "mirror", "final"])
def test_route_sums_and_finalize(rtow, ctx, scene_name):
    """Sample s's features x_s, reconstructed in fp64 from rt_guides' float
    prefix differences (each carries at most 1/2 ulp32 of its prefix sum),
    summed over the restated matched set, against the state's raw sums: per
    component within 2 spp ulp32(sum_s |x_s|) -- one rounding per add on each
    side, each at most 1/2 ulp32 of a partial sum that sum_s |x_s| bounds.
    finalize(state) equals the eight outputs bit for bit."""
    d = _prefix(rtow, ctx, scene_name)
    st = route_ref.split_state(d["route"]["state"])
    member = d["sel"]["member"]
    worst = 0.0
    for n in FEATURES:
        pre = np.stack([x[n].astype(np.float64) for x in d["g"]])
        x = np.diff(pre, axis=0)
        m, hit = (member, d["hit"]) if x.ndim == 3 else (member[..., None], d["hit"][..., None])
        assert not x[~np.broadcast_to(hit, x.shape)].any()  # a miss adds nothing
        want = (x * m).sum(0)
        bound = 2.0 * SPP * np.spacing(np.abs(x).sum(0).astype(np.float32)).astype(np.float64)
        err = np.abs(st[n].astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (n, float((err / bound).max()))
    print("route sums %s: largest |state - restated| / bound %.4f" % (scene_name, worst))
    fin = route_ref.finalize(d["route"]["state"])
    for n in NAMES:
        assert fin[n].dtype == d["route"][n].dtype and fin[n].tobytes() == d["route"][n].tobytes(), n
    part = d["route"]["matched"] < d["route"]["hits"]
    assert scene_name == "mirror" or part.any()


def test_route_census_of_the_five_sphere_frame(rtow, ctx):
    """The five-sphere frame of the tests above (67x37, 16 spp, seed 7, lens
    camera) contains every class the pass distinguishes."""
    d = _prefix(rtow, ctx, "five")
    r, sel = d["route"], d["sel"]
    hit = r["hits"] > 0
    census = {"matched == hits": int((hit & (r["matched"] == r["hits"])).sum()),
              "matched < hits": int((r["matched"] < r["hits"]).sum()),
              "candidate changed": int((sel["changes"] > 0).sum()),
              "route escaped": int((hit & ((r["route"] & 1) == 1)).sum()),
              "route with bounces": int((hit & (r["route"] >> 1 > 0)).sum())}
    print("route census five 67x37: %d hit pixels; %s" % (int(hit.sum()), census))
    assert all(v > 0 for v in census.values()), census


# ---- 3. invariance ----------------------------------------------------------
def test_route_every_walk_gives_the_same_bytes(rtow, ctx):
    bvh = rtow.RT_FLAG_ACCEL_BVH
    w, h = FRAMES[0]
    scene = rtow.final_scene()
    cam = _camera(rtow, "final", "cpu_lens", w, h)
    ctx.upload(scene)
    want = ctx.route(cam, rtow.make_params(w, h, 5, seed=5, flags=0), which=ALL)  # the scan
    assert (want["route"][want["hits"] > 0] > 0).any() and (want["matched"] < want["hits"]).any()
    got = ctx.route(cam, rtow.make_params(w, h, 5, seed=5, flags=bvh | rtow.RT_FLAG_LAYER_BVH), which=ALL)
    assert _same(want, got, ALL), "layer BVH"
    for mode in ("lds", "cells", "global"):
        ctx.upload(scene, grid_mode=mode)
        assert rtow.accel_info(scene, grid_mode=mode)["grid_placement"] == rtow.GRID_PLACEMENTS[mode]
        assert _same(want, ctx.route(cam, rtow.make_params(w, h, 5, seed=5, flags=bvh), which=ALL), ALL), mode
    ctx.upload(scene, grid_mode="auto", grid_scale=0.7)  # another cell size
    assert _same(want, ctx.route(cam, rtow.make_params(w, h, 5, seed=5, flags=bvh), which=ALL), ALL)
    ctx.upload(scene, grid_mode="auto", grid_scale=0)
    five = rtow.five_scene()
    ctx.upload(five)
    cam5 = _camera(rtow, "five", "cpu_lens", w, h)
    a = ctx.route(cam5, rtow.make_params(w, h, 5, seed=5, flags=3), which=ALL)
    b = ctx.route(cam5, rtow.make_params(w, h, 5, seed=5, flags=3 | bvh), which=ALL)  # the plain BVH
    assert _same(a, b, ALL) and (a["matched"] < a["hits"]).any()


def test_route_launch_split_and_bands_give_the_same_bytes(rtow, ctx):
    """16 spp as one, three (6 + 6 + 4) and sixteen launches (the later ones
    continue the stored state); a subset of the buffers; three interleaved
    bands with padding rows."""
    w, h = FRAMES[0]
    ctx.upload(rtow.five_scene())
    cam = _camera(rtow, "five", "cpu_lens", w, h)
    flags = rtow.RT_FLAG_ACCEL_BVH
    p = rtow.make_params(w, h, SPP, seed=9, flags=flags)
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, w * h * SPP)
    want = ctx.route(cam, p, which=ALL)
    assert (want["matched"] < want["hits"]).any()
    for per in (6, 1):
        ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, w * h * per)
        assert _same(want, ctx.route(cam, p, which=ALL), ALL), per
    part = ctx.route(cam, p, which=("normal", "route"))
    assert sorted(part) == ["kernel_ms", "normal", "route"]
    assert all(part[n].tobytes() == want[n].tobytes() for n in ("normal", "route"))
    only_state = ctx.route(cam, p, which=("state",))
    assert only_state["state"].tobytes() == want["state"].tobytes()
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    assert _same(want, ctx.route(cam, p, which=ALL), ALL)
    initial = route_ref.make_state(0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, -1)
    seen = np.zeros(h, int)
    for rank in range(3):
        pb = rtow.make_params(w, h, SPP, seed=9, flags=flags, rank=rank, world=3, row_block=8)
        got = ctx.route(cam, pb, which=ALL)
        rows = rtow.local_to_global_rows(pb)
        inside = rows < h
        assert inside.any() and (rank < 2 or (~inside).any())
        for n in NAMES:
            assert got[n][inside].tobytes() == want[n][rows[inside]].tobytes(), (rank, n)
            pad = {"id": -1, "route": rtow.ROUTE_NO_HIT}.get(n, 0)
            assert np.all(got[n][~inside] == pad), (rank, n)
        assert got["state"][:, inside].tobytes() == want["state"][:, rows[inside]].tobytes(), rank
        assert np.all(got["state"][:, ~inside] == initial[:, None, None, :]), rank
        seen[rows[inside]] += 1
    assert np.all(seen == 1)


# ---- 4. behaviour around other work -----------------------------------------
_THREE_LIBRARIES_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import rtow
rtow.aov_lib(), rtow.guides_lib(), rtow.route_lib()  # all loaded before any pass runs
AOV = ("hits", "id", "depth", "position", "normal", "albedo")
view = dict(lookfrom=(-2.0, 0.5, 2.0), lookat=(0.0, 0.0, -1.0), vfov=40.0, focus_dist=3.4)
p = rtow.make_params(16, 16, 2, seed=11, flags=rtow.RT_FLAG_ACCEL_BVH)
lens, pinhole = (rtow.camera_cpu(aspect=1.0, aperture=a, **view) for a in (0.1, 0.0))
with rtow.Context(0) as ctx:
    ctx.upload(rtow.five_scene())
    calls = {"aov": ctx.aov, "guides": lambda cam, p: ctx.guides(cam, p, max_bounces=0),
             "route": lambda cam, p: ctx.route(cam, p, max_bounces=0)}
    got = {name: calls[name](lens, p) for name in sys.argv[2:]}  # in the order under test
    for n in AOV:
        assert got["aov"][n].tobytes() == got["guides"][n].tobytes() == got["route"][n].tobytes(), n
    for name in got:
        sharp = calls[name](pinhole, p)
        assert (got[name]["hits"] > 0).any()
        assert got[name]["position"].tobytes() != sharp["position"].tobytes(), name
print("ok")
"""


@pytest.mark.parametrize("order", list(itertools.permutations(("route", "guides", "aov"))))
def test_three_libraries_in_one_process_upload_their_own_lens_table(order):
    """test_both_libraries_in_one_process_upload_their_own_lens_table's method
    with librtow_route.so as the third holder of a lens table of its own: a
    fresh process per first-call order, all three loaded, a lens camera; with
    nothing followed the three passes give the same bytes, and each one's
    positions differ from the same call with aperture 0."""
    pkg = os.path.join(ROOT, "ray-tracing-in-one-weekend_amd")
    r = subprocess.run([sys.executable, "-c", _THREE_LIBRARIES_CHILD, pkg, *order], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_route_between_renders_leaves_them_alone(rtow, ctx):
    scene = rtow.final_scene()
    ctx.upload(scene)
    cam = rtow.camera_cpu(aspect=64 / 36)
    p = rtow.make_params(64, 36, 5, seed=2024, flags=rtow.RT_FLAG_ACCEL_BVH)
    a, sa = ctx.render(cam, p)
    w, h = FRAMES[0]
    ctx.route(_camera(rtow, "final", "cpu_lens", w, h), rtow.make_params(w, h, 5, seed=1, flags=rtow.RT_FLAG_ACCEL_BVH))
    ctx.route(cam, p)
    b, sb = ctx.render(cam, p)
    want, segs = oracle_lib.kernel_render(scene, cam, p)
    assert np.array_equal(a, b) and np.array_equal(a, want)
    assert sa.segments == sb.segments == segs


def test_route_async_into_device_pointers(rtow, ctx):
    """rt_route_async into caller-owned device memory and state on a caller's
    stream gives rt_route's bytes, state included."""
    import torch
    w, h = FRAMES[0]
    ctx.upload(rtow.five_scene())
    cam = _camera(rtow, "five", "cpu_lens", w, h)
    p = rtow.make_params(w, h, 5, seed=9, flags=rtow.RT_FLAG_ACCEL_BVH)
    names = ("hits", "depth", "normal", "route", "matched")
    want = ctx.route(cam, p, which=names + ("state",), max_bounces=3)
    dev = torch.device("cuda:0")
    t = {n: torch.full((h, w, 3) if n == "normal" else (h, w), 7, device=dev,
                       dtype=torch.float32 if n in ("depth", "normal") else torch.int32) for n in names}
    nbytes = rtow.route_lib().rt_route_state_bytes(w, h)
    assert nbytes == 64 * w * h
    state = torch.full((nbytes // 4,), 7, device=dev, dtype=torch.int32)
    assert state.data_ptr() % 16 == 0
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ctx.route_async(cam, p, {n: t[n].data_ptr() for n in names}, state.data_ptr(), stream=stream.cuda_stream,
                    max_bounces=3)
    stream.synchronize()
    for n in names:
        assert t[n].cpu().numpy().tobytes() == want[n].tobytes(), n
    assert state.cpu().numpy().tobytes() == want["state"].tobytes()


def test_route_error_paths_on_the_device(rtow):
    L = rtow.route_lib()
    cam = rtow.camera_cpu(aspect=64 / 36)
    with rtow.Context(0) as c:
        p = rtow.make_params(64, 36, 1)
        with pytest.raises(rtow.RTError) as e:
            c.route(cam, p)
        assert e.value.status == -6  # RT_ERR_NO_SCENE
        c.upload(rtow.five_scene())
        bufs = rtow.RouteBuffers()  # every pointer NULL: RT_OK, nothing launched, the state never touched
        args = (c._h, ctypes.byref(cam), ctypes.byref(p), None, ctypes.byref(bufs))
        assert L.rt_route(*args, None) == 0
        assert L.rt_route_async(*args, ctypes.c_void_p(16), None) == 0
        bad = rtow.make_params(64, 36, 1)
        bad.band_offset = 1  # >= band_stride
        assert L.rt_route(c._h, ctypes.byref(cam), ctypes.byref(bad), None, ctypes.byref(bufs), None) == \
            rtow.RT_ERR_INVALID
        out = c.route(cam, rtow.make_params(67, 37, 0), which=ALL)  # spp = 0: the initial state
        for n in NAMES:
            assert np.all(out[n] == {"id": -1, "route": rtow.ROUTE_NO_HIT}.get(n, 0)), n
        assert np.all(out["state"] == route_ref.make_state(0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, -1)[:, None, None, :])


# ---- 5. the consumer --------------------------------------------------------
@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_denoise_with_route_guides(rtow, gpu_ctx, scene_name):
    """test_denoise_with_chain_guides' protocol at 128x72: 16 spp (seed 5)
    denoised at the defaults with rt_aov's, rt_guides' and rt_route's guides,
    against the product's 4096-spp render (seed 99); MSE on sqrt(mean) clamped
    to [0, 1], over the pixels whose first hit is a dielectric or a fuzz-0
    metal and over the frame.  The pass was built to beat the chain guides on
    the five-sphere scene's masked pixels, and on the MI355X it does not:
    masked error 16 spp 3.0612e-3, first-hit 8.6567e-4, chain 2.7579e-3, route
    2.7921e-3 (final scene: 8.6812e-4, 8.3814e-4, 7.3148e-4, route 7.1526e-4).
    The hollow shell's masked pixels split over six dominant routes ((bounces,
    escaped): (1,0) 181, (1,1) 215, (3,0) 175, (3,1) 115, (4,0) 317, (4,1)
    197, others 22; 79.4 % of their hit samples matched), so neighbouring
    pixels carry different routes' features and the filter's edge-stopping
    weights stay closed.  As DESIGN.md 10 and 14 did, the figures are printed,
    not asserted; rt_denoise's defaults were not touched."""
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
    first, chain, route = gpu_ctx.aov(cam, p16), gpu_ctx.guides(cam, p16), gpu_ctx.route(cam, p16)
    spec = _continues(rtow, scene, 0.0)
    mask = (first["id"] >= 0) & spec[np.maximum(first["id"], 0)]
    assert mask.mean() >= 0.03
    den = {"noisy": noisy, "first": gpu_ctx.denoise(noisy, first, 16), "chain": gpu_ctx.denoise(noisy, chain, 16),
           "route": gpu_ctx.denoise(noisy, route, 16)}
    e = {k: (_mse(v, 16, truth, mask), _mse(v, 16, truth)) for k, v in den.items()}
    print("route quality %s: masked pixels %.3f of the frame; mse masked / frame: 16 spp %.4e / %.4e, first-hit guides "
          "%.4e / %.4e, chain guides %.4e / %.4e, route guides %.4e / %.4e" %
          (scene_name, mask.mean(), *e["noisy"], *e["first"], *e["chain"], *e["route"]))
    keys, counts = np.unique(route["route"][mask], return_counts=True)
    share = route["matched"][mask].sum() / max(int(route["hits"][mask].sum()), 1)
    print("route census %s, masked pixels by dominant route (bounces, escaped): %s; matched / hits %.3f" %
          (scene_name, {(int(k) >> 1, int(k) & 1): int(c) for k, c in zip(keys, counts)}, share))
    print("route quality %s: route guides %s the chain guides on the masked pixels" %
          (scene_name, "beat" if e["route"][0] < e["chain"][0] else "do not beat"))
    assert all(np.isfinite(v).all() for v in den.values())
    # the buffers keep the sum contract the filter reads: the route's features where its samples hit
    assert np.array_equal(route["hits"], chain["hits"]) and np.array_equal(route["hits"] > 0, route["matched"] > 0)


def test_cli_denoise_guides_route(rtow, gpu_ctx):
    """gpu_ray_tracer --denoise --denoise-guides=route writes the bytes the
    Python path gives with rt_route at its defaults."""
    w, h, spp, seed = 64, 36, 8, 11
    gpu_ctx.upload(rtow.final_scene())
    cam = rtow.camera_gpu(w, h, defocus_angle=0.6, focus_dist=10.0)
    p = rtow.make_params(w, h, spp, max_depth=50, seed=seed,
                         flags=rtow.RT_FLAG_GPU_SEMANTICS | rtow.RT_FLAG_ACCEL_BVH)
    sums = gpu_ctx.render(cam, p)[0]
    chain = gpu_ctx.denoise(sums, gpu_ctx.guides(cam, p), spp)
    route = gpu_ctx.denoise(sums, gpu_ctx.route(cam, p), spp)
    tone = lambda x: rtow.tonemap(x, spp, rtow.RT_TONEMAP_GPU)  # noqa: E731
    assert not np.array_equal(tone(route), tone(chain))
    r = _cli(["--denoise", "--denoise-guides=route"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert np.array_equal(read_ppm_bytes(r.stdout), tone(route))
    r = _cli(["--denoise-guides=route"])  # the guides are the filter's
    assert r.returncode != 0 and r.stdout == b""
