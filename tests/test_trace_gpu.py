"""Closest-hit queries for ray batches on the GPU (include/rt_trace.h, rt_trace
/ Context.trace): every output byte is the CPU oracle's on tests/trace_cases.py's
lists (no tolerance, no ray left out but the invalid ones, which the oracle
never sees); one answer from every walk, placement, cell size, launch split
and position of a ray in its batch; invalid rays are flagged and leave their
neighbours alone; renders and rt_aov around a trace are unchanged; and rt_aov
itself, through a single-ray camera, reports the same bits."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import ray_fans as rf
import trace_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("id", "t", "position", "normal")
BVH, LAYER_BVH, OPEN = 1 << 9, (1 << 9) | (1 << 12), 1
LAYER_WALKS = (("scan", 0, None), ("layer_bvh", LAYER_BVH, None), ("grid-lds", BVH, "lds"),
               ("grid-cells", BVH, "cells"), ("grid-global", BVH, "global"))
PLAIN_WALKS = (("scan", 0, None), ("bvh", BVH, None))


def _walks(name):
    return LAYER_WALKS if name in rf.LAYER_SCENES else PLAIN_WALKS


def _same(got, want, what, names=NAMES):
    for n in names:
        if got[n].tobytes() != want[n].tobytes():
            a, b = got[n].reshape(len(want[n]), -1), want[n].reshape(len(want[n]), -1)
            bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(1))[0]
            raise AssertionError((what, n, len(bad), bad[:8].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist()))


@pytest.fixture
def ctx(rtow, gpu_ctx):
    """The session's context with its options at their defaults afterwards."""
    yield gpu_ctx
    gpu_ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_SCALE, 0)


def _trace(ctx, name, flags=0, sel=None, which=NAMES):
    L = tc.rays_of(name)
    o, d = (L["o"], L["d"]) if sel is None else (L["o"][sel], L["d"][sel])
    return ctx.trace(o, d, which=which, flags=flags)


# ---- 1. the oracle ------------------------------------------------------------
@pytest.mark.parametrize("scene_name", list(rf.SCENES))
def test_trace_is_the_oracles_in_every_walk(rtow, ctx, scene_name):
    """All four outputs, both interval flags, the scan, the BVH (or layer BVH)
    and on the layer scenes the grid in its three placements: the oracle's
    bytes.  The oracle is a brute-force scan that knows no walk, so this is
    also byte equality across the walks."""
    for walk, accel, mode in _walks(scene_name):
        if mode is not None:
            assert rtow.accel_info(rf.scene_of(scene_name), mode)["grid_placement"] == rtow.GRID_PLACEMENTS[mode]
        ctx.upload(rf.scene_of(scene_name), grid_mode=mode or "auto")
        for interval in (0, OPEN):
            got = _trace(ctx, scene_name, accel | interval)
            assert sorted(got) == sorted(NAMES + ("kernel_ms",))
            _same(got, tc.want_of(scene_name, interval), (scene_name, walk, interval))


@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("scene_name", rf.LAYER_SCENES)
def test_trace_is_the_oracles_at_other_cell_sizes(rtow, ctx, scene_name, scale):
    for mode in ("lds", "cells", "global"):
        ctx.upload(rf.scene_of(scene_name), grid_mode=mode, grid_scale=scale)
        assert ctx.grid_scale() == scale
        _same(_trace(ctx, scene_name, BVH), tc.want_of(scene_name), (scene_name, mode, scale))


# ---- 2. position in the batch, launch split -----------------------------------
@pytest.mark.parametrize("scene_name", list(rf.SCENES))
def test_a_rays_result_does_not_depend_on_its_place_in_the_batch(rtow, ctx, scene_name):
    """The list reversed and in a random permutation gives the permuted bytes
    (a ray's 63 wave neighbours change, the far origin at index 17 and the far
    wave are spread over other waves); prefixes of 1, 63, 64, 65 and 257 rays
    give the prefix of the full run; and RT_OPT_LAUNCH_SAMPLES = 64, one wave
    per launch, gives the same bytes."""
    ctx.upload(rf.scene_of(scene_name))
    want = tc.want_of(scene_name)
    n = tc.rays_of(scene_name)["n"]
    perm = np.random.default_rng(5).permutation(n)
    for what, sel in (("reversed", np.arange(n)[::-1]), ("permuted", perm)):
        got = _trace(ctx, scene_name, BVH, sel)
        _same(got, {k: want[k][sel] for k in NAMES}, (scene_name, what))
    assert n > 257  # (a block is 256 lanes: the last prefix and the full list run in two blocks)
    for m in (1, 63, 64, 65, 257):
        _same(_trace(ctx, scene_name, BVH, np.arange(m)), {k: want[k][:m] for k in NAMES}, (scene_name, "prefix", m))
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 64)
    for flags in (0, BVH):
        _same(_trace(ctx, scene_name, flags), want, (scene_name, "64 rays per launch", flags))
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 100)  # launches that end inside a wave and inside a block
    _same(_trace(ctx, scene_name, BVH), want, (scene_name, "100 rays per launch"))


@pytest.mark.parametrize("walk", LAYER_WALKS, ids=[w[0] for w in LAYER_WALKS])
def test_a_batch_of_several_blocks_is_the_concatenated_records(rtow, ctx, walk):
    """The final scene's list five times over, each copy in another
    permutation: 1445 rays, six blocks of 256 lanes, the last one partly
    filled, in every walk (each block stages the grid itself).  In one launch,
    and in launches of 512 (two whole blocks each, then a tail), 256, 300 and
    1000 rays: the concatenated oracle records, byte for byte."""
    _, accel, mode = walk
    L, want = tc.rays_of("final"), tc.want_of("final")
    n = L["n"]
    rng = np.random.default_rng(11)
    sel = np.concatenate([np.arange(n)] + [rng.permutation(n) for _ in range(4)])
    assert len(sel) > 5 * tc.BLOCK and len(sel) % tc.BLOCK != 0 and len(sel) % 512 > tc.BLOCK
    big = {k: want[k][sel] for k in NAMES}
    ctx.upload(rf.scene_of("final"), grid_mode=mode or "auto")
    for per in (0, 512, 256, 300, 1000):
        ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, per)
        _same(_trace(ctx, "final", accel, sel), big, (walk[0], "rays per launch", per))


# ---- 3. scene state -------------------------------------------------------------
def test_trace_does_not_depend_on_the_grid_fit_and_leaves_renders_alone(rtow, ctx):
    """A trace before any render (the builder's grid) equals a trace after a
    render that refitted the grid for its frame; the render and rt_aov around
    the traces give the bytes they give without them, and the render's segment
    count is not touched."""
    scene = rf.scene_of("final")
    W, H = 320, 180
    cam = rtow.camera_cpu(aspect=W / H)
    p = rtow.make_params(W, H, 2, seed=3, flags=BVH)
    ctx.upload(scene)
    img0, st0 = ctx.render(cam, p)
    aov0 = ctx.aov(cam, p)
    ctx.upload(scene)  # a fresh scene state: the builder's grid
    g0 = ctx.grid_scale()
    before = _trace(ctx, "final", BVH)
    img1, st1 = ctx.render(cam, p)
    g1 = ctx.grid_scale()
    after = _trace(ctx, "final", BVH)
    aov1 = ctx.aov(cam, p)
    img2, st2 = ctx.render(cam, p)
    print("grid scale: the builder's %r, fitted for %dx%d %r" % (g0, W, H, g1))
    assert g1 == pytest.approx(rtow.grid_fit(scene, cam, W, H)[0], abs=1e-12) and g0 != g1  # the render refitted the grid
    _same(before, tc.want_of("final"), "before the refit")
    _same(after, before, "after the refit")
    assert img1.tobytes() == img0.tobytes() == img2.tobytes()
    assert st0.segments == st1.segments == st2.segments
    for k in ("hits", "id", "depth", "position", "normal", "albedo"):
        assert aov0[k].tobytes() == aov1[k].tobytes(), k


# ---- 4. invalid rays, NULL outputs -------------------------------------------------
def test_invalid_rays_are_flagged_and_leave_their_neighbours_alone(rtow, ctx):
    """Each invalid form gives id = -2, t = +inf and zeros; the same batch with
    the invalid rays replaced by a plain valid ray gives every other ray the
    same bytes (two waves of the list hold invalid rays)."""
    ctx.upload(rf.scene_of("final"))
    L, want = tc.rays_of("final"), tc.want_of("final")
    got = _trace(ctx, "final", BVH)
    inv = ~L["valid"]
    assert inv.sum() == len(tc.INVALID)
    assert (got["id"][inv] == rtow.TRACE_INVALID).all() and (got["t"][inv] == np.inf).all()
    assert got["position"][inv].tobytes() == got["normal"][inv].tobytes() == bytes(12 * int(inv.sum()))
    o, d = L["o"].copy(), L["d"].copy()
    o[inv], d[inv] = L["o"][0], L["d"][0]
    clean = ctx.trace(o, d, flags=BVH)
    for k in NAMES:
        assert clean[k][~inv].tobytes() == want[k][~inv].tobytes(), k
        assert clean[k][inv].tobytes() == np.repeat(want[k][:1], inv.sum(), 0).tobytes(), k
    # a batch of invalid rays only: nothing is traced
    only = ctx.trace(L["o"][inv], L["d"][inv], flags=BVH)
    assert (only["id"] == rtow.TRACE_INVALID).all() and (only["t"] == np.inf).all()


def test_null_outputs_in_every_combination(rtow, ctx):
    ctx.upload(rf.scene_of("five"))
    want = tc.want_of("five")
    for k in range(1, 5):
        for which in itertools.combinations(NAMES, k):
            got = _trace(ctx, "five", BVH, which=which)
            assert sorted(got) == sorted(which + ("kernel_ms",))
            _same(got, want, which, which)
    assert list(_trace(ctx, "five", BVH, which=())) == ["kernel_ms"]


def test_trace_error_paths_on_the_device(rtow):
    L = rtow.trace_lib()
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)
    with rtow.Context(0) as c:
        with pytest.raises(rtow.RTError) as e:
            c.trace(o, d)
        assert e.value.status == rtow.RT_ERR_NO_SCENE
        with pytest.raises(rtow.RTError) as e:
            c.trace_async({"origin": 256, "direction": 512, "id": 1024}, 4)
        assert e.value.status == rtow.RT_ERR_NO_SCENE
        c.upload(rtow.five_scene())
        # n = 0, or every output NULL: RT_OK, nothing launched (the pointers are never read)
        rays, hits = rtow.TraceRays(n=0), rtow.TraceHits()
        assert L.rt_trace(c._h, ctypes.byref(rays), ctypes.byref(hits), 0, None) == 0
        assert L.rt_trace_async(c._h, ctypes.byref(rays), ctypes.byref(hits), 0, None) == 0
        rays = rtow.TraceRays(n=4, origin=o.ctypes.data, direction=d.ctypes.data)
        assert L.rt_trace(c._h, ctypes.byref(rays), ctypes.byref(hits), 0, None) == 0
        assert L.rt_trace_async(c._h, ctypes.byref(rays), ctypes.byref(hits), 0, None) == 0
        empty = c.trace(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
        assert empty["id"].shape == (0,) and empty["position"].shape == (0, 3)
        # other flag bits are ignored
        a = c.trace(tc.rays_of("five")["o"], tc.rays_of("five")["d"], flags=BVH)
        b = c.trace(tc.rays_of("five")["o"], tc.rays_of("five")["d"], flags=BVH | 2 | (1 << 8) | (1 << 10) | (1 << 11))
        _same(a, b, "other flags")
        _same(a, tc.want_of("five"), "own context")


# ---- 5. async, torch ------------------------------------------------------------------
def test_trace_async_on_a_second_stream_into_torch_tensors(rtow, ctx):
    import torch
    ctx.upload(rf.scene_of("final"))
    L, want = tc.rays_of("final"), tc.want_of("final")
    n = L["n"]
    dev = torch.device("cuda:0")
    o = torch.from_numpy(L["o"].copy()).to(dev)
    d = torch.from_numpy(L["d"].copy()).to(dev)
    out = {"id": torch.full((n,), 77, dtype=torch.int32, device=dev),
           "t": torch.full((n,), 7.0, dtype=torch.float32, device=dev),
           "position": torch.full((n, 3), 7.0, dtype=torch.float32, device=dev),
           "normal": torch.full((n, 3), 7.0, dtype=torch.float32, device=dev)}
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ptrs = {k: t.data_ptr() for k, t in out.items()}
    ptrs.update(origin=o.data_ptr(), direction=d.data_ptr())
    ctx.trace_async(ptrs, n, flags=BVH, stream=stream.cuda_stream)
    stream.synchronize()
    sync = _trace(ctx, "final", BVH)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    _same(got, sync, "async vs sync")
    _same(got, want, "async vs oracle")
    # overlapping device ranges are rejected before anything is enqueued
    ptrs["normal"] = ptrs["position"] + 12
    with pytest.raises(rtow.RTError) as e:
        ctx.trace_async(ptrs, n, flags=BVH, stream=stream.cuda_stream)
    assert e.value.status == rtow.RT_ERR_INVALID


# ---- 6. load order ------------------------------------------------------------------------
_BOTH_LIBRARIES_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import rtow
rtow.aov_lib(), rtow.trace_lib()  # both loaded before either pass runs
import ray_fans as rf
import trace_cases as tc
L = tc.rays_of("five")
view = dict(lookfrom=(-2.0, 0.5, 2.0), lookat=(0.0, 0.0, -1.0), vfov=40.0, focus_dist=3.4)
p = rtow.make_params(16, 16, 2, seed=11, flags=rtow.RT_FLAG_ACCEL_BVH)
lens, pinhole = (rtow.camera_cpu(aspect=1.0, aperture=a, **view) for a in (0.1, 0.0))
with rtow.Context(0) as ctx:
    ctx.upload(rf.scene_of("five"))
    calls = {"aov": lambda: ctx.aov(lens, p), "trace": lambda: ctx.trace(L["o"], L["d"], flags=rtow.RT_FLAG_ACCEL_BVH)}
    got = {name: calls[name]() for name in sys.argv[3:]}  # in the order under test
    want = tc.want_of("five")
    for k in ("id", "t", "position", "normal"):
        assert got["trace"][k].tobytes() == want[k].tobytes(), k
    # rt_aov's lens table is its own: a lens moves its positions
    sharp = ctx.aov(pinhole, p)
    assert (got["aov"]["hits"] > 0).any() and got["aov"]["position"].tobytes() != sharp["position"].tobytes()
print("ok")
"""


def test_trace_and_aov_in_one_process_in_both_load_orders():
    """librtow_trace.so and librtow_aov.so, both -Bsymbolic with device code of
    their own, loaded into one fresh process; whichever pass runs first, the
    trace gives the oracle's bytes and rt_aov still samples its lens."""
    pkg = os.path.join(ROOT, "ray-tracing-in-one-weekend_amd")
    for order in (("trace", "aov"), ("aov", "trace")):
        r = subprocess.run([sys.executable, "-c", _BOTH_LIBRARIES_CHILD, pkg, os.path.join(ROOT, "tests"), *order],
                           capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (order, r.stderr[-2000:])


# ---- 7. without the oracle ------------------------------------------------------------------
def test_rt_aov_through_a_single_ray_camera_reports_the_same_bits(rtow, ctx):
    """trace_cases.AOV_CHECK's ten rays (hits on a layer sphere, a grazing one,
    from inside glass, on the ground, axis-parallel with +0 and -0, from beyond
    oref, a frozen skip that then hits and one that then misses, a sky miss) as
    rt_aov sees them: 1 spp
    through the ray's single-ray camera on the 8 x 8 frame.  Every pixel's id,
    depth, position and normal are rt_trace's id, t, position and normal."""
    ctx.upload(rf.scene_of("final"))
    L = tc.rays_of("final")
    got = _trace(ctx, "final", BVH)
    tags = L["tags"]
    picks = tc.aov_check_rays("final")  # (index, tag, kind), fixed by the list and the oracle
    pick = [i for i, _, _ in picks]
    assert len(set(pick)) >= 8
    for i, tag, kind in picks:
        assert (got["id"][i] >= 0) == (kind == "hit"), (i, tag, kind)
    p = rtow.make_params(tc.FRAME[0], tc.FRAME[1], 1, seed=1, flags=BVH)
    for i in pick:
        a = ctx.aov(L["cams"][i], p)
        hit = got["id"][i] >= 0
        assert (a["hits"] == (1 if hit else 0)).all(), (i, tags[i])
        assert (a["id"] == got["id"][i]).all(), (i, tags[i])
        if hit:  # (rt_aov's values are sums from +0: a component of -0 reads +0 there)
            zero = np.float32(0.0)
            assert (a["depth"].view(np.uint32) == (zero + got["t"][i]).view(np.uint32)).all(), (i, tags[i])
            assert (a["position"].view(np.uint32) == (zero + got["position"][i]).view(np.uint32)).all(), (i, tags[i])
            assert (a["normal"].view(np.uint32) == (zero + got["normal"][i]).view(np.uint32)).all(), (i, tags[i])
