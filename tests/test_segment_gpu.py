"""Closest hits within a per-ray distance limit on the GPU (include/rt_segment.h,
rt_segment / Context.segment / Context.visible): every output byte is what
tests/segment_cases.py derives from the CPU oracle's rt_trace records on its
limit lists (no tolerance); without a limit the pass is rt_trace; at the
boundary every walk gives the scan's bytes and a larger limit never loses a
hit; one answer from every walk, placement, cell size, launch split and
position in the batch; rays that are never traced leave their neighbours alone;
renders and rt_trace around a pass are unchanged."""
import ctypes

import numpy as np
import pytest

import ray_fans as rf
import segment_cases as sg
import trace_cases as tc

pytestmark = pytest.mark.gpu

NAMES = sg.NAMES
BVH, LAYER_BVH, OPEN = 1 << 9, (1 << 9) | (1 << 12), 1
LAYER_WALKS = (("scan", 0, None), ("layer_bvh", LAYER_BVH, None), ("grid-lds", BVH, "lds"),
               ("grid-cells", BVH, "cells"), ("grid-global", BVH, "global"))
PLAIN_WALKS = (("scan", 0, None), ("bvh", BVH, None))
KEYS = sg.FACTORS + ("mixed",)


def _walks(name):
    return LAYER_WALKS if name in rf.LAYER_SCENES else PLAIN_WALKS


def _same(got, want, what, names=NAMES):
    for n in names:
        if got[n].tobytes() != want[n].tobytes():
            a, b = got[n].reshape(len(want[n]), -1), want[n].reshape(len(want[n]), -1)
            u = np.uint8 if a.dtype == np.uint8 else np.uint32
            bad = np.nonzero((a.view(u) != b.view(u)).any(1))[0]
            raise AssertionError((what, n, len(bad), bad[:8].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist()))


@pytest.fixture
def ctx(rtow, gpu_ctx):
    """The session's context with its options at their defaults afterwards."""
    yield gpu_ctx
    gpu_ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_SCALE, 0)


def _segment(ctx, name, t_max, flags=0, sel=None, which=NAMES):
    """t_max: an array, None, or a key of the limit list of the flags' interval."""
    L = tc.rays_of(name)
    if isinstance(t_max, (str, float)):
        t_max = sg.limits_of(name, flags & OPEN)[t_max]
    if sel is not None:
        t_max = None if t_max is None else t_max[sel]
    o, d = (L["o"], L["d"]) if sel is None else (L["o"][sel], L["d"][sel])
    return ctx.segment(o, d, t_max, which=which, flags=flags)


# ---- 1. the oracle ------------------------------------------------------------
@pytest.mark.parametrize("scene_name", list(rf.SCENES))
def test_segment_is_the_expected_record_in_every_walk(rtow, ctx, scene_name):
    """All five outputs on the four factor lists and the mixed list, both
    interval flags, the scan, the BVH (or layer BVH) and on the layer scenes
    the grid in its three placements: f >= 1.25 the oracle's record, f <= 0.75
    a miss, never-traced and invalid rays as the header says."""
    for walk, accel, mode in _walks(scene_name):
        ctx.upload(rf.scene_of(scene_name), grid_mode=mode or "auto")
        for interval in (0, OPEN):
            for key in KEYS:
                got = _segment(ctx, scene_name, key, accel | interval)
                assert sorted(got) == sorted(NAMES + ("kernel_ms",))
                _same(got, sg.want_of(scene_name, key, interval), (scene_name, walk, interval, key))


@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("scene_name", rf.LAYER_SCENES)
def test_segment_is_the_expected_record_at_other_cell_sizes(rtow, ctx, scene_name, scale):
    for mode in ("lds", "cells", "global"):
        ctx.upload(rf.scene_of(scene_name), grid_mode=mode, grid_scale=scale)
        assert ctx.grid_scale() == scale
        for key in KEYS:
            _same(_segment(ctx, scene_name, key, BVH), sg.want_of(scene_name, key), (scene_name, mode, scale, key))


# ---- 2. no limit ----------------------------------------------------------------
@pytest.mark.parametrize("scene_name", list(rf.SCENES))
def test_without_a_limit_the_pass_is_rt_trace(rtow, ctx, scene_name):
    """t_max = NULL, all +inf and all 1e30 (times a length of 1e3: the product
    stays finite; of 1e-3 too) on the full lists: the oracle's rt_trace records
    byte for byte, and rt_trace's own output, in every walk."""
    n = tc.rays_of(scene_name)["n"]
    for walk, accel, mode in _walks(scene_name):
        ctx.upload(rf.scene_of(scene_name), grid_mode=mode or "auto")
        for interval in (0, OPEN):
            want = sg.unlimited_want(scene_name, interval)
            for what, tm in (("NULL", None), ("+inf", np.full(n, np.inf, np.float32)), ("1e30", np.full(n, 1e30, np.float32))):
                _same(_segment(ctx, scene_name, tm, accel | interval), want, (scene_name, walk, interval, what))
        L = tc.rays_of(scene_name)
        _same(ctx.trace(L["o"], L["d"], flags=accel), _segment(ctx, scene_name, None, accel), (scene_name, walk, "rt_trace"),
              NAMES[1:])
    # a product that overflows: t_max = 3e38 on the rays of length 1e3
    _same(_segment(ctx, scene_name, np.full(n, 3e38, np.float32), BVH), sg.unlimited_want(scene_name), "overflow")


# ---- 3. at the boundary -----------------------------------------------------------
@pytest.mark.parametrize("scene_name", list(rf.SCENES))
def test_at_the_boundary_every_walk_gives_the_scans_bytes(rtow, ctx, scene_name):
    """Limits at each ray's fl32(t_o / len) and at its two float neighbours,
    where the scan root and the limit differ by the scan's rounding and the
    strict rule decides.  No oracle judgement: every walk gives the bytes of the
    pass's own scan variant, under both interval flags.  And a ray blocked at a
    limit is blocked, with the same record, at every larger limit (the three,
    then +inf); what it is blocked by is the oracle's record."""
    limits = sg.boundary_limits(scene_name) + (np.full(tc.rays_of(scene_name)["n"], np.inf, np.float32),)
    ref = {}
    for walk, accel, mode in _walks(scene_name):
        ctx.upload(rf.scene_of(scene_name), grid_mode=mode or "auto")
        for interval in (0, OPEN):
            for k, tm in enumerate(limits):
                got = _segment(ctx, scene_name, tm, accel | interval)
                if walk == "scan":
                    ref[interval, k] = got
                else:
                    _same(got, ref[interval, k], (scene_name, walk, interval, k))
    kinds = np.zeros(3, int)
    for interval in (0, OPEN):
        full = sg.unlimited_want(scene_name, interval)
        _same(ref[interval, 3], full, (scene_name, "+inf", interval))
        for k in range(3):
            b = ref[interval, k]["blocked"] == 1
            kinds[k] += int(b.sum())
            assert (ref[interval, k + 1]["blocked"][b] == 1).all(), (scene_name, interval, k)
            for n in NAMES:  # blocked: the unlimited record (so the same at every larger limit)
                assert ref[interval, k][n][b].tobytes() == full[n][b].tobytes(), (scene_name, interval, k, n)
            miss = ~b & tc.rays_of(scene_name)["valid"]
            assert (ref[interval, k]["id"][miss] == rtow.SEGMENT_MISS).all() and np.isinf(ref[interval, k]["t"][miss]).all()
    print(scene_name, "blocked below / at / above the boundary (both flags):", kinds.tolist())


# ---- 4. position in the batch, launch split ---------------------------------------
@pytest.mark.parametrize("scene_name", list(rf.SCENES))
def test_a_rays_result_does_not_depend_on_its_place_in_the_batch(rtow, ctx, scene_name):
    """The mixed list reversed and permuted gives the permuted bytes; prefixes
    of 1, 63, 64, 65 and 257 rays the prefix's; 64 and 100 rays per launch the
    same bytes."""
    ctx.upload(rf.scene_of(scene_name))
    want = sg.want_of(scene_name, "mixed")
    n = tc.rays_of(scene_name)["n"]
    perm = np.random.default_rng(5).permutation(n)
    for what, sel in (("reversed", np.arange(n)[::-1]), ("permuted", perm)):
        _same(_segment(ctx, scene_name, "mixed", BVH, sel), {k: want[k][sel] for k in NAMES}, (scene_name, what))
    assert n > 257
    for m in (1, 63, 64, 65, 257):
        _same(_segment(ctx, scene_name, "mixed", BVH, np.arange(m)), {k: want[k][:m] for k in NAMES},
              (scene_name, "prefix", m))
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 64)
    for flags in (0, BVH):
        _same(_segment(ctx, scene_name, "mixed", flags), want, (scene_name, "64 rays per launch", flags))
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 100)
    _same(_segment(ctx, scene_name, "mixed", BVH), want, (scene_name, "100 rays per launch"))


# ---- 5. rays that are never traced ---------------------------------------------------
def test_untraced_rays_are_flagged_and_leave_their_neighbours_alone(rtow, ctx):
    """t_max of either zero, -1 and -inf: a miss; NaN, and rt_trace's invalid
    forms: id = -2; all with blocked = 0, t = +inf and zeros.  The same batch
    with those rays replaced by a plain unlimited ray gives every other ray the
    same bytes."""
    ctx.upload(rf.scene_of("final"))
    L, want = tc.rays_of("final"), sg.want_of("final", "mixed")
    tm = sg.limits_of("final")["mixed"]
    got = _segment(ctx, "final", "mixed", BVH)
    special = np.zeros(L["n"], bool)
    special[[i for i, v in sg.SPECIAL if not v > 0]] = True  # zeros, negatives, NaN
    special |= ~L["valid"]
    nan = np.isnan(tm) | ~L["valid"]
    assert (got["id"][nan] == rtow.SEGMENT_INVALID).all() and (got["id"][special & ~nan] == rtow.SEGMENT_MISS).all()
    assert (got["blocked"][special] == 0).all() and (got["t"][special] == np.inf).all()
    assert got["position"][special].tobytes() == got["normal"][special].tobytes() == bytes(12 * int(special.sum()))
    o, d, t2 = L["o"].copy(), L["d"].copy(), tm.copy()
    o[special], d[special], t2[special] = L["o"][0], L["d"][0], np.inf
    clean = ctx.segment(o, d, t2, flags=BVH)
    first = sg.unlimited_want("final")
    for k in NAMES:
        assert clean[k][~special].tobytes() == want[k][~special].tobytes(), k
        assert clean[k][special].tobytes() == np.repeat(first[k][:1], special.sum(), 0).tobytes(), k
    only = ctx.segment(L["o"][special], L["d"][special], tm[special], flags=BVH)
    assert (only["id"] < 0).all() and (only["blocked"] == 0).all() and (only["t"] == np.inf).all()


# ---- 6. NULL outputs -------------------------------------------------------------------
def test_null_outputs(rtow, ctx):
    """Every single output alone (blocked alone among them), all five, and
    nothing wanted."""
    ctx.upload(rf.scene_of("five"))
    want = sg.want_of("five", "mixed")
    for which in [(n,) for n in NAMES] + [NAMES, ("blocked", "t"), ("id", "normal")]:
        got = _segment(ctx, "five", "mixed", BVH, which=which)
        assert sorted(got) == sorted(tuple(which) + ("kernel_ms",))
        _same(got, want, which, which)
    assert list(_segment(ctx, "five", "mixed", BVH, which=())) == ["kernel_ms"]


def test_segment_error_paths_on_the_device(rtow):
    L = rtow.segment_lib()
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)
    with rtow.Context(0) as c:
        with pytest.raises(rtow.RTError) as e:
            c.segment(o, d, 1.0)
        assert e.value.status == rtow.RT_ERR_NO_SCENE
        with pytest.raises(rtow.RTError) as e:
            c.segment_async({"origin": 256, "direction": 512, "blocked": 1024}, 4)
        assert e.value.status == rtow.RT_ERR_NO_SCENE
        c.upload(rtow.five_scene())
        # n = 0, or every output NULL: RT_OK, nothing launched (the pointers are never read)
        rays, hits = rtow.SegmentRays(n=0), rtow.SegmentHits()
        assert L.rt_segment(c._h, ctypes.byref(rays), ctypes.byref(hits), 0, None) == 0
        assert L.rt_segment_async(c._h, ctypes.byref(rays), ctypes.byref(hits), 0, None) == 0
        rays = rtow.SegmentRays(n=4, origin=o.ctypes.data, direction=d.ctypes.data)
        assert L.rt_segment(c._h, ctypes.byref(rays), ctypes.byref(hits), 0, None) == 0
        assert L.rt_segment_async(c._h, ctypes.byref(rays), ctypes.byref(hits), 0, None) == 0
        empty = c.segment(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
        assert empty["blocked"].shape == (0,) and empty["position"].shape == (0, 3)
        # a scalar t_max is every ray's; other flag bits are ignored
        R = tc.rays_of("five")
        a = c.segment(R["o"], R["d"], 2.5, flags=BVH)
        b = c.segment(R["o"], R["d"], np.full(R["n"], 2.5, np.float32), flags=BVH | 2 | (1 << 8) | (1 << 10) | (1 << 11))
        _same(a, b, "scalar t_max, other flags")
        assert 0 < a["blocked"].sum() < (sg.unlimited_want("five")["blocked"]).sum()


# ---- 7. async, torch ------------------------------------------------------------------
def test_segment_async_on_a_second_stream_into_torch_tensors(rtow, ctx):
    import torch
    ctx.upload(rf.scene_of("final"))
    L, want = tc.rays_of("final"), sg.want_of("final", "mixed")
    n = L["n"]
    dev = torch.device("cuda:0")
    o = torch.from_numpy(L["o"].copy()).to(dev)
    d = torch.from_numpy(L["d"].copy()).to(dev)
    tm = torch.from_numpy(sg.limits_of("final")["mixed"].copy()).to(dev)
    out = {"blocked": torch.full((n,), 77, dtype=torch.uint8, device=dev),
           "id": torch.full((n,), 77, dtype=torch.int32, device=dev),
           "t": torch.full((n,), 7.0, dtype=torch.float32, device=dev),
           "position": torch.full((n, 3), 7.0, dtype=torch.float32, device=dev),
           "normal": torch.full((n, 3), 7.0, dtype=torch.float32, device=dev)}
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ptrs = {k: t.data_ptr() for k, t in out.items()}
    ptrs.update(origin=o.data_ptr(), direction=d.data_ptr(), t_max=tm.data_ptr())
    ctx.segment_async(ptrs, n, flags=BVH, stream=stream.cuda_stream)
    stream.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    _same(got, want, "async vs expected")
    # without t_max: rt_trace's records, blocked alone
    only = {"origin": o.data_ptr(), "direction": d.data_ptr(), "blocked": out["blocked"].data_ptr()}
    ctx.segment_async(only, n, flags=BVH, stream=stream.cuda_stream)
    stream.synchronize()
    assert out["blocked"].cpu().numpy().tobytes() == sg.unlimited_want("final")["blocked"].tobytes()
    # overlapping device ranges are rejected before anything is enqueued
    ptrs["blocked"] = ptrs["t_max"] + 3
    with pytest.raises(rtow.RTError) as e:
        ctx.segment_async(ptrs, n, flags=BVH, stream=stream.cuda_stream)
    assert e.value.status == rtow.RT_ERR_INVALID


# ---- 8. scene state -------------------------------------------------------------------
def test_renders_and_rt_trace_around_a_segment_pass_are_unchanged(rtow, ctx):
    scene = rf.scene_of("final")
    W, H = 320, 180
    cam = rtow.camera_cpu(aspect=W / H)
    p = rtow.make_params(W, H, 2, seed=3, flags=BVH)
    L = tc.rays_of("final")
    ctx.upload(scene)
    img0, st0 = ctx.render(cam, p)
    tr0 = ctx.trace(L["o"], L["d"], flags=BVH)
    before = _segment(ctx, "final", "mixed", BVH)
    img1, st1 = ctx.render(cam, p)
    after = _segment(ctx, "final", "mixed", BVH)
    tr1 = ctx.trace(L["o"], L["d"], flags=BVH)
    img2, st2 = ctx.render(cam, p)
    _same(before, sg.want_of("final", "mixed"), "before")
    _same(after, before, "after a render")
    assert img1.tobytes() == img0.tobytes() == img2.tobytes()
    assert st0.segments == st1.segments == st2.segments
    _same(tr1, tr0, "rt_trace", NAMES[1:])


# ---- 9. visible -----------------------------------------------------------------------
def test_visible_on_pairs_with_a_known_answer(rtow, ctx):
    """The final scene: the ground (centre (0, -1000, 0), r = 1000) and the big
    spheres of radius 1 at (0, 1, 0), (-4, 1, 0) and (4, 1, 0)."""
    ctx.upload(rtow.final_scene())
    pairs = [((-5.0, 30.0, 0.0), (5.0, 31.0, 3.0), True),     # two sky points above the scene
             ((20.0, 40.0, -7.0), (-3.0, 25.0, 9.0), True),
             ((0.0, 1.0, 3.0), (0.0, 1.0, -3.0), False),      # opposite sides of the glass sphere
             ((-4.0, 1.0, 2.5), (-4.0, 1.0, -2.5), False),    # ... of the diffuse one
             ((4.0, 3.5, 0.0), (4.0, -3.0, 0.0), False),      # ... and through it into the ground
             ((0.0, 30.0, 0.0), (0.0, -5.0, 30.0), False),    # a sky point and a point under the ground
             ((0.0, 2.0, 0.0), (0.0, 30.0, 0.0), True),       # from the top of a sphere: t_min skips its surface
             ((0.0, 30.0, 0.0), (0.0, 2.0, 0.0), True),       # to it: shrink stops short of the surface
             ((0.0, 30.0, 0.0), (0.0, 1.5, 0.0), False),      # to a point inside it
             ((0.0, 30.0, 0.0), (0.0, 2.5, 0.0), True)]       # to a point above it
    a = np.array([p[0] for p in pairs], np.float32)
    b = np.array([p[1] for p in pairs], np.float32)
    want = [p[2] for p in pairs]
    for flags in (0, BVH):
        v = ctx.visible(a, b, flags=flags)
        assert v.dtype == bool and v.tolist() == want, (flags, v.tolist())
        assert ctx.visible(b, a, flags=flags).tolist() == want  # (the other way round: the same here)
    # from one point to many; shrink = 0 ends on the surface's root itself, shrink = 1 leaves nothing
    assert ctx.visible((0.0, 30.0, 0.0), b[[6, 7, 8, 9]]).tolist() == [True, True, False, True]
    assert ctx.visible(a, b, shrink=1.0).all()
    assert ctx.visible(a[8:9], b[8:9], shrink=0.0).tolist() == [False]
    # a point from itself is an invalid ray and not blocked
    assert ctx.visible(a[:1], a[:1]).tolist() == [True]
