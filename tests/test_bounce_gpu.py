"""The render's path step for ray batches on the GPU (include/rt_bounce.h,
rt_bounce / Context.bounce, Context.camera_rays): a wavefront loop over the
pass reproduces rt_render and the CPU oracle's render bit for bit, its
intermediate states are the oracle's chain records, the camera rays are the
render's, a ray's result depends on nothing but the ray, and the pass leaves
renders, rt_trace and rt_segment alone.  Every comparison is byte equality."""
import ctypes

import numpy as np
import pytest

import bounce_cases as bc
import features_cases as fc
import oracle_lib

pytestmark = pytest.mark.gpu

EV = oracle_lib.EVENTS
OUT = ("status", "id", "t", "position", "normal", "scatter", "attenuation")


@pytest.fixture
def ctx(rtow, gpu_ctx):
    """The session's context with its options at their defaults afterwards."""
    yield gpu_ctx
    gpu_ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_SCALE, 0)


def _same(got, want, what, names=OUT):
    for n in names:
        if got[n].tobytes() != want[n].tobytes():
            a, b = got[n].reshape(len(want[n]), -1), want[n].reshape(len(want[n]), -1)
            bad = np.nonzero((a.view(np.uint8) != b.view(np.uint8)).any(1))[0]
            raise AssertionError((what, n, len(bad), bad[:8].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist()))


# ---- 1. the render judge ---------------------------------------------------------
@pytest.mark.parametrize("case", bc.RENDER_CASES)
def test_path_trace_is_the_render_and_the_oracles_render(rtow, ctx, case):
    """rtow.path_trace -- camera rays, max_depth steps of rt_bounce with
    compaction, the pixel sums restated in numpy -- gives rt_render's bytes and
    the oracle's, and traces as many rays as the render counts segments: every
    frame of the case, max_depth 50 and 3, every walk of the scene."""
    scene = fc.scene_of(rtow, case)
    for frame in fc.frames_of(case):
        cam = fc.camera_of(rtow, case, frame)
        for depth in bc.DEPTHS:
            want, segs = oracle_lib.kernel_render(scene, cam, bc.params_of(rtow, case, frame, depth))
            for walk, accel, mode in bc.walks_of(rtow, case):
                ctx.upload(scene, grid_mode=mode or "auto")
                p = bc.params_of(rtow, case, frame, depth, accel)
                what = (case, frame, depth, walk)
                got, traced = rtow.path_trace(ctx, cam, p)
                assert got.dtype == want.dtype and got.shape == want.shape, what
                bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
                assert got.tobytes() == want.tobytes(), (what, len(bad[0]), [b[:4].tolist() for b in bad])
                assert traced == segs, (what, traced, segs)
                img, st = ctx.render(cam, p)
                assert img.tobytes() == got.tobytes(), what
                assert st.segments == traced, what


# ---- 2. the chain judge ----------------------------------------------------------
@pytest.mark.parametrize("case", bc.CHAIN_CASES)
def test_the_chain_over_bounces_is_the_oracles_terminals(rtow, ctx, case):
    """Following only specular continuations for -1 (nothing), 1, 2 and 8
    bounces, with total += t and thr = fmin(thr * attenuation, 2^100): the
    terminal is rto_kernel_terminals' record (rt_guides' form of a skip)."""
    ctx.upload(fc.scene_of(rtow, case))
    frame = fc.frames_of(case)[0]
    cam, p = fc.camera_of(rtow, case, frame), fc.params_of(rtow, case, frame)
    runs = [(k, f) for k in bc.CHAIN_BOUNCES for f in bc.CHAIN_FUZZ]
    if case == "clamp":
        runs.append((bc.CLAMP_BOUNCES, 0.0))
    for k, fuzz in runs:
        want = fc.terminals(rtow, case, frame, k, fuzz, keep_dir=False)
        got = bc.chain(rtow, ctx, cam, p, k, fuzz)
        assert got.shape == want.shape
        for name in bc.CHAIN_FIELDS:
            if got[name].tobytes() != want[name].tobytes():
                bad = np.argwhere((got[name] != want[name]).reshape(want.shape + (-1,)).any(-1))
                i = tuple(bad[0])
                raise AssertionError((case, k, fuzz, name, len(bad), i, got[i], want[i]))


# ---- 3. camera rays --------------------------------------------------------------
@pytest.mark.parametrize("case", bc.CAMERA_CASES)
def test_camera_rays_are_the_renders(rtow, ctx, case):
    """rt_trace on the camera rays gives the oracle's first-hit records in
    rt_aov's form, sample by sample, wherever the record has no SKIP_TMIN
    event, and rt_aov's buffers at 1 spp for sample 0; the origins are the
    oracle's; keys are (pix, s, 0); padding rows are zeros and come back
    INVALID from rt_bounce and rt_trace."""
    ctx.upload(fc.scene_of(rtow, case))
    for frame in fc.frames_of(case):
        cam, p = fc.camera_of(rtow, case, frame), fc.params_of(rtow, case, frame)
        o, d, key = ctx.camera_rays(cam, p)
        shape = (p.local_rows, p.width, p.spp)
        assert o.shape == d.shape == key.shape == (int(np.prod(shape)), 3)
        assert o.reshape(shape + (3,)).tobytes() == oracle_lib.camera_origins(cam, p).tobytes(), (case, frame)
        grow = rtow.local_to_global_rows(p)
        inside = np.broadcast_to((grow < p.height)[:, None, None], shape).ravel()
        pix = np.broadcast_to((grow[:, None] * p.width + np.arange(p.width)[None, :])[:, :, None], shape).ravel()
        smp = np.broadcast_to(np.arange(p.spp)[None, None, :], shape).ravel()
        assert (key[inside, 0] == pix[inside]).all() and (key[:, 1] == smp).all() and not key[:, 2].any()
        if "bands" in fc.CASES[case]:
            assert not inside.all()  # the banded case has padding rows
        pad = ~inside
        assert not o[pad].any() and not d[pad].any() and not key[pad, 0].any()
        tr = ctx.trace(o, d, flags=p.flags)
        bo = ctx.bounce(o, d, key, p.seed, flags=p.flags)
        assert (tr["id"][pad] == rtow.TRACE_INVALID).all() and (bo["status"][pad] == rtow.BOUNCE_INVALID).all()
        assert (bo["id"][pad] == -2).all() and np.isinf(bo["t"][pad]).all() and not bo["attenuation"][pad].any()
        assert not (bo["status"][inside] == rtow.BOUNCE_INVALID).any()
        term = fc.terminals(rtow, case, frame, -1, 0.0, keep_dir=True).ravel()
        ok = inside & ((term["events"] & EV["skip_tmin"]) == 0)
        assert (tr["id"][ok] == term["sphere"][ok]).all(), (case, frame)
        hit = ok & (term["sphere"] >= 0)
        assert hit.any() or frame != fc.FRAMES[0]
        for name, field in (("t", "depth"), ("position", "P"), ("normal", "N")):
            assert tr[name][hit].tobytes() == term[field][hit].tobytes(), (case, frame, name)
        # without a skip rt_bounce's hit record is rt_trace's
        for name in ("id", "t", "position", "normal"):
            assert bo[name][ok].tobytes() == tr[name][ok].tobytes(), (case, frame, name)
        # a range of samples is that range of the full batch
        if p.spp >= 3:
            o2, d2, k2 = ctx.camera_rays(cam, p, sample0=1, samples=2)
            sel = np.arange(o.shape[0]).reshape(shape)[:, :, 1:3].ravel()
            assert o2.tobytes() == o[sel].tobytes() and d2.tobytes() == d[sel].tobytes() and k2.tobytes() == key[sel].tobytes()
        # rt_aov at 1 spp is sample 0 (its values are sums from +0)
        import copy
        p1 = copy.copy(p)
        p1.spp = 1
        a = ctx.aov(cam, p1)
        s0 = np.arange(o.shape[0]).reshape(shape)[:, :, 0]
        k0 = (inside & ((term["events"] & EV["skip_tmin"]) == 0)).reshape(shape)[:, :, 0]
        zero = np.float32(0.0)
        ids = np.where(tr["id"][s0] == rtow.TRACE_INVALID, -1, tr["id"][s0])
        assert (a["id"][k0] == ids[k0]).all() and (a["hits"][k0] == (ids[k0] >= 0)).all()
        h0 = k0 & (ids >= 0)
        assert (a["depth"][h0].view(np.uint32) == (zero + tr["t"][s0][h0]).view(np.uint32)).all()
        assert (a["position"][h0].view(np.uint32) == (zero + tr["position"][s0][h0]).view(np.uint32)).all()
        assert (a["normal"][h0].view(np.uint32) == (zero + tr["normal"][s0][h0]).view(np.uint32)).all()


# ---- 4. independence ---------------------------------------------------------------
def _uncompacted(rtow, ctx, cam, p, order=None):
    """path_trace without compaction: every step traces the whole batch (a
    finished path's slot holds an invalid ray), optionally with the batch in
    another order -> the image."""
    f32, spp = np.float32, p.spp
    scale = f32(2.0 ** (32 - max(spp, 1).bit_length()))
    o, d, key = ctx.camera_rays(cam, p)
    n = o.shape[0]
    order = np.arange(n) if order is None else order
    o, d, key = o[order], d[order], key[order]
    frm, thr, alive = np.full(n, -1, np.int32), np.ones((n, 3), f32), np.ones(n, bool)
    sums = np.zeros((p.local_rows * p.width, 3), np.uint64)
    for _ in range(p.max_depth):
        got = ctx.bounce(o, d, key, p.seed, frm, flags=p.flags)
        assert (got["status"][~alive] == rtow.BOUNCE_INVALID).all()
        thr = thr * got["attenuation"]
        miss = alive & (got["status"] == rtow.BOUNCE_MISS)
        np.add.at(sums, order[miss] // spp, np.trunc(thr[miss] * scale).astype(np.uint64))
        alive = alive & (got["status"] == rtow.BOUNCE_SCATTERED)
        o, d, frm = got["position"], got["scatter"], np.where(alive, got["id"], -1).astype(np.int32)  # (dead: d = +0)
        key = key + np.array([0, 0, 1], np.uint32)
        if not alive.any():
            break
    return (sums.astype(np.uint32).astype(f32) * (f32(1.0) / scale)).reshape(p.local_rows, p.width, 3)


def test_the_image_does_not_depend_on_compaction_order_launches_or_the_grid(rtow, ctx):
    case, frame = "final-lens", fc.FRAMES[0]
    scene, cam = fc.scene_of(rtow, case), fc.camera_of(rtow, case, frame)
    p = bc.params_of(rtow, case, frame, 12)
    ctx.upload(scene)
    want, _ = rtow.path_trace(ctx, cam, p)
    assert want.tobytes() == ctx.render(cam, p)[0].tobytes()
    assert _uncompacted(rtow, ctx, cam, p).tobytes() == want.tobytes()
    n = p.local_rows * p.width * p.spp
    perm = np.random.default_rng(7).permutation(n)
    assert _uncompacted(rtow, ctx, cam, p, perm).tobytes() == want.tobytes()
    # several launches over batches of more than 256 rays whose length is no multiple of 64
    assert n > 256 and n % 64 != 0
    for per in (1000, 300):
        ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, per)
        assert rtow.path_trace(ctx, cam, p)[0].tobytes() == want.tobytes(), per
    ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    for scale in (0.5, 2.0):
        for mode in ("lds", "cells", "global"):
            ctx.upload(scene, grid_mode=mode, grid_scale=scale)
            assert ctx.grid_scale() == scale
            assert rtow.path_trace(ctx, cam, p)[0].tobytes() == want.tobytes(), (mode, scale)


def _second_step(rtow, ctx, case):
    """The case's secondary rays: origin, direction, from, key after one step, and the seed and flags."""
    frame = fc.FRAMES[0]
    cam, p = fc.camera_of(rtow, case, frame), fc.params_of(rtow, case, frame)
    o, d, key = ctx.camera_rays(cam, p)
    got = ctx.bounce(o, d, key, p.seed, flags=p.flags)
    on = got["status"] == rtow.BOUNCE_SCATTERED
    return (got["position"][on], got["scatter"][on], got["id"][on], key[on] + np.array([0, 0, 1], np.uint32)), p


def test_invalid_rays_mid_wave_leave_their_neighbours_alone_and_outputs_are_independent(rtow, ctx):
    """Each invalid form, placed inside a wave of secondary rays, is reported
    INVALID with zeros, and every other ray keeps its bytes; any subset of the
    outputs wanted gives the bytes of all wanted."""
    ctx.upload(fc.scene_of(rtow, "final-lens"))
    (o, d, frm, key), p = _second_step(rtow, ctx, "final-lens")
    o, d, frm, key = o[:700].copy(), d[:700].copy(), frm[:700].copy(), key[:700].copy()
    assert len(o) == 700
    want = ctx.bounce(o, d, key, p.seed, frm, flags=p.flags)
    assert set(np.unique(want["status"])) >= {rtow.BOUNCE_MISS, rtow.BOUNCE_SCATTERED}
    nsph = ctx.scene.n
    forms = {70: ("o", (np.nan, 0, 0)), 71: ("o", (0, np.inf, 0)), 100: ("d", (0, 0, 0)), 101: ("d", (np.nan, 1, 0)),
             130: ("d", (1e30, 1e30, 0)), 131: ("d", (-np.inf, 0, 0)), 200: ("f", -2), 201: ("f", nsph), 202: ("f", 2 ** 31 - 1),
             300: ("k", (0, 2 ** 24, 0)), 301: ("k", (0, 0, 2 ** 24 - 1)), 302: ("k", (5, 2 ** 32 - 1, 2 ** 32 - 1))}
    o2, d2, f2, k2 = o.copy(), d.copy(), frm.copy(), key.copy()
    for i, (what, v) in forms.items():
        {"o": o2, "d": d2, "f": f2, "k": k2}[what][i] = v
    with np.errstate(all="ignore"):
        got = ctx.bounce(o2, d2, k2, p.seed, f2, flags=p.flags)
    inv = np.zeros(700, bool)
    inv[list(forms)] = True
    assert (got["status"][inv] == rtow.BOUNCE_INVALID).all() and (got["id"][inv] == -2).all()
    assert np.isinf(got["t"][inv]).all()
    for name in ("position", "normal", "scatter", "attenuation"):
        assert got[name][inv].tobytes() == bytes(12 * len(forms)), name
    _same({k: got[k][~inv] for k in OUT}, {k: want[k][~inv] for k in OUT}, "neighbours of invalid rays")
    # the largest valid key values are valid
    k3 = key.copy()
    k3[5] = (2 ** 32 - 1, 2 ** 24 - 1, 2 ** 24 - 2)
    assert ctx.bounce(o, d, k3, p.seed, frm, which=("status",), flags=p.flags)["status"][5] != rtow.BOUNCE_INVALID
    # from = None is -1 for every ray
    none = ctx.bounce(o, d, key, p.seed, None, flags=p.flags)
    _same(none, ctx.bounce(o, d, key, p.seed, np.full(700, -1, np.int32), flags=p.flags), "from NULL")
    for which in (("status",), ("scatter",), ("attenuation", "id"), ("t", "normal"), ("position", "status", "scatter")):
        sub = ctx.bounce(o, d, key, p.seed, frm, which=which, flags=p.flags)
        assert sorted(sub) == sorted(which + ("kernel_ms",))
        _same(sub, want, which, which)
    assert list(ctx.bounce(o, d, key, p.seed, frm, which=(), flags=p.flags)) == ["kernel_ms"]
    empty = ctx.bounce(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), 1)
    assert empty["status"].shape == (0,) and empty["scatter"].shape == (0, 3)


def test_the_seed_and_the_metal_flag_are_the_renders(rtow, ctx):
    """A 64-bit seed is reduced as rt_params.seed is (path_trace with such a
    seed is the render), and the async form on device tensors gives the
    synchronous form's bytes."""
    import torch
    case, frame = "five-lens-gpusem", fc.FRAMES[1]
    ctx.upload(fc.scene_of(rtow, case))
    cam = fc.camera_of(rtow, case, frame)
    p = bc.params_of(rtow, case, frame, 8)
    p.seed = 0x123456789ABCDEF0
    assert rtow.path_trace(ctx, cam, p)[0].tobytes() == ctx.render(cam, p)[0].tobytes()
    (o, d, frm, key), p = _second_step(rtow, ctx, case)
    want = ctx.bounce(o, d, key, p.seed, frm, flags=p.flags)
    n = len(o)
    dev = torch.device("cuda:0")
    ins = {"origin": torch.from_numpy(o.copy()).to(dev), "direction": torch.from_numpy(d.copy()).to(dev),
           "from": torch.from_numpy(frm.copy()).to(dev), "key": torch.from_numpy(key.view(np.int32).copy()).to(dev)}
    outs = {f: torch.full((n, 3) if ch == 3 else (n,), 7, dtype=getattr(torch, np.dtype(dt).name), device=dev)
            for f, dt, ch in rtow.BOUNCE_FIELDS}
    ptrs = {k: t.data_ptr() for k, t in list(ins.items()) + list(outs.items())}
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ctx.bounce_async(ptrs, n, p.seed, flags=p.flags, stream=stream.cuda_stream)
    stream.synchronize()
    _same({k: t.cpu().numpy() for k, t in outs.items()}, want, "async vs sync")
    ptrs["scatter"] = ptrs["key"] + 4
    with pytest.raises(rtow.RTError) as e:
        ctx.bounce_async(ptrs, n, p.seed, flags=p.flags, stream=stream.cuda_stream)
    assert e.value.status == rtow.RT_ERR_INVALID


# ---- 5. nothing else moves -----------------------------------------------------------
def test_a_pass_leaves_renders_traces_segments_and_counters_alone(rtow, ctx):
    case, frame = "final-lens", fc.FRAMES[0]
    scene, cam, p = fc.scene_of(rtow, case), fc.camera_of(rtow, case, frame), fc.params_of(rtow, case, frame)
    ctx.upload(scene)
    (o, d, frm, key), _ = _second_step(rtow, ctx, case)
    ctx.upload(scene)  # a fresh scene state
    ctx.reset_stats()
    img0, st0 = ctx.render(cam, p)
    tr0 = ctx.trace(o, d, flags=p.flags)
    sg0 = ctx.segment(o, d, 2.0, flags=p.flags)
    before = ctx.collect_stats().segments
    ctx.camera_rays(cam, p)
    ctx.bounce(o, d, key, p.seed, frm, flags=p.flags)
    assert ctx.collect_stats().segments == before == st0.segments
    img1, st1 = ctx.render(cam, p)
    tr1 = ctx.trace(o, d, flags=p.flags)
    sg1 = ctx.segment(o, d, 2.0, flags=p.flags)
    assert img1.tobytes() == img0.tobytes() and st1.segments == st0.segments
    for k in ("id", "t", "position", "normal"):
        assert tr0[k].tobytes() == tr1[k].tobytes() and sg0[k].tobytes() == sg1[k].tobytes(), k
    assert sg0["blocked"].tobytes() == sg1["blocked"].tobytes()


def test_bounce_error_paths_on_the_device(rtow):
    L = rtow.bounce_lib()
    o, d, k = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32), np.zeros((4, 3), np.uint32)
    cam, p = rtow.camera_cpu(aspect=2.0), rtow.make_params(4, 2, 1)
    with rtow.Context(0) as c:
        with pytest.raises(rtow.RTError) as e:
            c.bounce(o, d, k, 0)
        assert e.value.status == rtow.RT_ERR_NO_SCENE
        with pytest.raises(rtow.RTError) as e:
            c.camera_rays(cam, p)
        assert e.value.status == rtow.RT_ERR_NO_SCENE
        c.upload(rtow.five_scene())
        # n = 0, or every output NULL: RT_OK, nothing launched (the pointers are never read)
        rays, outs = rtow.BounceRays(n=0), rtow.BounceOut()
        assert L.rt_bounce(c._h, ctypes.byref(rays), ctypes.byref(outs), 0, None) == 0
        assert L.rt_bounce_async(c._h, ctypes.byref(rays), ctypes.byref(outs), 0, None) == 0
        rays = rtow.BounceRays(n=4, origin=o.ctypes.data, direction=d.ctypes.data, key=k.ctypes.data)
        assert L.rt_bounce(c._h, ctypes.byref(rays), ctypes.byref(outs), 0, None) == 0
        assert L.rt_bounce_async(c._h, ctypes.byref(rays), ctypes.byref(outs), 0, None) == 0
        assert c.camera_rays(cam, p, samples=0)[0].shape == (0, 3)
