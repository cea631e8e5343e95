"""The wavefront loop's device step on the GPU (include/rt_paths.h,
rt_paths_step / Context.paths_step, rtow.path_trace_device): synthetic steps
against tests/paths_ref.py at the tile's and the scan block's edges, the
deposits, subsets and the asynchronous form, the whole loop against rt_render
and rtow.path_trace, its independence of the rays' order, and the passes next
to it.  Every comparison is byte equality."""
import ctypes

import numpy as np
import pytest

import bounce_cases as bc
import features_cases as fc
import paths_ref

pytestmark = pytest.mark.gpu

PATTERNS = ("all", "none", "alternate", "last", "first", "mix")
FILL = 0xA5  # the byte the output buffers hold before a step


@pytest.fixture
def ctx(rtow, gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)


def _edges(rtow):
    L = rtow.paths_lib()
    return L.rt_paths_tile(), L.rt_paths_scan_block()


def _raw_step(rtow, ctx, d, sums, shift, want=paths_ref.NEXT):
    """rt_paths_step on host arrays whose outputs are pre-filled with FILL -> (full-length outputs, count)."""
    n = len(d["status"])
    a = rtow.PathsIn(n=n, shift=shift, n_slots=0 if sums is None else len(sums))
    keep = {k: np.ascontiguousarray(d[k]) for k, _, _ in rtow.PATHS_INPUTS}
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    o = rtow.PathsOut()
    out = {}
    for name, dt, ch in rtow.PATHS_NEXT:
        if name in want:
            out[name] = np.frombuffer(bytes([FILL]) * (n * ch * 4), dt).reshape((n, 3) if ch == 3 else (n,)).copy()
            setattr(o, "from_" if name == "from" else name, out[name].ctypes.data)
    count = np.full(1, 0xFFFFFFFF, np.uint32)
    o.count = count.ctypes.data
    if sums is not None:
        o.sums = sums.ctypes.data
    rtow.check(rtow.paths_lib().rt_paths_step(ctx._h, ctypes.byref(a), ctypes.byref(o), None), "rt_paths_step")
    return out, int(count[0])


def _check_step(rtow, ctx, d, n_slots, shift, what):
    sums = np.arange(3 * n_slots, dtype=np.uint32).reshape(n_slots, 3) * np.uint32(1000003)
    want_sums = sums.copy()
    want, want_count = paths_ref.step(d["status"], d["id"], d["position"], d["scatter"], d["attenuation"], d["key"],
                                      d["throughput"], d["slot"], want_sums, shift)
    got, count = _raw_step(rtow, ctx, d, sums, shift)
    assert count == want_count, (what, count, want_count)
    for name in paths_ref.NEXT:
        g, w = got[name], want[name]
        assert g[:count].tobytes() == w.tobytes(), (what, name, np.nonzero((g[:count] != w).reshape(count, -1).any(1))[0][:8])
        assert (g[count:].view(np.uint8) == FILL).all(), (what, name, "the tail was written")
    assert sums.tobytes() == want_sums.tobytes(), what
    return count


# ---- 1. synthetic steps ------------------------------------------------------------
def _sizes(rtow):
    T, B = _edges(rtow)
    return [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, (B + 1) * T + 5]


@pytest.mark.parametrize("which", range(9))
def test_a_step_is_the_restatement_at_every_edge(rtow, ctx, which):
    """n at the wave's, the tile's and the scan block's edges (the last: more
    tiles than the scan block has threads, and a ragged last tile), under every
    status pattern: count, every field of the next batch up to count, the
    untouched tail beyond it, and the sums."""
    n = _sizes(rtow)[which]
    T, B = _edges(rtow)
    assert _sizes(rtow)[-1] > B * T and _sizes(rtow)[-1] % T
    seen = set()
    for pattern in PATTERNS:
        d = paths_ref.synthetic(n, pattern, seed=which)
        seen.add(_check_step(rtow, ctx, d, 37, 25, (n, pattern)))
    assert 0 in seen and n in seen


# ---- 2. deposits -------------------------------------------------------------------
def test_deposits_under_contention_out_of_range_slots_and_the_clamp(rtow, ctx):
    T, _ = _edges(rtow)
    n, f32 = 2 * T + 1, np.float32
    # every ray misses into ONE slot
    d = paths_ref.synthetic(n, "none", seed=5)
    d["status"][:] = 0
    d["slot"][:] = 2
    sums = np.zeros((4, 3), np.uint32)
    got, count = _raw_step(rtow, ctx, d, sums, 31)
    want = paths_ref.fixed(d["throughput"] * d["attenuation"], 31).astype(np.uint64).sum(0) % 2 ** 32
    assert count == 0 and (sums[2] == want).all() and not sums[[0, 1, 3]].any()
    assert want.astype(np.uint64).tolist() != paths_ref.fixed(d["throughput"] * d["attenuation"], 31).astype(np.uint64).sum(0).tolist()  # it wrapped
    # a random slot map, slots >= n_slots among them: ignored, the neighbours unchanged
    d = paths_ref.synthetic(n, "mix", seed=6, n_slots=90)
    assert ((d["slot"] >= 61) & (d["status"] == 0)).any()
    _check_step(rtow, ctx, d, 61, 20, "random slots")
    block = np.full((63, 3), 0xA5A5A5A5, np.uint32)  # the sums are its middle 61 rows
    want = block.copy()
    paths_ref.step(*(d[k] for k, _, _ in rtow.PATHS_INPUTS), want[1:62], 20)
    _raw_step(rtow, ctx, d, block[1:62], 20)
    assert block.tobytes() == want.tobytes()
    # a NaN, a negative, an infinite and a huge throughput; accumulated over two calls, not cleared
    thr = np.array([[np.nan, -1.0, 0.5], [np.inf, 3e10, -np.inf], [1.0, 2.0 ** -31, 0.75]], f32)
    d = paths_ref.synthetic(3, "none", seed=7)
    d["status"][:], d["slot"][:], d["throughput"], d["attenuation"] = 0, [0, 1, 1], thr, np.ones((3, 3), f32)
    sums = np.zeros((2, 3), np.uint32)
    _raw_step(rtow, ctx, d, sums, 31)
    assert sums.tolist() == [[0, 0, 2 ** 30], [(4294967040 + 2 ** 31) % 2 ** 32, 4294967040 + 1, 3 * 2 ** 29]]
    once = sums.copy()
    _raw_step(rtow, ctx, d, sums, 31)
    assert (sums == once + once).all()  # (uint32: modulo 2^32)
    want = np.zeros((2, 3), np.uint32)
    paths_ref.step(*(d[k] for k, _, _ in rtow.PATHS_INPUTS), want, 31)
    assert (want == once).all()


# ---- 3. aliasing and subsets ---------------------------------------------------------
def test_subsets_null_sums_the_async_form_and_the_empty_batch(rtow, ctx):
    import torch
    T, _ = _edges(rtow)
    n, n_slots, shift = 3 * T + 17, 37, 25
    d = paths_ref.synthetic(n, "mix", seed=9)
    full, count = _raw_step(rtow, ctx, d, np.zeros((n_slots, 3), np.uint32), shift)
    bounced = {k: d[k] for k in ("status", "id", "position", "scatter", "attenuation")}
    # Context.paths_step: trimmed to count, sums added in place, None = no deposit
    sums = np.zeros((n_slots, 3), np.uint32)
    got = ctx.paths_step(bounced, d["key"], d["throughput"], d["slot"], sums, shift)
    want_sums = np.zeros((n_slots, 3), np.uint32)
    want, _ = paths_ref.step(*(d[k] for k, _, _ in rtow.PATHS_INPUTS), want_sums, shift)
    assert got["count"] == count and (sums == want_sums).all() and sums.any()
    for name in paths_ref.NEXT:
        assert got[name].tobytes() == want[name].tobytes() == full[name][:count].tobytes(), name
    for which in (("origin",), ("slot", "key"), ("from", "throughput", "direction"), ()):
        sub = ctx.paths_step(bounced, d["key"], d["throughput"], d["slot"], None, shift, which=which)
        assert sorted(sub) == sorted(which + ("count", "kernel_ms")) and sub["count"] == count
        for name in which:
            assert sub[name].tobytes() == want[name].tobytes(), (which, name)
    # the async form on torch tensors with caller scratch; origin, direction and from land in the arrays the
    # bounce read (not inputs of the step)
    dev = torch.device("cuda:0")
    as_i32 = lambda a: a.view(np.int32) if a.dtype == np.uint32 else a  # noqa: E731
    t = {k: torch.from_numpy(as_i32(np.ascontiguousarray(d[k])).copy()).to(dev) for k, _, _ in rtow.PATHS_INPUTS}
    bounce_in = {"origin": torch.full((n, 3), 7.0, device=dev), "direction": torch.full((n, 3), 7.0, device=dev),
                 "from": torch.full((n,), 7, dtype=torch.int32, device=dev)}
    nxt = {"key": torch.full((n, 3), 7, dtype=torch.int32, device=dev), "throughput": torch.full((n, 3), 7.0, device=dev),
           "slot": torch.full((n,), 7, dtype=torch.int32, device=dev)}
    dsums = torch.zeros((n_slots, 3), dtype=torch.int32, device=dev)
    dcount = torch.full((1,), -1, dtype=torch.int32, device=dev)
    scratch = torch.zeros(rtow.paths_scratch_bytes(n), dtype=torch.uint8, device=dev)
    assert scratch.data_ptr() % 16 == 0
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    ptrs.update({"out_" + k: v.data_ptr() for k, v in list(bounce_in.items()) + list(nxt.items())})
    ptrs.update(sums=dsums.data_ptr(), count=dcount.data_ptr())
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    for _ in range(2):  # the second call adds again
        ctx.paths_step_async(ptrs, n, n_slots, shift, scratch.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert int(dcount.item()) == count
    for name, buf in list(bounce_in.items()) + list(nxt.items()):
        g = buf.cpu().numpy()
        assert g[:count].tobytes() == want[name].tobytes(), name
        assert (g[count:] == 7).all(), name
    assert (dsums.cpu().numpy().view(np.uint32) == want_sums + want_sums).all()
    dframe = torch.zeros((n_slots, 3), device=dev)
    ctx.paths_frame_async(dsums.data_ptr(), n_slots, shift, dframe.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert dframe.cpu().numpy().tobytes() == paths_ref.frame(want_sums + want_sums, shift).tobytes()
    assert ctx.paths_frame(want_sums, shift).tobytes() == paths_ref.frame(want_sums, shift).tobytes()
    top = np.array([[2 ** 32 - 1, 2 ** 31, 1]], np.uint32)
    assert ctx.paths_frame(top, 0).tobytes() == paths_ref.frame(top, 0).tobytes()
    # a forbidden overlap is refused on the device pointers too
    with pytest.raises(rtow.RTError) as e:
        ctx.paths_step_async(dict(ptrs, out_key=ptrs["key"]), n, n_slots, shift, scratch.data_ptr(), stream.cuda_stream)
    assert e.value.status == rtow.RT_ERR_INVALID
    # n = 0: count is set to 0 and nothing else happens
    dcount.fill_(-1)
    ctx.paths_step_async(ptrs, 0, n_slots, shift, scratch.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert int(dcount.item()) == 0 and (dsums.cpu().numpy().view(np.uint32) == want_sums + want_sums).all()
    empty = paths_ref.synthetic(0, "mix")
    got = ctx.paths_step({k: empty[k] for k in bounced}, empty["key"], empty["throughput"], empty["slot"], sums, shift)
    assert got["count"] == 0 and got["origin"].shape == (0, 3) and (sums == want_sums).all()


# ---- 4. the loop ---------------------------------------------------------------------
def test_the_excluded_cases_are_the_ones_path_trace_refuses(rtow, ctx):
    assert len(bc.RENDER_CASES) == 20
    for case in fc.CASES:
        ctx.upload(fc.scene_of(rtow, case))
        frame = fc.frames_of(case)[0]
        cam, p = fc.camera_of(rtow, case, frame), bc.params_of(rtow, case, frame, 1)
        refused = []
        for fn in (rtow.path_trace, rtow.path_trace_device):
            try:
                fn(ctx, cam, p)
                refused.append(False)
            except ValueError:
                refused.append(True)
        assert refused == [case not in bc.RENDER_CASES] * 2, (case, refused)


@pytest.mark.parametrize("case", bc.RENDER_CASES)
def test_the_device_loop_is_the_render_and_path_trace(rtow, ctx, case):
    """rtow.path_trace_device gives rt_render's bytes and rtow.path_trace's,
    and traces as many rays as the render counts segments: every frame of the
    case at max_depth 50, the context's default walk."""
    ctx.upload(fc.scene_of(rtow, case))
    for frame in fc.frames_of(case):
        cam, p = fc.camera_of(rtow, case, frame), bc.params_of(rtow, case, frame, 50)
        got, traced = rtow.path_trace_device(ctx, cam, p)
        img, st = ctx.render(cam, p)
        assert got.dtype == img.dtype and got.shape == img.shape
        bad = np.nonzero(got.view(np.uint32) != img.view(np.uint32))
        assert got.tobytes() == img.tobytes(), (case, frame, len(bad[0]), [b[:4].tolist() for b in bad])
        assert traced == st.segments, (case, frame, traced, st.segments)
        host, host_traced = rtow.path_trace(ctx, cam, p)
        assert host.tobytes() == got.tobytes() and host_traced == traced, (case, frame)


def test_the_device_loop_at_other_depths_chunks_and_on_a_banded_frame(rtow, ctx):
    case, frame = "final-pinhole-gpusem", fc.FRAMES[0]
    ctx.upload(fc.scene_of(rtow, case))
    cam = fc.camera_of(rtow, case, frame)
    for depth, chunk in ((3, 4), (50, 1), (50, 5), (50, 7), (50, 64)):
        p = bc.params_of(rtow, case, frame, depth)
        assert p.spp == 16
        img, st = ctx.render(cam, p)
        got, traced = rtow.path_trace_device(ctx, cam, p, chunk_spp=chunk)
        assert got.tobytes() == img.tobytes() and traced == st.segments, (depth, chunk)
    case = "final-bands"
    ctx.upload(fc.scene_of(rtow, case))
    cam, p = fc.camera_of(rtow, case, frame), bc.params_of(rtow, case, frame, 50)
    assert (rtow.local_to_global_rows(p) >= p.height).any()  # padding rows
    img, st = ctx.render(cam, p)
    for chunk in (4, 2):
        got, traced = rtow.path_trace_device(ctx, cam, p, chunk_spp=chunk)
        assert got.tobytes() == img.tobytes() and traced == st.segments, chunk


# ---- 5. order independence and stability -------------------------------------------------
def _host_loop(rtow, ctx, cam, p, order=None):
    """The loop over Context.bounce and Context.paths_step with the camera
    batch in `order`; every step's next batch is also compared with the numpy
    restatement's, in its order."""
    o, d, key = ctx.camera_rays(cam, p)
    n = len(o)
    order = np.arange(n) if order is None else order
    o, d, key = o[order], d[order], key[order]
    slot = (order // p.spp).astype(np.uint32)
    frm, thr = np.full(n, -1, np.int32), np.ones((n, 3), np.float32)
    shift = rtow.paths_shift(p.spp)
    sums = np.zeros((p.local_rows * p.width, 3), np.uint32)
    ref_sums = sums.copy()
    for _ in range(p.max_depth):
        if not len(o):
            break
        got = ctx.bounce(o, d, key, p.seed, frm, ("status", "id", "position", "scatter", "attenuation"), p.flags)
        want, count = paths_ref.step(got["status"], got["id"], got["position"], got["scatter"], got["attenuation"], key,
                                     thr, slot, ref_sums, shift)
        nxt = ctx.paths_step(got, key, thr, slot, sums, shift)
        assert nxt["count"] == count
        for name in paths_ref.NEXT:
            assert nxt[name].tobytes() == want[name].tobytes(), name
        o, d, frm, key, thr, slot = (nxt[k] for k in paths_ref.NEXT)
    assert (sums == ref_sums).all()
    return ctx.paths_frame(sums, shift).reshape(p.local_rows, p.width, 3)


def test_the_image_does_not_depend_on_the_rays_order_and_the_compaction_is_stable(rtow, ctx):
    case, frame = "final-lens", fc.FRAMES[0]
    ctx.upload(fc.scene_of(rtow, case))
    cam, p = fc.camera_of(rtow, case, frame), bc.params_of(rtow, case, frame, 12)
    want, _ = rtow.path_trace_device(ctx, cam, p)
    assert want.tobytes() == ctx.render(cam, p)[0].tobytes()
    assert _host_loop(rtow, ctx, cam, p).tobytes() == want.tobytes()
    n = p.local_rows * p.width * p.spp
    T, _ = _edges(rtow)
    assert n > 4 * T
    perm = np.random.default_rng(11).permutation(n)
    assert _host_loop(rtow, ctx, cam, p, perm).tobytes() == want.tobytes()


# ---- 6. neighbours -------------------------------------------------------------------------
def test_a_step_leaves_renders_bounces_traces_and_counters_alone(rtow, ctx):
    case, frame = "final-lens", fc.FRAMES[0]
    scene, cam, p = fc.scene_of(rtow, case), fc.camera_of(rtow, case, frame), fc.params_of(rtow, case, frame)
    ctx.upload(scene)
    o, d, key = ctx.camera_rays(cam, p)
    ctx.reset_stats()
    img0, st0 = ctx.render(cam, p)
    b0 = ctx.bounce(o, d, key, p.seed, flags=p.flags)
    tr0 = ctx.trace(o, d, flags=p.flags)
    before = ctx.collect_stats().segments
    n = len(o)
    sums = np.zeros((p.local_rows * p.width, 3), np.uint32)
    nxt = ctx.paths_step(b0, key, np.ones((n, 3), np.float32), (np.arange(n) // p.spp).astype(np.uint32), sums,
                         rtow.paths_shift(p.spp))
    assert 0 < nxt["count"] < n and sums.any()
    ctx.paths_frame(sums, rtow.paths_shift(p.spp))
    assert ctx.collect_stats().segments == before == st0.segments
    img1, st1 = ctx.render(cam, p)
    b1 = ctx.bounce(o, d, key, p.seed, flags=p.flags)
    tr1 = ctx.trace(o, d, flags=p.flags)
    assert img1.tobytes() == img0.tobytes() and st1.segments == st0.segments
    for k in ("status", "id", "t", "position", "normal", "scatter", "attenuation"):
        assert b0[k].tobytes() == b1[k].tobytes(), k
    for k in ("id", "t", "position", "normal"):
        assert tr0[k].tobytes() == tr1[k].tobytes(), k


def test_paths_need_no_scene(rtow):
    """The pass reads no scene: a fresh context without an upload runs it."""
    d = paths_ref.synthetic(100, "mix", seed=1)
    with rtow.Context(0) as c:
        sums = np.zeros((37, 3), np.uint32)
        got = c.paths_step({k: d[k] for k in ("status", "id", "position", "scatter", "attenuation")}, d["key"],
                           d["throughput"], d["slot"], sums, 25)
        want_sums = np.zeros((37, 3), np.uint32)
        want, count = paths_ref.step(*(d[k] for k, _, _ in rtow.PATHS_INPUTS), want_sums, 25)
        assert got["count"] == count and got["key"].tobytes() == want["key"].tobytes() and (sums == want_sums).all()
