"""The clamped temporal resolve on the GPU (include/rt_resolve.h, rt_resolve /
Context.resolve): the kernel gives the bits of the numpy restatement
(tests/resolve_ref.py) on synthetic frames that reach every branch and on
consecutive frames of a real orbit; the identity properties of test_resolve.py
hold on the device; the asynchronous and the out = NULL paths agree with the
synchronous one and out == cur is rejected where the header says so; histories
pass between rt_temporal and rt_resolve; the pass leaves the context's renders
alone; and on the 8-frame orbits of test_temporal_gpu.py the accumulated frame
beats its denoised input, and rt_temporal with a history of the same length."""
import ctypes

import numpy as np
import pytest

import resolve_ref as ref
import temporal_ref as tref
from test_resolve import (OFF, SPP, check_clamp, check_flat_neighbourhood, check_partial_restarts,
                          check_running_mean)
from test_temporal_gpu import _mse, orbit_cameras, orbit_sequence, same_bits

pytestmark = pytest.mark.gpu

# test_temporal_gpu.py's frames, and 17x33: a tile edge in both directions with a partly filled wave
FRAMES = ((67, 37), (5, 3), (1, 1), (2, 2), (64, 64), (17, 33))
OPTIONS = {
    "defaults": {},
    "all_off": OFF,
    "max_len_1": dict(max_len=1),
    "max_len_32": dict(max_len=32),
    "gamma_half": dict(gamma=0.5),
    "keep_partial": dict(flags=ref.KEEP_PARTIAL),
    "loose_plane": dict(plane_tol=1e-2),
    "tight_plane": dict(plane_tol=1e-4),
}

_inputs = {}


def inputs(w, h):
    """The seeded frame, history, view and rays of that size, made once and never written to."""
    if (w, h) not in _inputs:
        frame, hist, view, rays = ref.synthetic_inputs(w, h, SPP, seed=1000 * w + h)
        for a in list(frame.values()) + [hist]:
            a.setflags(write=False)
        _inputs[(w, h)] = frame, hist, view, rays
    return _inputs[(w, h)]


def device_step(ctx):
    """Context.resolve with resolve_ref's signature."""
    def step(cur, hits, depth, normal, spp, rays, prev=None, history=None, **options):
        return ctx.resolve(cur, dict(hits=hits, depth=depth, normal=normal), spp, prev, rays, history, **options)
    return step


@pytest.mark.parametrize("options", list(OPTIONS), ids=list(OPTIONS))
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
def test_resolve_equals_the_restatement_bit_for_bit(gpu_ctx, frame, options):
    """The synthetic inputs (test_resolve_synthetic_inputs_reach_every_branch
    shows what they reach), with a history and without."""
    w, h = frame
    f, hist, view, rays = inputs(w, h)
    opt = OPTIONS[options]
    for prev, history in ((view, hist), (None, None)):
        out, hout = gpu_ctx.resolve(f["cur"], f, SPP, prev, rays, history, **opt)
        want_out, want_hist = ref.resolve_ref(spp=SPP, rays=rays, prev=prev, history=history,
                                              **{**ref.DEFAULTS, **opt}, **f)
        assert np.isfinite(want_out).all() and np.isfinite(want_hist).all()
        same_bits(out, want_out)
        same_bits(hout, want_hist)


@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_resolve_equals_the_restatement_on_an_orbit(rtow, gpu_ctx, scene_name):
    """Three consecutive frames of a 2-degree-per-frame orbit at 67x37 and 4
    spp, each frame's history_out the next frame's history_in.  So that the
    comparison is not one of restarts only, at least a tenth of the fully
    covered pixels (some 150 of them) must have gathered history in the later
    frames; at 4 spp and this size the mean depth is noisy, and the plane test
    turns many away."""
    w, h = 67, 37
    gpu_ctx.upload(rtow.final_scene() if scene_name == "final" else rtow.five_scene())
    hist = view = None
    for i, cam in enumerate(orbit_cameras(rtow, scene_name, w, h, 3, 2.0)):
        p = rtow.make_params(w, h, SPP, seed=1 + i, flags=rtow.RT_FLAG_ACCEL_BVH)
        cur, g = gpu_ctx.render(cam, p)[0], gpu_ctx.aov(cam, p)
        rays = rtow.resolve_rays(cam, w, h)
        out, hout = gpu_ctx.resolve(cur, g, SPP, view, rays, hist)
        want_out, want_hist = ref.resolve_ref(cur, g["hits"], g["depth"], g["normal"], SPP, rays, view, hist)
        same_bits(out, want_out)
        same_bits(hout, want_hist)
        if i:
            full = g["hits"] == SPP
            share = float((hout[0, ..., 3][full] > 1).mean())
            print(f"orbit {scene_name}, frame {i}: {share:.3f} of the fully covered pixels found history")
            assert share > 0.1
        hist, view = hout, rtow.temporal_view(cam, w, h)


@pytest.mark.parametrize("max_len", [1, 3, 32])
def test_resolve_running_mean_on_the_device(gpu_ctx, max_len):
    check_running_mean(device_step(gpu_ctx), max_len)


def test_resolve_partial_pixels_on_the_device(gpu_ctx):
    check_partial_restarts(device_step(gpu_ctx))


def test_resolve_flat_neighbourhood_on_the_device(gpu_ctx):
    check_flat_neighbourhood(device_step(gpu_ctx))


def test_resolve_clamp_on_the_device(gpu_ctx):
    check_clamp(device_step(gpu_ctx))


def test_resolve_struct_zero_means_default(rtow, gpu_ctx):
    """Options left out (the struct's zeros) are the documented defaults."""
    f, hist, view, rays = inputs(67, 37)
    a = gpu_ctx.resolve(f["cur"], f, SPP, view, rays, hist)
    b = gpu_ctx.resolve(f["cur"], f, SPP, view, rays, hist, **rtow.RESOLVE_DEFAULTS)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    d = rtow.resolve_desc(67, 37, SPP, view, rays)
    assert (d.max_len, d.plane_tol, d.normal_cos, d.gamma, d.flags) == (0, 0.0, 0.0, 0.0, 0)


def test_resolve_async_without_out_and_in_place(rtow, gpu_ctx):
    """rt_resolve_async into caller-owned device memory on a caller's stream
    gives the synchronous call's bytes, with out a buffer of its own and with
    out = NULL (the same history), and leaves the inputs alone; out == cur is
    RT_ERR_INVALID there (the kernel reads cur's neighbourhood) and nothing is
    written; the synchronous call takes out = NULL and out == cur."""
    import torch
    w, h = FRAMES[0]
    f, hist, view, rays = inputs(w, h)
    want_out, want_hist = gpu_ctx.resolve(f["cur"], f, SPP, view, rays, hist)
    dev = torch.device("cuda:0")
    host = {**f, "hits": f["hits"].view(np.int32), "history_in": hist}
    t = {k: torch.from_numpy(np.array(a)).to(dev) for k, a in host.items()}
    out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device=dev)
    hout = torch.full((3, h, w, 4), 7.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    ptrs["history_out"] = hout.data_ptr()
    gpu_ctx.resolve_async({**ptrs, "out": out.data_ptr()}, w, h, SPP, view, rays, stream=stream.cuda_stream)
    stream.synchronize()
    assert out.cpu().numpy().tobytes() == want_out.tobytes()
    assert hout.cpu().numpy().tobytes() == want_hist.tobytes()
    for k, a in host.items():
        assert t[k].cpu().numpy().tobytes() == a.tobytes(), k
    hout.fill_(7.0)
    torch.cuda.current_stream(dev).synchronize()
    gpu_ctx.resolve_async(ptrs, w, h, SPP, view, rays, stream=stream.cuda_stream)  # out = NULL
    stream.synchronize()
    assert hout.cpu().numpy().tobytes() == want_hist.tobytes()
    hout.fill_(7.0)
    torch.cuda.current_stream(dev).synchronize()
    with pytest.raises(rtow.RTError):
        gpu_ctx.resolve_async({**ptrs, "out": ptrs["cur"]}, w, h, SPP, view, rays, stream=stream.cuda_stream)
    stream.synchronize()
    assert t["cur"].cpu().numpy().tobytes() == f["cur"].tobytes()
    assert (hout.cpu().numpy() == 7.0).all()
    # the synchronous call with out = NULL and with out == cur
    d = rtow.resolve_desc(w, h, SPP, view, rays)
    cur = np.array(f["cur"])
    h2 = np.zeros_like(want_hist)
    d.cur, d.hits, d.depth, d.normal = (a.ctypes.data for a in (cur, f["hits"], f["depth"], f["normal"]))
    d.history_in, d.history_out = hist.ctypes.data, h2.ctypes.data
    assert rtow.resolve_lib().rt_resolve(gpu_ctx._h, ctypes.byref(d), None) == 0
    assert h2.tobytes() == want_hist.tobytes() and cur.tobytes() == f["cur"].tobytes()
    d.out = cur.ctypes.data
    h2[:] = 0
    assert rtow.resolve_lib().rt_resolve(gpu_ctx._h, ctypes.byref(d), None) == 0
    assert cur.tobytes() == want_out.tobytes() and h2.tobytes() == want_hist.tobytes()


def test_histories_pass_between_temporal_and_resolve(rtow, gpu_ctx):
    """Four consecutive orbit frames of the five-sphere scene (67x37, 4 spp)
    through temporal, resolve, temporal, resolve, each fed the other's
    history: the device gives the restatements' bits at every step, and both
    passes do use what the other wrote."""
    w, h = 67, 37
    gpu_ctx.upload(rtow.five_scene())
    hist = want_hist = view = None
    for i, cam in enumerate(orbit_cameras(rtow, "five", w, h, 4, 2.0)):
        p = rtow.make_params(w, h, SPP, seed=1 + i, flags=rtow.RT_FLAG_ACCEL_BVH)
        cur, g = gpu_ctx.render(cam, p)[0], gpu_ctx.aov(cam, p)
        if i % 2 == 0:
            out, hist = gpu_ctx.temporal(cur, g, SPP, view, hist, max_len=8)
            want_out, want_hist = tref.temporal_ref(cur, g["hits"], g["position"], g["normal"], SPP, view, want_hist,
                                                    max_len=8)
        else:
            rays = rtow.resolve_rays(cam, w, h)
            out, hist = gpu_ctx.resolve(cur, g, SPP, view, rays, hist, max_len=8)
            want_out, want_hist = ref.resolve_ref(cur, g["hits"], g["depth"], g["normal"], SPP, rays, view, want_hist,
                                                  max_len=8)
        same_bits(out, want_out)
        same_bits(hist, want_hist)
        if i:
            full = g["hits"] == SPP
            share = float((hist[0, ..., 3][full] > 1).mean())
            print(f"mixed chain, frame {i} ({'resolve' if i % 2 else 'temporal'}): {share:.3f} of the fully covered "
                  "pixels found the other pass's history")
            assert share > 0.1  # (not a chain of restarts: as in the orbit test above)
        view = rtow.temporal_view(cam, w, h)
    # some history went through two hand-overs at least; four frames give a length of 4, up to the rounding of
    # three weighted means (each below 8 * 2^-24 relative: two products, two sums and a division per tap pair)
    assert 2.0 < hist[0, ..., 3].max() <= 4.0 * (1 + 24 * 2.0 ** -24)


def test_resolve_between_renders_leaves_them_alone(rtow, gpu_ctx):
    """A render before the pass and a render after it give the same bytes, and
    the pass needs no scene of its own."""
    gpu_ctx.upload(rtow.final_scene())
    cam = rtow.camera_cpu(aspect=64 / 36)
    p = rtow.make_params(64, 36, 5, seed=2024, flags=rtow.RT_FLAG_ACCEL_BVH)
    a, sa = gpu_ctx.render(cam, p)
    g = gpu_ctx.aov(cam, p)
    rays = rtow.resolve_rays(cam, 64, 36)
    _, hist = gpu_ctx.resolve(a, g, 5, now_rays=rays)
    gpu_ctx.resolve(a, g, 5, rtow.temporal_view(cam, 64, 36), rays, hist)
    b, sb = gpu_ctx.render(cam, p)
    assert a.tobytes() == b.tobytes() and sa.segments == sb.segments
    f, fh, view, srays = inputs(67, 37)
    with rtow.Context(0) as fresh:  # no rt_scene_upload
        c = fresh.resolve(f["cur"], f, SPP, view, srays, fh)
    d = gpu_ctx.resolve(f["cur"], f, SPP, view, srays, fh)
    assert c[0].tobytes() == d[0].tobytes() and c[1].tobytes() == d[1].tobytes()


def accumulate(rtow, ctx, seq, cams, which, spp=16, **options):
    hist = view = out = None
    for (den, g, v), cam in zip(seq, cams):
        if which == "resolve":
            out, hist = ctx.resolve(den, g, spp, view, rtow.resolve_rays(cam, den.shape[1], den.shape[0]), hist,
                                    **options)
        else:
            out, hist = ctx.temporal(den, g, spp, view, hist, **options)
        view = v
    return out


@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_resolve_lowers_the_error_and_beats_temporal_at_the_same_length(rtow, gpu_ctx, scene_name):
    """The sequences of test_temporal_lowers_the_error_of_the_denoised_frame
    (128x72, 16 spp, 8-frame orbit at 1 degree per frame, seeds 1..8, every
    frame denoised; truth: the 4096-spp render of the last camera, seed 99; MSE
    on sqrt(mean) clamped to [0, 1]), built once per scene and fed to both
    passes.  (a) rt_resolve at its defaults: accumulated < denoised input.
    (b) both passes at max_len = 8, otherwise at their own defaults:
    rt_resolve's error < rt_temporal's.  DESIGN.md 12 records the figures.

    Measured on the MI355X at the tuned defaults (max_len 2, plane_tol 0.003,
    gamma 1): (a) final 6.862e-4 -> 5.586e-4, five 2.685e-4 -> 2.172e-4
    (rt_temporal at its defaults: 6.410e-4, 2.096e-4); (b) final 6.995e-4 <
    8.798e-4, five 2.950e-4 < 3.067e-4.  With a plane_tol of 0.03, the best
    choice for max_len 2 alone, (b) fails on the final scene (9.832e-4): the
    default is the value that does best over max_len 2, 4 and 8 together."""
    seq, truth = orbit_sequence(rtow, gpu_ctx, scene_name)
    cams = orbit_cameras(rtow, scene_name, 128, 72, 8, 1.0)
    mden = _mse(seq[-1][0], 16, truth)
    m_def = _mse(accumulate(rtow, gpu_ctx, seq, cams, "resolve"), 16, truth)
    m_res8 = _mse(accumulate(rtow, gpu_ctx, seq, cams, "resolve", max_len=8), 16, truth)
    m_tmp8 = _mse(accumulate(rtow, gpu_ctx, seq, cams, "temporal", max_len=8), 16, truth)
    m_tmp = _mse(accumulate(rtow, gpu_ctx, seq, cams, "temporal"), 16, truth)
    print(f"resolve quality {scene_name}: mse denoised {mden:.6e}, resolve defaults {m_def:.6e}, "
          f"resolve max_len 8 {m_res8:.6e}, temporal max_len 8 {m_tmp8:.6e}, temporal defaults {m_tmp:.6e}")
    assert m_def < mden
    assert m_res8 < m_tmp8
