"""Temporal accumulation with reprojection on the GPU (include/rt_temporal.h,
rt_temporal / Context.temporal): the kernel gives the bits of the numpy
restatement (tests/temporal_ref.py) on synthetic frames that reach every
branch and on consecutive frames of a real orbit; the identity-view properties
of test_temporal.py hold on the device; the asynchronous, the in-place and the
out = NULL paths agree with the synchronous one; the pass leaves the context's
renders alone; and on an 8-frame orbit the accumulated frame is closer to a
4096-spp render than the denoised frame it was fed."""
import ctypes

import numpy as np
import pytest

import temporal_ref as ref
from test_temporal import OFF, SPP, check_disocclusion, check_running_mean, check_shift

pytestmark = pytest.mark.gpu

# 67x37: no multiple of the 16x16 tile, several blocks; 5x3, 2x2: smaller than
# a wave's 16x4; 1x1: the degenerate frame, whose four taps are one pixel or
# none; 64x64: whole tiles
FRAMES = ((67, 37), (5, 3), (1, 1), (2, 2), (64, 64))
OPTIONS = {
    "defaults": {},
    "tests_off": OFF,
    "max_len_1": dict(max_len=1),
    "max_len_32": dict(max_len=32),  # the history's lengths stay below the limit
    "tight_plane": dict(plane_tol=1e-4),
    "loose_plane": dict(plane_tol=0.01),
}
FIVE_VIEW = dict(lookfrom=(-2.0, 0.5, 2.0), lookat=(0.0, 0.0, -1.0), vfov=40.0, focus_dist=3.4)
FINAL_VIEW = dict(lookfrom=(13.0, 2.0, 3.0), lookat=(0.0, 0.0, 0.0), focus_dist=10.0)

_inputs = {}


def inputs(w, h):
    """The seeded frame, history and view of that size, made once and never written to."""
    if (w, h) not in _inputs:
        frame, hist, view = ref.synthetic_inputs(w, h, SPP, seed=1000 * w + h)
        for a in list(frame.values()) + [hist]:
            a.setflags(write=False)
        _inputs[(w, h)] = frame, hist, view
    return _inputs[(w, h)]


def same_bits(got, want):
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())


def device_step(ctx):
    """Context.temporal with temporal_ref's signature."""
    def step(cur, hits, position, normal, spp, prev=None, history=None, **options):
        return ctx.temporal(cur, dict(hits=hits, position=position, normal=normal), spp, prev, history, **options)
    return step


@pytest.mark.parametrize("options", list(OPTIONS), ids=list(OPTIONS))
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
def test_temporal_equals_the_restatement_bit_for_bit(gpu_ctx, frame, options):
    """(a) the synthetic inputs (test_synthetic_inputs_reach_every_branch in
    test_temporal.py shows what they reach), with a history and without."""
    w, h = frame
    f, hist, view = inputs(w, h)
    opt = OPTIONS[options]
    for prev, history in ((view, hist), (None, None)):
        out, hout = gpu_ctx.temporal(f["cur"], f, SPP, prev, history, **opt)
        want_out, want_hist = ref.temporal_ref(spp=SPP, prev=prev, history=history, **{**ref.DEFAULTS, **opt}, **f)
        assert np.isfinite(want_out).all() and np.isfinite(want_hist).all()
        same_bits(out, want_out)
        same_bits(hout, want_hist)


def orbit_cameras(rtow, scene_name, w, h, frames, degrees):
    view = FIVE_VIEW if scene_name == "five" else FINAL_VIEW
    extra = {k: v for k, v in view.items() if k not in ("lookfrom", "lookat")}
    return [rtow.camera_cpu(lookfrom=ref.orbit(view["lookfrom"], view["lookat"], degrees * i), lookat=view["lookat"],
                            aspect=w / h, aperture=0.1, **extra) for i in range(frames)]


@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_temporal_equals_the_restatement_on_an_orbit(rtow, gpu_ctx, scene_name):
    """(b) three consecutive frames of a 2-degree-per-frame orbit at 67x37 and
    4 spp, each frame's history_out the next frame's history_in; the later
    frames do find history."""
    w, h = 67, 37
    gpu_ctx.upload(rtow.final_scene() if scene_name == "final" else rtow.five_scene())
    hist = view = None
    for i, cam in enumerate(orbit_cameras(rtow, scene_name, w, h, 3, 2.0)):
        p = rtow.make_params(w, h, SPP, seed=1 + i, flags=rtow.RT_FLAG_ACCEL_BVH)
        cur, g = gpu_ctx.render(cam, p)[0], gpu_ctx.aov(cam, p)
        out, hout = gpu_ctx.temporal(cur, g, SPP, view, hist)
        want_out, want_hist = ref.temporal_ref(cur, g["hits"], g["position"], g["normal"], SPP, view, hist)
        same_bits(out, want_out)
        same_bits(hout, want_hist)
        if i:
            geo = g["hits"] > 0
            share = float((hout[0, ..., 3][geo] > 1).mean())
            print(f"orbit {scene_name}, frame {i}: {share:.3f} of the geometry pixels found history")
            assert share > 0.5
        hist, view = hout, rtow.temporal_view(cam, w, h)


@pytest.mark.parametrize("max_len", [1, 3, 32])
def test_temporal_running_mean_on_the_device(gpu_ctx, max_len):
    check_running_mean(device_step(gpu_ctx), max_len)


def test_temporal_shift_on_the_device(gpu_ctx):
    check_shift(device_step(gpu_ctx))


@pytest.mark.parametrize("kind", ["normal", "depth"])
def test_temporal_disocclusion_on_the_device(gpu_ctx, kind):
    check_disocclusion(device_step(gpu_ctx), kind)


def test_temporal_struct_zero_means_default(rtow, gpu_ctx):
    """Options left out (the struct's zeros) are the documented defaults."""
    f, hist, view = inputs(67, 37)
    a = gpu_ctx.temporal(f["cur"], f, SPP, view, hist)
    b = gpu_ctx.temporal(f["cur"], f, SPP, view, hist, **rtow.TEMPORAL_DEFAULTS)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    d = rtow.temporal_desc(67, 37, SPP, view)
    assert (d.max_len, d.plane_tol, d.normal_cos) == (0, 0.0, 0.0)


def test_temporal_async_in_place_and_without_out(rtow, gpu_ctx):
    """rt_temporal_async into caller-owned device memory on a caller's stream
    gives the synchronous call's bytes, with out a buffer of its own, with out
    aliasing cur, and with out = NULL (the same history); the inputs are left
    alone."""
    import torch
    w, h = FRAMES[0]
    f, hist, view = inputs(w, h)
    want_out, want_hist = gpu_ctx.temporal(f["cur"], f, SPP, view, hist)
    dev = torch.device("cuda:0")
    host = {**f, "hits": f["hits"].view(np.int32), "history_in": hist}
    t = {k: torch.from_numpy(np.array(a)).to(dev) for k, a in host.items()}
    out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device=dev)
    hout = torch.full((3, h, w, 4), 7.0, dtype=torch.float32, device=dev)
    assert hout.numel() * 4 == rtow.temporal_lib().rt_temporal_history_bytes(w, h)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    ptrs["history_out"] = hout.data_ptr()
    gpu_ctx.temporal_async({**ptrs, "out": out.data_ptr()}, w, h, SPP, view, stream=stream.cuda_stream)
    stream.synchronize()
    assert out.cpu().numpy().tobytes() == want_out.tobytes()
    assert hout.cpu().numpy().tobytes() == want_hist.tobytes()
    for k, a in host.items():
        assert t[k].cpu().numpy().tobytes() == a.tobytes(), k
    hout.fill_(7.0)
    torch.cuda.current_stream(dev).synchronize()
    gpu_ctx.temporal_async(ptrs, w, h, SPP, view, stream=stream.cuda_stream)  # out = NULL
    stream.synchronize()
    assert hout.cpu().numpy().tobytes() == want_hist.tobytes()
    hout.fill_(7.0)
    torch.cuda.current_stream(dev).synchronize()
    gpu_ctx.temporal_async({**ptrs, "out": ptrs["cur"]}, w, h, SPP, view, stream=stream.cuda_stream)
    stream.synchronize()
    assert t["cur"].cpu().numpy().tobytes() == want_out.tobytes()
    assert hout.cpu().numpy().tobytes() == want_hist.tobytes()
    # the synchronous call with out = NULL and with out == cur
    d = rtow.temporal_desc(w, h, SPP, view)
    cur = np.array(f["cur"])
    h2 = np.zeros_like(want_hist)
    d.cur, d.hits, d.position, d.normal = (a.ctypes.data for a in (cur, f["hits"], f["position"], f["normal"]))
    d.history_in, d.history_out = hist.ctypes.data, h2.ctypes.data
    assert rtow.temporal_lib().rt_temporal(gpu_ctx._h, ctypes.byref(d), None) == 0
    assert h2.tobytes() == want_hist.tobytes() and cur.tobytes() == f["cur"].tobytes()
    d.out = cur.ctypes.data
    assert rtow.temporal_lib().rt_temporal(gpu_ctx._h, ctypes.byref(d), None) == 0
    assert cur.tobytes() == want_out.tobytes()


def test_async_chain_of_all_passes_equals_the_synchronous_chain(rtow, gpu_ctx):
    """render -> aov -> denoise -> temporal of two consecutive orbit frames of
    the five-sphere scene (67x37, 4 spp), enqueued on one caller stream into
    torch device buffers, the second frame's history the first one's: the bytes
    of the same chain through the synchronous Context.aov / denoise / temporal,
    whose staging uploads and downloads every buffer in between."""
    import torch
    w, h = 67, 37
    gpu_ctx.upload(rtow.five_scene())
    cams = orbit_cameras(rtow, "five", w, h, 2, 2.0)
    frames = [(cam, rtow.make_params(w, h, SPP, seed=1 + i, flags=rtow.RT_FLAG_ACCEL_BVH), rtow.temporal_view(cam, w, h))
              for i, cam in enumerate(cams)]
    want = []
    hist = prev = None
    for cam, p, view in frames:
        g = gpu_ctx.aov(cam, p)
        den = gpu_ctx.denoise(gpu_ctx.render(cam, p)[0], g, SPP)
        out, hist = gpu_ctx.temporal(den, g, SPP, prev, hist)
        want.append((den, out, hist))
        prev = view
    dev = torch.device("cuda:0")

    def buf(*shape, dtype=torch.float32):
        return torch.full(shape, 7, dtype=dtype, device=dev)
    t = dict(beauty=buf(h, w, 3), hits=buf(h, w, dtype=torch.int32), position=buf(h, w, 3), normal=buf(h, w, 3),
             albedo=buf(h, w, 3), den=buf(h, w, 3), out=buf(h, w, 3))
    hists = [buf(3, h, w, 4), buf(3, h, w, 4)]
    scratch = torch.empty(rtow.denoise_lib().rt_denoise_scratch_bytes(w, h), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ptr = {k: v.data_ptr() for k, v in t.items()}
    prev = None
    for i, (cam, p, view) in enumerate(frames):
        gpu_ctx.render_async(cam, p, ptr["beauty"], stream.cuda_stream)
        gpu_ctx.aov_async(cam, p, {k: ptr[k] for k in ("hits", "position", "normal", "albedo")},
                          stream=stream.cuda_stream)
        gpu_ctx.denoise_async({**{k: ptr[k] for k in rtow.DENOISE_INPUTS}, "out": ptr["den"]}, w, h, SPP,
                              scratch.data_ptr(), stream=stream.cuda_stream)
        gpu_ctx.temporal_async({"cur": ptr["den"], "hits": ptr["hits"], "position": ptr["position"],
                                "normal": ptr["normal"], "history_in": hists[1 - i].data_ptr() if i else None,
                                "history_out": hists[i].data_ptr(), "out": ptr["out"]},
                               w, h, SPP, prev, stream=stream.cuda_stream)
        stream.synchronize()
        den, out, hist = want[i]
        assert t["den"].cpu().numpy().tobytes() == den.tobytes(), i
        assert t["out"].cpu().numpy().tobytes() == out.tobytes(), i
        assert hists[i].cpu().numpy().tobytes() == hist.tobytes(), i
        prev = view
    geo = want[1][2][1, ..., 3] == 0
    assert (want[1][2][0, ..., 3][geo] > 1).mean() > 0.5  # the second frame did use the first one's history


def test_temporal_between_renders_leaves_them_alone(rtow, gpu_ctx):
    """The pass shares the context's serialisation and nothing else: a render
    before it and a render after it give the same bytes, and it needs no scene
    of its own."""
    gpu_ctx.upload(rtow.final_scene())
    cam = rtow.camera_cpu(aspect=64 / 36)
    p = rtow.make_params(64, 36, 5, seed=2024, flags=rtow.RT_FLAG_ACCEL_BVH)
    a, sa = gpu_ctx.render(cam, p)
    g = gpu_ctx.aov(cam, p)
    _, hist = gpu_ctx.temporal(a, g, 5)
    gpu_ctx.temporal(a, g, 5, rtow.temporal_view(cam, 64, 36), hist)
    b, sb = gpu_ctx.render(cam, p)
    assert a.tobytes() == b.tobytes() and sa.segments == sb.segments
    f, fh, view = inputs(67, 37)
    with rtow.Context(0) as fresh:  # no rt_scene_upload
        c = fresh.temporal(f["cur"], f, SPP, view, fh)
    d = gpu_ctx.temporal(f["cur"], f, SPP, view, fh)
    assert c[0].tobytes() == d[0].tobytes() and c[1].tobytes() == d[1].tobytes()


def _mse(sums, spp, truth):
    x = np.clip(np.sqrt(sums.astype(np.float64) / spp), 0.0, 1.0)
    return float(((x - truth) ** 2).mean())


def orbit_sequence(rtow, ctx, scene_name, w=128, h=72, spp=16, frames=8, degrees=1.0, seed0=1):
    """The quality test's sequence: per frame (denoised sums, feature buffers,
    view), seeds seed0 .. seed0 + frames - 1, and the truth of the last camera."""
    ctx.upload(rtow.final_scene() if scene_name == "final" else rtow.five_scene())
    flags = rtow.RT_FLAG_ACCEL_BVH
    cams = orbit_cameras(rtow, scene_name, w, h, frames, degrees)
    seq = []
    for i, cam in enumerate(cams):
        p = rtow.make_params(w, h, spp, seed=seed0 + i, flags=flags)
        g = ctx.aov(cam, p)
        seq.append((ctx.denoise(ctx.render(cam, p)[0], g, spp), g, rtow.temporal_view(cam, w, h)))
    truth = ctx.render(cams[-1], rtow.make_params(w, h, 4096, seed=99, flags=flags))[0]
    return seq, np.clip(np.sqrt(truth.astype(np.float64) / 4096), 0.0, 1.0)


def accumulate(ctx, seq, spp=16, **options):
    hist = view = out = None
    for den, g, v in seq:
        out, hist = ctx.temporal(den, g, spp, view, hist, **options)
        view = v
    return out, hist


@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_temporal_lowers_the_error_of_the_denoised_frame(rtow, gpu_ctx, scene_name):
    """End to end at 128x72, 16 spp: an 8-frame orbit at 1 degree per frame
    about lookat, seeds 1..8, every frame through render -> aov -> denoise ->
    temporal (defaults).  Truth: the product's 4096-spp render of the last
    camera with seed 99.  MSE on sqrt(mean) clamped to [0, 1].  The last
    accumulated frame's error is below the error of that frame's denoised
    input alone.  Nothing is asserted against a higher-spp render (DESIGN.md
    11 records the figures).

    Measured on the MI355X at the tuned defaults (max_len 2, plane_tol
    0.0003): final 6.86e-4 -> 6.41e-4, five 2.69e-4 -> 2.10e-4.  At the
    issue's starting values (max_len 32, plane_tol 0.01) both scenes get
    worse, 1.157e-3 and 7.44e-4: a loose plane test lets the silhouette
    pixels' history in ("Quality")."""
    seq, truth = orbit_sequence(rtow, gpu_ctx, scene_name)
    out, hist = accumulate(gpu_ctx, seq)
    den, g = seq[-1][0], seq[-1][1]
    mden, macc = _mse(den, 16, truth), _mse(out, 16, truth)
    geo = g["hits"] > 0
    share = float((hist[0, ..., 3][geo] >= 4).mean())
    print(f"temporal quality {scene_name}: mse denoised {mden:.6e}, accumulated {macc:.6e}, "
          f"share of non-sky pixels with len >= 4: {share:.4f}")
    assert macc < mden
