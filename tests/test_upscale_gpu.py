"""Guided upsampling on the GPU (include/rt_upscale.h, rt_upscale /
Context.upscale): the two kernels give the bits of the numpy restatement
(tests/upscale_ref.py) on synthetic frame pairs that reach every branch and on
real frames rendered at both sizes; the properties of test_upscale.py hold on
the device; the asynchronous path, stage = NULL and the struct's zeros agree
with the synchronous call; the pass leaves the context's renders alone; and a
denoised 64x36 frame upsampled to 128x72 is closer to a 4096-spp render than
its plain bilinear upsample."""
import numpy as np
import pytest

import upscale_ref as ref
from test_temporal_gpu import FINAL_VIEW, FIVE_VIEW, _mse, same_bits
from test_upscale import OFF, check_demodulation, check_edges, check_identity, check_sky, synthetic

pytestmark = pytest.mark.gpu

# lo -> hi: the degenerate pair; one low-resolution pixel under several; smaller than a wave's 16x4; a
# non-integer ratio with partial tiles in both frames; whole tiles; a large ratio; shrinking
SHAPES = ((1, 1, 1, 1), (1, 1, 3, 2), (5, 3, 10, 6), (33, 17, 67, 37), (64, 64, 128, 128), (8, 8, 64, 64),
          (67, 37, 33, 17))
OPTIONS = {
    "defaults": {},
    "tests_off": OFF,
    "tight_plane": dict(plane_tol=1e-4),
    "tight_normal": dict(normal_cos=0.99),
    "no_albedo": dict(flags=ref.NO_ALBEDO),
}

_inputs = {}


def inputs(shape):
    """The seeded pair of frames of that shape, made once and never written to."""
    if shape not in _inputs:
        s = synthetic(shape)
        for a in [s["cur"]] + list(s["lo"].values()) + list(s["hi"].values()):
            a.setflags(write=False)
        _inputs[shape] = s
    return _inputs[shape]


def device_step(ctx):
    """Context.upscale with upscale_ref's signature."""
    def step(cur, lo, hi, lo_spp, spp, lo_view, rays, **options):
        return ctx.upscale(cur, lo, lo_spp, hi, spp, lo_view, rays, **options)
    return step


def without_albedo(aov):
    return {k: v for k, v in aov.items() if k != "albedo"}


@pytest.mark.parametrize("options", list(OPTIONS), ids=list(OPTIONS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_upscale_equals_the_restatement_bit_for_bit(gpu_ctx, shape, options):
    """The synthetic inputs (test_upscale_synthetic_inputs_reach_every_branch
    shows what they reach).  With NO_ALBEDO the albedo pointers are NULL."""
    s = inputs(shape)
    opt = OPTIONS[options]
    lo, hi = (s["lo"], s["hi"]) if "flags" not in opt else (without_albedo(s["lo"]), without_albedo(s["hi"]))
    out, stage = gpu_ctx.upscale(s["cur"], lo, s["lo_spp"], hi, s["spp"], s["lo_view"], s["rays"], **opt)
    want, want_stage = ref.upscale_ref(s["cur"], lo, hi, s["lo_spp"], s["spp"], s["lo_view"], s["rays"],
                                       **{**ref.DEFAULTS, **opt})
    assert np.isfinite(want).all()
    same_bits(out, want)
    assert np.array_equal(stage, want_stage)


def scene_cameras(rtow, scene_name, model):
    """The low-resolution (64x36) and the output (128x72) camera of one view."""
    view = FIVE_VIEW if scene_name == "five" else FINAL_VIEW
    if model == "cpu":
        return tuple(rtow.camera_cpu(aspect=64 / 36, aperture=0.1, **view) for _ in range(2))
    return tuple(rtow.camera_gpu(w, h, **view) for w, h in ((64, 36), (128, 72)))


def frames(rtow, ctx, cams, lo_spp, spp, denoise):
    """Render and rt_aov at both sizes through the ABI -> (cur, aov_lo, aov_hi, view, rays)."""
    flags = rtow.RT_FLAG_ACCEL_BVH
    p_lo = rtow.make_params(64, 36, lo_spp, seed=1, flags=flags)
    p_hi = rtow.make_params(128, 72, spp, seed=2, flags=flags)
    g_lo, g_hi = ctx.aov(cams[0], p_lo), ctx.aov(cams[1], p_hi)
    cur = ctx.render(cams[0], p_lo)[0]
    if denoise:
        cur = ctx.denoise(cur, g_lo, lo_spp)
    return cur, g_lo, g_hi, rtow.temporal_view(cams[0], 64, 36), rtow.resolve_rays(cams[1], 128, 72)


@pytest.mark.parametrize("model", ["cpu", "gpu"])
@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_upscale_equals_the_restatement_on_real_frames(rtow, gpu_ctx, scene_name, model):
    """64x36 -> 128x72 with both camera models, 4 spp below and 8 above: bit
    equality, a guided majority, and a mapping that is the half-pixel one the
    two frames of one camera must have."""
    gpu_ctx.upload(rtow.final_scene() if scene_name == "final" else rtow.five_scene())
    cams = scene_cameras(rtow, scene_name, model)
    cur, g_lo, g_hi, view, rays = frames(rtow, gpu_ctx, cams, 4, 8, False)
    assert list(view.eye) == list(rays.eye)
    out, stage = gpu_ctx.upscale(cur, g_lo, 4, g_hi, 8, view, rays)
    c = {}
    want, want_stage = ref.upscale_ref(cur, g_lo, g_hi, 4, 8, view, rays, census=c)
    same_bits(out, want)
    assert np.array_equal(stage, want_stage)
    share = [float((stage == k).mean()) for k in (1, 2, 3)]
    print(f"real frames {scene_name} {model}: stage shares {share[0]:.4f} {share[1]:.4f} {share[2]:.4f}")
    assert share[0] > 0.8
    # where the output's pixel (i, j) lies in the low-resolution frame, from the two headers' formulas.  GPU
    # model: pixel centres at (i + 0.5) / W of the width.  CPU model: fs = (i + 0.5) / (W - 1) and
    # ft = (H - 0.5 - j) / (H - 1) at the output's size, x = fs (w - 1) - 0.5 and y = (h - 0.5) - ft (h - 1) below
    jj, ii = np.mgrid[0:72, 0:128]
    if model == "gpu":
        ex, ey = (ii + 0.5) / 2 - 0.5, (jj + 0.5) / 2 - 0.5
    else:
        ex, ey = (ii + 0.5) * 63 / 127 - 0.5, 35.5 - (71.5 - jj) * 35 / 71
    assert np.abs(c["x"] - ex).max() < 2.0 ** -7 and np.abs(c["y"] - ey).max() < 2.0 ** -7


def test_upscale_identity_on_the_device(gpu_ctx):
    check_identity(device_step(gpu_ctx))


def test_upscale_demodulation_on_the_device(gpu_ctx):
    check_demodulation(device_step(gpu_ctx))


def test_upscale_edges_on_the_device(gpu_ctx):
    check_edges(device_step(gpu_ctx))


def test_upscale_sky_on_the_device(gpu_ctx):
    check_sky(device_step(gpu_ctx))


def test_upscale_struct_zero_means_default_and_stage_may_be_null(rtow, gpu_ctx):
    """Options left out (the struct's zeros) are the documented defaults; with
    stage = NULL the same out is written."""
    s = inputs((33, 17, 67, 37))
    args = (s["cur"], s["lo"], s["lo_spp"], s["hi"], s["spp"], s["lo_view"], s["rays"])
    a = gpu_ctx.upscale(*args)
    b = gpu_ctx.upscale(*args, **rtow.UPSCALE_DEFAULTS)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    d = rtow.upscale_desc(33, 17, 4, 67, 37, 8, s["lo_view"], s["rays"])
    assert (d.plane_tol, d.normal_cos, d.flags) == (0.0, 0.0, 0)
    c = gpu_ctx.upscale(*args, want_stage=False)
    assert c[1] is None and c[0].tobytes() == a[0].tobytes()


def test_upscale_async_on_a_second_stream(rtow, gpu_ctx):
    """rt_upscale_async into caller-owned device memory on a caller's stream
    gives the synchronous call's bytes, with a stage buffer and with stage =
    NULL, and leaves the inputs alone."""
    import torch
    shape = (33, 17, 67, 37)
    w, h, W, H = shape
    s = inputs(shape)
    want, want_stage = gpu_ctx.upscale(s["cur"], s["lo"], s["lo_spp"], s["hi"], s["spp"], s["lo_view"], s["rays"])
    dev = torch.device("cuda:0")
    host = {"cur": s["cur"]}
    for tag in ("lo", "hi"):
        for k, a in s[tag].items():
            host[f"{k}_{tag}"] = a.view(np.int32) if k == "hits" else a
    t = {k: torch.from_numpy(np.array(a)).to(dev) for k, a in host.items()}
    out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device=dev)
    stage = torch.full((H, W), 7, dtype=torch.uint8, device=dev)
    nbytes = rtow.upscale_scratch_bytes(w, h)
    assert nbytes == 48 * w * h
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    ptrs["out"] = out.data_ptr()
    call = (w, h, s["lo_spp"], W, H, s["spp"], s["lo_view"], s["rays"], scratch.data_ptr())
    gpu_ctx.upscale_async({**ptrs, "stage": stage.data_ptr()}, *call, stream=stream.cuda_stream)
    stream.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert stage.cpu().numpy().tobytes() == want_stage.tobytes()
    assert scratch.cpu().numpy().view(np.float32).tobytes() == ref.planes(s["cur"], s["lo"], s["lo_spp"]).tobytes()
    for k, a in host.items():
        assert t[k].cpu().numpy().tobytes() == a.tobytes(), k
    out.fill_(7.0)
    stage.fill_(7)
    torch.cuda.current_stream(dev).synchronize()
    gpu_ctx.upscale_async(ptrs, *call, stream=stream.cuda_stream)  # stage = NULL
    stream.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert (stage.cpu().numpy() == 7).all()
    with pytest.raises(rtow.RTError):  # out on an input: rejected, nothing written
        gpu_ctx.upscale_async({**ptrs, "out": ptrs["position_hi"]}, *call, stream=stream.cuda_stream)
    stream.synchronize()
    assert t["position_hi"].cpu().numpy().tobytes() == host["position_hi"].tobytes()


def test_upscale_between_renders_leaves_them_alone(rtow, gpu_ctx):
    """A render before the pass and a render after it give the same bytes, and
    the pass needs no scene of its own."""
    gpu_ctx.upload(rtow.final_scene())
    cam = rtow.camera_cpu(aspect=64 / 36)
    p = rtow.make_params(64, 36, 5, seed=2024, flags=rtow.RT_FLAG_ACCEL_BVH)
    a, sa = gpu_ctx.render(cam, p)
    g = gpu_ctx.aov(cam, p)
    gpu_ctx.upscale(a, g, 5, g, 5, rtow.temporal_view(cam, 64, 36), rtow.resolve_rays(cam, 64, 36))
    b, sb = gpu_ctx.render(cam, p)
    assert a.tobytes() == b.tobytes() and sa.segments == sb.segments
    s = inputs((33, 17, 67, 37))
    args = (s["cur"], s["lo"], s["lo_spp"], s["hi"], s["spp"], s["lo_view"], s["rays"])
    with rtow.Context(0) as fresh:  # no rt_scene_upload
        c = fresh.upscale(*args)
    d = gpu_ctx.upscale(*args)
    assert c[0].tobytes() == d[0].tobytes() and c[1].tobytes() == d[1].tobytes()


@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_upscale_beats_the_plain_bilinear_upsample(rtow, gpu_ctx, scene_name):
    """Truth: the 4096-spp 128x72 render (seed 99), MSE on sqrt(mean) clamped
    to [0, 1] (test_temporal_gpu.py's _mse).  Input: the 64x36 frame at 16
    spp, denoised.  rt_upscale at its defaults (output guides at 16 spp) has a
    lower error than the plain bilinear upsample of the same frame at the same
    (x, y), computed here in numpy.  Recorded, not asserted: the native
    128x72, 16-spp, denoised frame's error.  DESIGN.md 13 has the figures.

    Measured on the MI355X at the tuned defaults (plane_tol 0.1, normal_cos
    -0.5): final 2.823e-3 plain, 1.438e-3 upsampled, 7.08e-4 native; five
    7.960e-4, 5.270e-4, 2.51e-4.  At the issue's starting values (0.01, 0.9):
    1.689e-3 and 5.225e-4, the test passing there too."""
    gpu_ctx.upload(rtow.final_scene() if scene_name == "final" else rtow.five_scene())
    cams = scene_cameras(rtow, scene_name, "cpu")
    flags = rtow.RT_FLAG_ACCEL_BVH
    truth = gpu_ctx.render(cams[1], rtow.make_params(128, 72, 4096, seed=99, flags=flags))[0]
    truth = np.clip(np.sqrt(truth.astype(np.float64) / 4096), 0.0, 1.0)
    den, g_lo, g_hi, view, rays = frames(rtow, gpu_ctx, cams, 16, 16, True)
    out, stage = gpu_ctx.upscale(den, g_lo, 16, g_hi, 16, view, rays)
    plain = ref.plain_bilinear(den, 16, view, rays, 128, 72)
    m_up, m_plain = _mse(out, 16, truth), _mse(plain, 1, truth)
    p_hi = rtow.make_params(128, 72, 16, seed=2, flags=flags)
    native = gpu_ctx.denoise(gpu_ctx.render(cams[1], p_hi)[0], g_hi, 16)
    m_native = _mse(native, 16, truth)
    print(f"upscale quality {scene_name}: mse plain bilinear {m_plain:.6e}, rt_upscale {m_up:.6e}, native 128x72 "
          f"denoised {m_native:.6e}; stage shares " + " ".join(f"{float((stage == k).mean()):.4f}" for k in (1, 2, 3)))
    assert m_up < m_plain
