"""Time guided upsampling (include/rt_upscale.h) and the two preview pipelines
it chooses between: final scene, 16 spp, everything in device buffers, HIP
events around repeated enqueues after a warm-up.

  python tools/upscale_time.py [--width 3840 --height 2160 --spp 16 --reps 20 --log profiles/upscale_pass.log]

The low-resolution frame is half the output's size in both directions.  Stage
by stage: the native pipeline (render, aov pass and denoiser at the output's
size) and the upscaled one (render, aov pass and denoiser at the low size, the
aov pass at the output's size, rt_upscale).  The pass is timed as a whole and
with an output of 1 x 1 pixel, which leaves its first launch; the second is the
difference.  Prints the pass as a share of its byte bound -- launch 1 reads 52 B
and writes 48 B per low-resolution pixel, launch 2 reads those 48 B once, 40 B
per output pixel and writes 12 B (13 B with a stage buffer, which the timed
calls do not ask for) -- next to rt_resolve at the output's size as a share of
its own bound (tools/resolve_time.py), and writes the same lines to --log."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-in-one-weekend_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before rtow: INTEGRATION.md, "Loading")

import rtow  # noqa: E402


def timed(fn, reps, stream):
    fn()
    fn()
    stream.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def orbit(lookfrom, degrees):
    a = math.radians(degrees)
    x, y, z = lookfrom
    return (x * math.cos(a) + z * math.sin(a), y, -x * math.sin(a) + z * math.cos(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hbm-tbps", type=float, default=6.3, help="achievable HBM bandwidth the bounds are taken at")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "upscale_pass.log"))
    a = ap.parse_args()
    W, H, spp = a.width, a.height, a.spp
    w, h = W // 2, H // 2
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream

    def buffers(cols, rows):
        g = {"hits": torch.zeros((rows, cols), dtype=torch.int32, device=dev),
             "depth": torch.zeros((rows, cols), dtype=torch.float32, device=dev)}
        for k in ("position", "normal", "albedo", "beauty", "den"):
            g[k] = torch.zeros((rows, cols, 3), dtype=torch.float32, device=dev)
        g["scratch"] = torch.empty(rtow.denoise_lib().rt_denoise_scratch_bytes(cols, rows), dtype=torch.uint8, device=dev)
        return g

    lo, hi = buffers(w, h), buffers(W, H)
    out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    stage = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    up_scratch = torch.empty(rtow.upscale_scratch_bytes(w, h), dtype=torch.uint8, device=dev)
    hist = [torch.zeros((3, H, W, 4), dtype=torch.float32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    cams = [rtow.camera_cpu(lookfrom=orbit((13.0, 2.0, 3.0), d), aspect=W / H) for d in (0.0, 1.0)]
    cam = cams[1]
    flags = rtow.RT_FLAG_ACCEL_BVH
    aov_names = ("hits", "depth", "position", "normal", "albedo")

    def stages(ctx, g, cols, rows, seed, camera=cam):
        p = rtow.make_params(cols, rows, spp, seed=seed, flags=flags)
        dn = {"beauty": g["beauty"].data_ptr(), "out": g["den"].data_ptr(),
              **{k: g[k].data_ptr() for k in rtow.DENOISE_INPUTS[1:]}}
        return (("render", lambda: ctx.render_async(camera, p, g["beauty"].data_ptr(), s)),
                ("aov pass", lambda: ctx.aov_async(camera, p, {k: g[k].data_ptr() for k in aov_names}, s)),
                ("denoise", lambda: ctx.denoise_async(dn, cols, rows, spp, g["scratch"].data_ptr(), s)))

    with rtow.Context(0) as ctx:
        ctx.upload(rtow.final_scene())
        # the yardstick's history: the previous frame of a 1-degree orbit at the output's size
        for _, fn in stages(ctx, hi, W, H, 7, cams[0]):
            fn()
        rs = {"cur": hi["den"].data_ptr(), "out": out.data_ptr(), **{k: hi[k].data_ptr() for k in ("hits", "depth", "normal")}}
        ctx.resolve_async({**rs, "history_out": hist[0].data_ptr()}, W, H, spp, None, rtow.resolve_rays(cams[0], W, H), s)
        stream.synchronize()
        say(f"output {W}x{H}, low resolution {w}x{h}, {spp} spp, final scene, {a.reps} repetitions after 2 warm-up "
            "calls, HIP events")
        native = {name: timed(fn, a.reps, stream) for name, fn in stages(ctx, hi, W, H, 8)}
        low = {name: timed(fn, a.reps, stream) for name, fn in stages(ctx, lo, w, h, 9)}
        view, rays = rtow.temporal_view(cam, w, h), rtow.resolve_rays(cam, W, H)
        ptrs = {"cur": lo["den"].data_ptr(), "out": out.data_ptr()}
        for tag, g in (("lo", lo), ("hi", hi)):
            for k in ("hits", "position", "normal", "albedo"):
                ptrs[f"{k}_{tag}"] = g[k].data_ptr()

        def upscale(cols=W, rows=H, r=rays, **extra):
            ctx.upscale_async({**ptrs, **extra}, w, h, spp, cols, rows, spp, view, r, up_scratch.data_ptr(), s)

        t_up = timed(upscale, a.reps, stream)
        one = rtow.resolve_rays(cam, 2, 2)  # (the CPU camera model needs two pixels each way; one is computed)
        t_l1 = timed(lambda: upscale(1, 1, one), a.reps, stream)
        t_res = timed(lambda: ctx.resolve_async({**rs, "history_in": hist[0].data_ptr(), "history_out": hist[1].data_ptr()},
                                                W, H, spp, rtow.temporal_view(cams[0], W, H), rays, s), a.reps, stream)
        for name, ms in native.items():
            say(f"{name:9s} {W}x{H} {ms:8.3f} ms")
        for name, ms in low.items():
            say(f"{name:9s} {w}x{h} {ms:8.3f} ms")
        say(f"upscale   {w}x{h} -> {W}x{H} {t_up:8.3f} ms: launch 1 (timed with a 1x1 output) {t_l1:8.3f} ms, launch 2 "
            f"(the difference) {t_up - t_l1:8.3f} ms")
        t_native = sum(native.values())
        t_upscaled = sum(low.values()) + native["aov pass"] + t_up
        say(f"native pipeline (render + aov pass + denoise at {W}x{H}) {t_native:8.3f} ms")
        say(f"upscaled pipeline ({w}x{h} render + aov pass + denoise, {W}x{H} aov pass, upscale) {t_upscaled:8.3f} ms "
            f"= {100.0 * t_upscaled / t_native:.1f} % of the native one")
        nb = 52 * W * H + 148 * w * h
        bound = nb / (a.hbm_tbps * 1e12) * 1e3
        frac = bound / t_up
        say(f"upscale byte bound: 52 B x {W * H} + (52 + 48 + 48) B x {w * h} = {nb} B = {bound:.3f} ms at "
            f"{a.hbm_tbps} TB/s; the pass reaches {100.0 * frac:.1f} % of it")
        rb = 140 * W * H
        rbound = rb / (a.hbm_tbps * 1e12) * 1e3
        rfrac = rbound / t_res
        say(f"yardstick rt_resolve {W}x{H} {t_res:8.3f} ms; its byte bound 140 B x {W * H} = {rb} B = {rbound:.3f} ms; "
            f"it reaches {100.0 * rfrac:.1f} % of it; upscale's share is {frac / rfrac:.2f} of resolve's")
        upscale(stage=stage.data_ptr())
        stream.synchronize()
        st = stage.cpu().numpy()
        say("share of output pixels per stage: " + ", ".join(f"stage {k} {float((st == k).mean()):.5f}" for k in (1, 2, 3))
            + f"; output finite: {bool(np.isfinite(out.cpu().numpy()).all())}")
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
