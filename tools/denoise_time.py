"""Time the guided a-trous denoiser (include/rt_denoise.h) on a real frame, next
to the render and the feature pass it serves: final scene, 16 spp, everything
in device buffers, HIP events around repeated enqueues after a warm-up.

  python tools/denoise_time.py [--width 3840 --height 2160 --spp 16 --reps 20]

Prints, per iteration count 1..8, the time of one rt_denoise_async (prepare +
iterations) and its increment over the count before, and for the default count
the share of the byte bound per iteration (48 B read + 16 B written per pixel)
at the given bandwidth figure."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hbm-tbps", type=float, default=6.3, help="achievable HBM bandwidth the bound is taken at")
    a = ap.parse_args()
    w, h, spp = a.width, a.height, a.spp
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    cam = rtow.camera_cpu(aspect=w / h)
    p = rtow.make_params(w, h, spp, seed=7, flags=rtow.RT_FLAG_ACCEL_BVH)
    beauty = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    out = torch.zeros_like(beauty)
    g = {"hits": torch.zeros((h, w), dtype=torch.int32, device=dev)}
    for k in ("position", "normal", "albedo"):
        g[k] = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty(rtow.denoise_lib().rt_denoise_scratch_bytes(w, h), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with rtow.Context(0) as ctx:
        ctx.upload(rtow.final_scene())
        gp = {k: t.data_ptr() for k, t in g.items()}
        t_render = timed(lambda: ctx.render_async(cam, p, beauty.data_ptr(), s), a.reps, stream)
        t_aov = timed(lambda: ctx.aov_async(cam, p, gp, s), a.reps, stream)
        print(f"frame {w}x{h}, {spp} spp, final scene, {a.reps} repetitions after 2 warm-up calls, HIP events")
        print(f"render   {t_render:8.3f} ms")
        print(f"aov pass {t_aov:8.3f} ms")
        ptrs = {"beauty": beauty.data_ptr(), "out": out.data_ptr(), **gp}
        prev, times = None, {}
        for it in range(1, 9):
            t = timed(lambda: ctx.denoise_async(ptrs, w, h, spp, scratch.data_ptr(), s, iterations=it), a.reps,
                      stream)
            times[it] = t
            inc = "" if prev is None else f"  (+{t - prev:6.3f} ms for step {1 << (it - 1)})"
            print(f"denoise, {it} iteration(s) {t:8.3f} ms{inc}")
            prev = t
        its = rtow.DENOISE_DEFAULTS["iterations"]
        per = (times[its] - times[1]) / (its - 1)
        gb = 64.0 * w * h / 1e9
        bound_ms = gb / (a.hbm_tbps * 1e3) * 1e3
        print(f"default ({its} iterations): {times[its]:.3f} ms; mean increment per iteration {per:.3f} ms")
        print(f"byte bound per iteration: {gb:.3f} GB = {bound_ms:.3f} ms at {a.hbm_tbps} TB/s; "
              f"the mean increment reaches {100.0 * bound_ms / per:.1f} % of it "
              f"({gb / per:.2f} TB/s of the bound's bytes)")
        chk = np.isfinite(out.cpu().numpy()).all()
        print(f"output finite: {bool(chk)}")


if __name__ == "__main__":
    main()
