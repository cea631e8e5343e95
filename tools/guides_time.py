"""Time the chain-following feature pass (include/rt_guides.h, defaults) next
to the first-hit pass (include/rt_aov.h) it extends: final scene, everything
in device buffers, HIP events around repeated enqueues after a warm-up.

  python tools/guides_time.py [--width 3840 --height 2160 --spp 1 16 --reps 20 --log profiles/guides_pass.log]

There is no target: the number to read rt_guides against is rt_aov on the same
device in the same run.  Prints both times, their ratio and the mean number of
specular bounces followed per hit sample, and writes the same lines to --log."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-in-one-weekend_amd"))

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
    ap.add_argument("--spp", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "guides_pass.log"))
    a = ap.parse_args()
    w, h = a.width, a.height
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    cam = rtow.camera_cpu(aspect=w / h)
    g = {}
    for name, _, ch in rtow.GUIDES_FIELDS:
        dt = torch.float32 if name in ("depth", "position", "normal", "albedo") else torch.int32
        g[name] = torch.zeros((h, w, 3) if ch == 3 else (h, w), dtype=dt, device=dev)
    torch.cuda.synchronize()
    gp = {k: t.data_ptr() for k, t in g.items()}
    ap6 = {k: gp[k] for k, _, _ in rtow.AOV_FIELDS}
    with rtow.Context(0) as ctx:
        ctx.upload(rtow.final_scene())
        say(f"frame {w}x{h}, final scene, {a.reps} repetitions after 2 warm-up calls, HIP events; rt_guides at its "
            f"defaults (max_bounces {rtow.GUIDES_DEFAULTS['max_bounces']}, max_fuzz 0), all eight buffers; rt_aov all six")
        for spp in a.spp:
            p = rtow.make_params(w, h, spp, seed=7, flags=rtow.RT_FLAG_ACCEL_BVH)
            t_aov = timed(lambda: ctx.aov_async(cam, p, ap6, s), a.reps, stream)
            t_gd = timed(lambda: ctx.guides_async(cam, p, gp, s), a.reps, stream)
            t_g0 = timed(lambda: ctx.guides_async(cam, p, gp, s, max_bounces=0), a.reps, stream)
            ctx.guides_async(cam, p, gp, s)
            stream.synchronize()
            hits = int(g["hits"].sum(dtype=torch.int64))
            bounces = int(g["bounces"].sum(dtype=torch.int64))
            escaped = int(g["escaped"].sum(dtype=torch.int64))
            say(f"{spp:3d} spp: rt_aov {t_aov:8.3f} ms, rt_guides {t_gd:8.3f} ms (ratio {t_gd / t_aov:.2f}), rt_guides "
                f"with nothing followed {t_g0:8.3f} ms; hit samples {hits}, bounces followed {bounces} "
                f"({bounces / max(hits, 1):.3f} per hit sample), escaped {escaped} ({escaped / max(hits, 1):.3f})")
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
