"""Time the clamped temporal resolve (include/rt_resolve.h) on a real orbit,
next to rt_temporal on the same inputs and to the render, the feature pass and
the denoiser both follow: final scene, 16 spp, everything in device buffers, HIP
events around repeated enqueues after a warm-up.

  python tools/resolve_time.py [--width 3840 --height 2160 --spp 16 --reps 20 --log profiles/resolve_pass.log]

Two frames of a 1-degree-per-frame orbit: the first fills a history, the second
is timed stage by stage with that history as its input (every repetition reads
the same history and writes the other buffer).  Prints the pass as a share of
its byte bound (32 B of sums and 48 B of history read, 60 B written per pixel)
at the given bandwidth figure, and writes the same lines to --log."""
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
    ap.add_argument("--hbm-tbps", type=float, default=6.3, help="achievable HBM bandwidth the bound is taken at")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "resolve_pass.log"))
    a = ap.parse_args()
    w, h, spp = a.width, a.height, a.spp
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    cams = [rtow.camera_cpu(lookfrom=orbit((13.0, 2.0, 3.0), d), aspect=w / h) for d in (0.0, 1.0)]
    beauty = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    den = torch.zeros_like(beauty)
    out = torch.zeros_like(beauty)
    g = {"hits": torch.zeros((h, w), dtype=torch.int32, device=dev)}
    g["depth"] = torch.zeros((h, w), dtype=torch.float32, device=dev)
    for k in ("position", "normal", "albedo"):
        g[k] = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty(rtow.denoise_lib().rt_denoise_scratch_bytes(w, h), dtype=torch.uint8, device=dev)
    hist = [torch.zeros((3, h, w, 4), dtype=torch.float32, device=dev) for _ in range(2)]
    assert hist[0].numel() * 4 == rtow.temporal_lib().rt_temporal_history_bytes(w, h)
    torch.cuda.synchronize()
    with rtow.Context(0) as ctx:
        ctx.upload(rtow.final_scene())
        gp = {k: t.data_ptr() for k, t in g.items()}
        dn = {"beauty": beauty.data_ptr(), "out": den.data_ptr(), **{k: gp[k] for k in rtow.DENOISE_INPUTS[1:]}}
        tp = {"cur": den.data_ptr(), "out": out.data_ptr(), **{k: gp[k] for k in ("hits", "position", "normal")}}
        rs = {"cur": den.data_ptr(), "out": out.data_ptr(), **{k: gp[k] for k in ("hits", "depth", "normal")}}

        def frame(i, time_it):
            p = rtow.make_params(w, h, spp, seed=7 + i, flags=rtow.RT_FLAG_ACCEL_BVH)
            prev = rtow.temporal_view(cams[i - 1], w, h) if i else None
            now = rtow.resolve_rays(cams[i], w, h)
            hp = {"history_out": hist[i & 1].data_ptr()}
            if i:
                hp["history_in"] = hist[(i - 1) & 1].data_ptr()
            stages = (("render", lambda: ctx.render_async(cams[i], p, beauty.data_ptr(), s)),
                      ("aov pass", lambda: ctx.aov_async(cams[i], p, gp, s)),
                      ("denoise", lambda: ctx.denoise_async(dn, w, h, spp, scratch.data_ptr(), s)),
                      ("temporal", lambda: ctx.temporal_async({**tp, **hp}, w, h, spp, prev, s)),
                      ("resolve", lambda: ctx.resolve_async({**rs, **hp}, w, h, spp, prev, now, s)))
            times = {}
            for name, fn in stages:
                if time_it:
                    times[name] = timed(fn, a.reps, stream)
                else:
                    fn()
            stream.synchronize()
            return times

        frame(0, False)
        t = frame(1, True)
        say(f"frame {w}x{h}, {spp} spp, final scene, second frame of a 1-degree orbit, {a.reps} repetitions after 2 "
            "warm-up calls, HIP events")
        for name, ms in t.items():
            say(f"{name:9s}{ms:8.3f} ms")
        say(f"render, aov pass, denoise and resolve {sum(t.values()) - t['temporal']:8.3f} ms")
        # hist[0] still holds the first frame's history, hist[1] the second frame's (the resolve ran last)
        now, prev = rtow.resolve_rays(cams[1], w, h), rtow.temporal_view(cams[0], w, h)
        hp = {"history_in": hist[0].data_ptr(), "history_out": hist[1].data_ptr()}
        t1 = timed(lambda: ctx.resolve_async({**rs, **hp}, w, h, spp, prev, now, s, gamma=float("inf")), a.reps, stream)
        say(f"resolve with the clamp off (no neighbourhood reads) {t1:8.3f} ms")
        ctx.resolve_async({**rs, **hp}, w, h, spp, prev, now, s)  # the defaults' history for the share below
        stream.synchronize()
        gb = 140.0 * w * h / 1e9
        bound_ms = gb / (a.hbm_tbps * 1e3) * 1e3
        say(f"byte bound: 140 B per pixel = {gb:.3f} GB = {bound_ms:.3f} ms at {a.hbm_tbps} TB/s; the pass reaches "
            f"{100.0 * bound_ms / t['resolve']:.1f} % of it ({gb / t['resolve']:.2f} TB/s of the bound's bytes)")
        ln = hist[1][0, ..., 3].cpu().numpy()
        geo = g["hits"].cpu().numpy() > 0
        say(f"non-sky pixels that found history (resolve): {float((ln[geo] > 1).mean()):.4f}; output finite: "
            f"{bool(np.isfinite(out.cpu().numpy()).all())}")
        t0 = timed(lambda: ctx.resolve_async({**rs, "history_out": hist[0].data_ptr()}, w, h, spp, None, now, s), a.reps,
                   stream)
        say(f"resolve without a history (first frame) {t0:8.3f} ms")
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
