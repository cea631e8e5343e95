"""Time the dominant-route feature pass (include/rt_route.h, defaults) next to
the chain-following pass (include/rt_guides.h) whose chains it traces and the
first-hit pass (include/rt_aov.h), in one run: tools/guides_time.py's protocol
(final scene, everything in device buffers, HIP events around repeated
enqueues after a warm-up).

  python tools/route_time.py [--width 3840 --height 2160 --spp 1 16 --reps 20 --log profiles/route_pass.log]

There is no target: the number to read rt_route against is rt_guides on the
same device in the same run.  On top of rt_guides' work it moves 128 B of state
per pixel and launch and runs the finalize kernel (at most 64 B read and 52 B
written per pixel); the finalize kernel is timed alone as the difference
between an spp = 0 call (one initialising launch and the finalize) and is
compared with its HBM bound at 6.3 TB/s.  Prints the times, the ratios and the
share of hit samples the dominant routes cover, and writes the same lines to
--log."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-in-one-weekend_amd"))

import torch  # noqa: E402  (before rtow: INTEGRATION.md, "Loading")

import rtow  # noqa: E402
from guides_time import timed  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--spp", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "route_pass.log"))
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
    for name, _, ch in rtow.GUIDES_FIELDS + rtow.ROUTE_FIELDS[6:]:
        dt = torch.float32 if name in ("depth", "position", "normal", "albedo") else torch.int32
        g[name] = torch.zeros((h, w, 3) if ch == 3 else (h, w), dtype=dt, device=dev)
    state = torch.zeros(rtow.route_lib().rt_route_state_bytes(w, h) // 4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ptr = {k: t.data_ptr() for k, t in g.items()}
    ap6 = {k: ptr[k] for k, _, _ in rtow.AOV_FIELDS}
    gp8 = {k: ptr[k] for k, _, _ in rtow.GUIDES_FIELDS}
    rp8 = {k: ptr[k] for k, _, _ in rtow.ROUTE_FIELDS}
    st = state.data_ptr()
    with rtow.Context(0) as ctx:
        ctx.upload(rtow.final_scene())
        say(f"frame {w}x{h}, final scene, {a.reps} repetitions after 2 warm-up calls, HIP events; rt_route and "
            f"rt_guides at their defaults (max_bounces {rtow.GUIDES_DEFAULTS['max_bounces']}, max_fuzz 0), all eight "
            f"buffers each; rt_aov all six")
        p0 = rtow.make_params(w, h, 0, seed=7, flags=rtow.RT_FLAG_ACCEL_BVH)
        t_r0 = timed(lambda: ctx.route_async(cam, p0, rp8, st, s), a.reps, stream)
        t_g0 = timed(lambda: ctx.guides_async(cam, p0, gp8, s), a.reps, stream)
        px = w * h
        bound = px * (64 + 52) / HBM_BYTES_PER_S * 1e3
        say(f"  0 spp (an initialising launch; rt_route adds its finalize kernel): rt_route {t_r0:8.3f} ms, rt_guides "
            f"{t_g0:8.3f} ms; finalize at 64 B read + 52 B written per pixel: HBM bound {bound:.3f} ms at 6.3 TB/s")
        for spp in a.spp:
            p = rtow.make_params(w, h, spp, seed=7, flags=rtow.RT_FLAG_ACCEL_BVH)
            t_aov = timed(lambda: ctx.aov_async(cam, p, ap6, s), a.reps, stream)
            t_gd = timed(lambda: ctx.guides_async(cam, p, gp8, s), a.reps, stream)
            t_rt = timed(lambda: ctx.route_async(cam, p, rp8, st, s), a.reps, stream)
            ctx.route_async(cam, p, rp8, st, s)
            stream.synchronize()
            hits = int(g["hits"].sum(dtype=torch.int64))
            matched = int(g["matched"].sum(dtype=torch.int64))
            mixed = int((g["matched"] < g["hits"]).sum())
            say(f"{spp:3d} spp: rt_aov {t_aov:8.3f} ms, rt_guides {t_gd:8.3f} ms, rt_route {t_rt:8.3f} ms (ratio to "
                f"rt_guides {t_rt / t_gd:.3f}, to rt_aov {t_rt / t_aov:.2f}); hit samples {hits}, on their pixel's "
                f"dominant route {matched} ({matched / max(hits, 1):.3f}); pixels with matched < hits {mixed} "
                f"({mixed / px:.4f} of the frame)")
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
