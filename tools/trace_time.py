"""Time the batch query (include/rt_trace.h) next to the first-hit pass
(include/rt_aov.h) on the same rays: final scene, the pinhole camera's
pixel-centre rays of a 3840x2160 frame, everything in device buffers, HIP
events around repeated enqueues after a warm-up.

  python tools/trace_time.py [--width 3840 --height 2160 --reps 20 --log profiles/trace_pass.log]

Batch (a) holds the rays in 8x8-tile order, a wave's 64 rays one tile of the
frame as in rt_aov; batch (b) the same rays in a random permutation.  There is
no target: (a) is read against rt_aov at 1 spp on the same frame in the same
run (rt_aov jitters its rays inside the pixel and writes 52 bytes per pixel
where rt_trace reads 24 and writes 32), and (b) shows what incoherent waves
cost.  Prints the times and writes the same lines to --log."""
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


def pixel_centre_rays(cam, w, h):
    """The CPU-model pinhole camera's rays through the pixel centres, float32
    (h, w, 3) origins and unnormalised directions (camera_dir with u = 0.5)."""
    f32 = np.float32
    col, row = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    fs = (col + f32(0.5)) * f32(1.0 / (w - 1))
    ft = (f32(h - 1) - row + f32(0.5)) * f32(1.0 / (h - 1))
    eye, corner, hz, vt = (np.array(v[:], f32) for v in (cam.eye, cam.corner, cam.horiz, cam.vert))
    d = corner + fs[..., None] * hz + ft[..., None] * vt - eye
    return np.broadcast_to(eye, d.shape).copy(), d.astype(f32)


def tile_order(w, h, tile=8):
    """Pixel indices in 8x8-tile order (tiles row-major, pixels row-major in a tile)."""
    idx = np.arange(w * h).reshape(h, w)
    assert w % tile == 0 and h % tile == 0
    return idx.reshape(h // tile, tile, w // tile, tile).transpose(0, 2, 1, 3).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "trace_pass.log"))
    a = ap.parse_args()
    w, h = a.width, a.height
    n = w * h
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    cam = rtow.camera_cpu(aspect=w / h, aperture=0.0)
    o, d = pixel_centre_rays(cam, w, h)
    order = {"(a) 8x8-tile order": tile_order(w, h), "(b) random permutation": np.random.default_rng(1).permutation(n)}
    out = {"id": torch.zeros(n, dtype=torch.int32, device=dev), "t": torch.zeros(n, dtype=torch.float32, device=dev),
           "position": torch.zeros((n, 3), dtype=torch.float32, device=dev),
           "normal": torch.zeros((n, 3), dtype=torch.float32, device=dev)}
    aov = {}
    for name, _, ch in rtow.AOV_FIELDS:
        dt = torch.float32 if name in ("depth", "position", "normal", "albedo") else torch.int32
        aov[name] = torch.zeros((h, w, 3) if ch == 3 else (h, w), dtype=dt, device=dev)
    torch.cuda.synchronize()
    with rtow.Context(0) as ctx:
        ctx.upload(rtow.final_scene())
        say(f"frame {w}x{h} ({n} rays), final scene, RT_FLAG_ACCEL_BVH (layer grid), {a.reps} repetitions after 2 "
            f"warm-up calls, HIP events; rt_trace all four outputs, rt_aov all six at 1 spp")
        p = rtow.make_params(w, h, 1, seed=7, flags=rtow.RT_FLAG_ACCEL_BVH)
        ap6 = {k: t.data_ptr() for k, t in aov.items()}
        t_aov = timed(lambda: ctx.aov_async(cam, p, ap6, s), a.reps, stream)
        say(f"rt_aov 1 spp: {t_aov:8.3f} ms")
        ids = {}
        for label, sel in order.items():
            to = torch.from_numpy(np.ascontiguousarray(o.reshape(-1, 3)[sel])).to(dev)
            td = torch.from_numpy(np.ascontiguousarray(d.reshape(-1, 3)[sel])).to(dev)
            ptrs = {k: t.data_ptr() for k, t in out.items()}
            ptrs.update(origin=to.data_ptr(), direction=td.data_ptr())
            torch.cuda.synchronize()
            t_tr = timed(lambda: ctx.trace_async(ptrs, n, rtow.RT_FLAG_ACCEL_BVH, s), a.reps, stream)
            stream.synchronize()
            got = out["id"].cpu().numpy()
            back = np.empty(n, np.int32)
            back[sel] = got
            ids[label] = back
            say(f"rt_trace {label}: {t_tr:8.3f} ms (ratio to rt_aov {t_tr / t_aov:.2f}), "
                f"{t_tr * 1e6 / n:.3f} ns per ray, hits {int((got >= 0).sum())}, invalid {int((got == -2).sum())}")
        a_ids, b_ids = ids.values()
        say(f"ids of the two orders agree: {bool(np.array_equal(a_ids, b_ids))}")
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
