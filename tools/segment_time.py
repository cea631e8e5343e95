"""Time the limited query (include/rt_segment.h) next to the batch query
(include/rt_trace.h) on secondary rays: final scene, layer grid, everything in
device buffers, HIP events around repeated enqueues after a warm-up.

  python tools/segment_time.py [--width 3840 --height 2160 --reps 20 --log profiles/segment_pass.log]

The rays: rt_trace on the pinhole camera's pixel-centre rays of the frame (in
8x8-tile order, tools/trace_time.py's batch (a)); from every hit one
cosine-weighted hemisphere ray, origin = position, direction = normal + a
uniform unit vector (numpy, seeded), kept in the primary rays' order.  These
are the rays of an ambient-occlusion or a diffuse bounce pass: neighbours
start close together and fan out.

rt_trace is timed on them twice, first and last; the spread of the two is the
run's noise.  rt_segment is timed without a limit (t_max = +inf: the same
walks, one more input) and at world lengths 4, 1 and 0.25.  There is no
target: the lines say what a limit saves on this scene.  Prints the times and
writes the same lines to --log."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-in-one-weekend_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before rtow: INTEGRATION.md, "Loading")

import rtow  # noqa: E402
from trace_time import pixel_centre_rays, tile_order, timed  # noqa: E402

LENGTHS = (4.0, 1.0, 0.25)


def hemisphere_rays(position, normal, seed):
    """One cosine-weighted direction per hit: normal + a uniform unit vector
    (float32; a sum shorter than 1e-3 is replaced by the normal)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=position.shape).astype(np.float32)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = normal + u
    short = np.linalg.norm(d, axis=1) < 1e-3
    d[short] = normal[short]
    return position, d.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "segment_pass.log"))
    a = ap.parse_args()
    w, h = a.width, a.height
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    flags = rtow.RT_FLAG_ACCEL_BVH
    cam = rtow.camera_cpu(aspect=w / h, aperture=0.0)
    o, d = pixel_centre_rays(cam, w, h)
    sel = tile_order(w, h)
    with rtow.Context(0) as ctx:
        ctx.upload(rtow.final_scene())
        first = ctx.trace(o.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel], which=("id", "position", "normal"), flags=flags)
        hit = first["id"] >= 0
        so, sd = hemisphere_rays(first["position"][hit], first["normal"][hit], seed=17)
        n = len(so)
        ln = np.linalg.norm(sd.astype(np.float64), axis=1)
        say(f"frame {w}x{h}: {w * h} primary rays, {n} hits, one cosine-hemisphere ray per hit (seed 17); final scene, "
            f"RT_FLAG_ACCEL_BVH (layer grid), {a.reps} repetitions after 2 warm-up calls, HIP events, all outputs")
        to, td = torch.from_numpy(so).to(dev), torch.from_numpy(sd).to(dev)
        out = {"blocked": torch.zeros(n, dtype=torch.uint8, device=dev), "id": torch.zeros(n, dtype=torch.int32, device=dev),
               "t": torch.zeros(n, dtype=torch.float32, device=dev),
               "position": torch.zeros((n, 3), dtype=torch.float32, device=dev),
               "normal": torch.zeros((n, 3), dtype=torch.float32, device=dev)}
        ptrs = {k: t.data_ptr() for k, t in out.items()}
        ptrs.update(origin=to.data_ptr(), direction=td.data_ptr())
        tptrs = {k: v for k, v in ptrs.items() if k != "blocked"}
        torch.cuda.synchronize()

        def time_trace(label):
            t = timed(lambda: ctx.trace_async(tptrs, n, flags, s), a.reps, stream)
            stream.synchronize()
            ids = out["id"].cpu().numpy()
            say(f"rt_trace {label}: {t:8.3f} ms, {t * 1e6 / n:.3f} ns per ray, hits {int((ids >= 0).sum())}")
            return t, ids

        t_first, ids_trace = time_trace("(first)")
        rows = []
        for label, length in [("t_max = +inf", np.inf)] + [(f"length {L:g}", L) for L in LENGTHS]:
            tm = torch.from_numpy((length / ln).astype(np.float32)).to(dev)
            ptrs["t_max"] = tm.data_ptr()
            torch.cuda.synchronize()
            t = timed(lambda: ctx.segment_async(ptrs, n, flags, s), a.reps, stream)
            stream.synchronize()
            ids, blocked = out["id"].cpu().numpy(), out["blocked"].cpu().numpy()
            assert ((ids >= 0) == (blocked == 1)).all()
            rows.append((label, t, int(blocked.sum())))
            if not np.isfinite(length):
                say(f"rt_segment {label}: ids equal rt_trace's: {bool(np.array_equal(ids, ids_trace))}")
        t_last, _ = time_trace("(last)")
        t_ref = 0.5 * (t_first + t_last)
        say(f"rt_trace twice: {t_first:.3f} and {t_last:.3f} ms, spread {abs(t_first - t_last):.3f} ms "
            f"({100 * abs(t_first - t_last) / t_ref:.1f} %): the noise; mean {t_ref:.3f} ms")
        for label, t, nb in rows:
            say(f"rt_segment {label}: {t:8.3f} ms, {t / t_ref:.2f} of rt_trace ({t - t_ref:+.3f} ms), "
                f"blocked {nb} ({100 * nb / n:.1f} %)")
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
