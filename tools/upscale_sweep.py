"""Sweep rt_upscale's plane_tol and normal_cos on the quality set-up of
tests/test_upscale_gpu.py: final and five-sphere scene, a 64x36
frame at 16 spp, denoised, upsampled to 128x72 with 16-spp guides; truth: the
4096-spp 128x72 render; MSE on sqrt(mean) clamped to [0, 1]; several seed sets.

  python tools/upscale_sweep.py [--seeds 3 --plane 0.01,0.1,inf --cos -1,0.9 --log profiles/upscale_sweep.log]

Prints, per scene, the mean MSE over the seed sets for every pair of options,
the plain bilinear upsample's and the native denoised frame's, and the share of
pixels per stage at each plane_tol (at normal_cos 0.9, or the first value given)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-in-one-weekend_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import rtow  # noqa: E402
import upscale_ref  # noqa: E402

VIEWS = {"final": dict(lookfrom=(13.0, 2.0, 3.0), lookat=(0.0, 0.0, 0.0), focus_dist=10.0),
         "five": dict(lookfrom=(-2.0, 0.5, 2.0), lookat=(0.0, 0.0, -1.0), vfov=40.0, focus_dist=3.4)}
PLANE = (0.001, 0.003, 0.01, 0.03, 0.1, 0.3, float("inf"))
COS = (-1.0, 0.5, 0.8, 0.9, 0.95, 0.99, 0.999)


def mse(mean, truth):
    return float(((np.clip(np.sqrt(mean), 0.0, 1.0) - truth) ** 2).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--plane", default=",".join(str(v) for v in PLANE), help="plane_tol values (inf = test off)")
    ap.add_argument("--cos", default=",".join(str(v) for v in COS), help="normal_cos values (-1 = test off)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "upscale_sweep.log"))
    a = ap.parse_args()
    plane, cos = [float(v) for v in a.plane.split(",")], [float(v) for v in a.cos.split(",")]
    mid = 0.9 if 0.9 in cos else cos[0]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    flags = rtow.RT_FLAG_ACCEL_BVH
    with rtow.Context(0) as ctx:
        for name, view in VIEWS.items():
            ctx.upload(rtow.final_scene() if name == "final" else rtow.five_scene())
            cam = rtow.camera_cpu(aspect=64 / 36, aperture=0.1, **view)
            truth = ctx.render(cam, rtow.make_params(128, 72, 4096, seed=99, flags=flags))[0]
            truth = np.clip(np.sqrt(truth.astype(np.float64) / 4096), 0.0, 1.0)
            lo_view, rays = rtow.temporal_view(cam, 64, 36), rtow.resolve_rays(cam, 128, 72)
            table = np.zeros((len(plane), len(cos)))
            stages = np.zeros((len(plane), 3))
            plain = native = 0.0
            for k in range(a.seeds):
                p_lo = rtow.make_params(64, 36, 16, seed=1 + 2 * k, flags=flags)
                p_hi = rtow.make_params(128, 72, 16, seed=2 + 2 * k, flags=flags)
                g_lo, g_hi = ctx.aov(cam, p_lo), ctx.aov(cam, p_hi)
                den = ctx.denoise(ctx.render(cam, p_lo)[0], g_lo, 16)
                plain += mse(upscale_ref.plain_bilinear(den, 16, lo_view, rays, 128, 72), truth) / a.seeds
                native += mse(ctx.denoise(ctx.render(cam, p_hi)[0], g_hi, 16).astype(np.float64) / 16, truth) / a.seeds
                for i, pt in enumerate(plane):
                    for j, nc in enumerate(cos):
                        out, st = ctx.upscale(den, g_lo, 16, g_hi, 16, lo_view, rays, plane_tol=pt, normal_cos=nc)
                        table[i, j] += mse(out.astype(np.float64) / 16, truth) / a.seeds
                        if nc == mid:
                            stages[i] += [float((st == s).mean()) / a.seeds for s in (1, 2, 3)]
            say(f"{name}: 64x36 -> 128x72, 16 spp, denoised, mean MSE over {a.seeds} seed sets; plain bilinear "
                f"{plain:.4e}, native 128x72 denoised {native:.4e}")
            say("plane_tol \\ normal_cos " + " ".join(f"{nc:10.3f}" for nc in cos) + f"   stage shares at {mid}")
            for i, pt in enumerate(plane):
                say(f"{pt:22.3f} " + " ".join(f"{v:10.4e}" for v in table[i]) +
                    "   " + " ".join(f"{v:.4f}" for v in stages[i]))
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
