"""The mirror room and the fp64 solution of its one-bounce paths (test
infrastructure): shared by the GPU test of rt_guides' geometry
(test_guides_gpu.py) and the CPU test of the chain oracle's
(test_features_oracle.py)."""
import numpy as np

A_MIRROR = (0.7, 0.6, 0.5)


def mirror_room(rtow, dx=2.5):
    """A fuzz-0 metal sphere at the origin, a lambertian ground and four small
    lambertian spheres with distinct albedos around it."""
    c = [(0, 0, 0), (0, -1001, 0), (dx, -0.5, 0.5), (dx, -0.5, -0.5), (-dx, -0.5, 0.5), (-dx, -0.5, -0.5)]
    c = np.array(c, np.float32)
    alb = np.array([A_MIRROR, (0.5, 0.5, 0.5), (0.8, 0.2, 0.1), (0.1, 0.7, 0.3), (0.2, 0.3, 0.9), (0.9, 0.8, 0.15)],
                   np.float32)
    kind = np.array([rtow.RT_METAL] + [rtow.RT_LAMBERTIAN] * 5, np.uint32)
    return rtow.Scene(c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(),
                      np.array([1, 1000, 0.5, 0.5, 0.5, 0.5], np.float32), kind, alb, np.zeros(6, np.float32))


def mirror_room_camera(rtow, w, h):
    return rtow.camera_gpu(w, h, lookfrom=(0.0, 0.5, 6.0), lookat=(0.0, 0.0, 0.0), vfov=40.0, defocus_angle=0.0,
                           focus_dist=6.0)


def roots64(o, d, c, r):
    """fp64 roots (t0 <= t1, NaN where the line misses) of |o + t d - c| = |r|, |d| = 1."""
    oc = o - c
    b = (oc * d).sum(-1)
    cc = (oc * oc).sum(-1) - r * r
    disc = b * b - cc
    sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
    q = -(b + np.where(b < 0, -sq, sq))  # no cancellation
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = q, np.where(q != 0, cc / q, np.nan)
    return np.minimum(ta, tb), np.maximum(ta, tb)


def second_hop64(eye, M, NM, C, R, tmin=0.001):
    """fp64: the ray from eye through M reflected about NM; per ray the sorted
    offers of all spheres (the entering root if past t_min, else the exiting
    one; inf = none), their order, the reflected direction and, per sphere,
    how far the line passes from its surface."""
    d = M - eye
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    n = NM / np.linalg.norm(NM, axis=-1, keepdims=True)
    r = d - 2.0 * (d * n).sum(-1, keepdims=True) * n
    r /= np.linalg.norm(r, axis=-1, keepdims=True)
    a0, a1 = roots64(M[:, None, :], r[:, None, :], C[None, :, :], R[None, :])
    with np.errstate(invalid="ignore"):
        offer = np.where(a0 > tmin, a0, a1)
        offer = np.where(np.isnan(offer) | (offer <= tmin), np.inf, offer)
    oc = M[:, None, :] - C[None, :, :]
    along = (oc * r[:, None, :]).sum(-1)
    perp = np.sqrt(np.maximum((oc * oc).sum(-1) - along * along, 0.0))
    limb = np.where(along < 0, np.abs(perp - np.abs(R)[None, :]), np.inf)  # spheres ahead of the ray only
    return offer, r, limb


def left_out64(offer, limb, tol):
    """Rays whose two nearest offers are within tol (relative: tol / t), or
    that pass a limb within tol: fp32 and fp64 may pick different spheres."""
    srt = np.sort(offer, axis=-1)
    t = srt[:, 0]
    with np.errstate(invalid="ignore"):
        close = np.isfinite(srt[:, 1]) & ((srt[:, 1] - t) < tol)
    return close | (limb.min(-1) < tol) | ~np.isfinite(t)
