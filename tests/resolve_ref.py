"""numpy float32 restatement of the clamped temporal resolve with centre
reprojection (include/rt_resolve.h, "Semantics"): the same operations in the
same order as csrc/rt_resolve.hip, vectorised over pixels, looping over the
nine neighbourhood pixels and the four taps in the specified order.  Every
intermediate is a float32 array, so each numpy operation rounds once, like the
kernel's (no contraction there): the two agree bit for bit.

The projection, the gather, the blend and the history packing are
temporal_ref's (csrc/rt_reproject.h on the device); the guide preparation is
post_ref's.  The options are the EFFECTIVE ones (after the
desc's "0 = default" rule): plane_tol inf = plane test off, normal_cos -1 =
normal test off, gamma inf = clamp off."""
from collections import namedtuple

import numpy as np

import temporal_ref as tref
from post_ref import F, _dot, guides

DEFAULTS = dict(max_len=2, plane_tol=0.003, normal_cos=0.9, gamma=1.0)
KEEP_PARTIAL = 1

# rt_resolve_rays; anything with these attributes (rtow.ResolveRays too) is a set of rays here
Rays = namedtuple("Rays", "eye d00 du dv")
# The identity pair: rays and a view that take pixel (i, j) to the point (i 2^-20, j 2^-20, 1) at depth 1
# and back to (i, j) EXACTLY.  The steps are that small so that D.D rounds to 1 for every pixel of a small
# frame ((i^2 + j^2) 2^-40 is far below half an ulp of 1): dl = 1, u = D and P = u hold exactly, and the
# view's x = (2^20 * P.x) / 1 is the integer i.  With rays (i, j, 1) and temporal_ref.IDENTITY the
# normalisation D / |D| would round, x would miss i by an ulp, and no property would be exact.
STEP = 2.0 ** -20
IDENTITY_RAYS = Rays(eye=(0.0, 0.0, 0.0), d00=(0.0, 0.0, 1.0), du=(STEP, 0.0, 0.0), dv=(0.0, STEP, 0.0))
IDENTITY_VIEW = tref.View(eye=(0.0, 0.0, 0.0), px=(1 / STEP, 0.0, 0.0), py=(0.0, 1 / STEP, 0.0), pw=(0.0, 0.0, 1.0),
                          x0=0.0, y0=0.0)


def _v3(v):
    return np.array([v[0], v[1], v[2]], F)


def centre_rays(rays, w, h):
    """D (h, w, 3) float32: (d00 + float(i) * du) + float(j) * dv."""
    jj, ii = np.mgrid[0:h, 0:w].astype(F)
    D = (_v3(rays.d00) + ii[..., None] * _v3(rays.du)) + jj[..., None] * _v3(rays.dv)
    assert D.dtype == F
    return D


def prepare(cur, hits, depth, normal, spp, rays):
    """Step 1 -> (c, n, P, sky)."""
    cur, depth, normal = (np.asarray(a, F) for a in (cur, depth, normal))
    hits = np.asarray(hits, np.uint32)
    H, W = hits.shape
    c = (cur / F(spp)).astype(F)
    n, _, sky = guides(normal, np.zeros_like(normal), hits)
    D = centre_rays(rays, W, H)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tm = depth / hits.astype(F)
        dl = np.sqrt(_dot(D, D))
        u = D / dl[..., None]
        P = _v3(rays.eye) + u * tm[..., None]
    assert tm.dtype == F and u.dtype == F and P.dtype == F
    P = np.where(sky[..., None], F(0), P).astype(F)
    return c, n, P, sky


def neighbourhood(c, gamma):
    """Step 2 -> (lo, hi, k): per channel mean -+ gamma * sd over the up to
    nine pixels around each pixel, dy outer, dx inner, and their number."""
    H, W, _ = c.shape
    m1, m2, k = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F), np.zeros((H, W), F)
    yy, xx = np.mgrid[0:H, 0:W]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ty, tx = yy + dy, xx + dx
            inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
            cq = c[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
            m1 = np.where(inside[..., None], m1 + cq, m1)
            m2 = np.where(inside[..., None], m2 + cq * cq, m2)
            k = np.where(inside, k + F(1), k)
    mu = m1 / k[..., None]
    v = m2 / k[..., None] - mu * mu
    v = np.where(v > 0, v, F(0))
    sd = np.sqrt(v)
    lo, hi = mu - F(gamma) * sd, mu + F(gamma) * sd
    assert lo.dtype == F and hi.dtype == F and sd.dtype == F
    return lo, hi, k


def resolve_ref(cur, hits, depth, normal, spp, rays, prev=None, history=None, max_len=2, plane_tol=0.003,
                normal_cos=0.9, gamma=1.0, flags=0, census=None):
    """cur, normal (H, W, 3) float32 sums, hits (H, W) uint32, depth (H, W)
    float32 sums, rays the frame's centre rays, history (3, H, W, 4) float32 or
    None, prev a view -> (out (H, W, 3), history_out (3, H, W, 4)).  census (a
    dict, optional) receives what the pixels, their taps and the clamp did."""
    c, n, P, sky = prepare(cur, hits, depth, normal, spp, rays)
    hits = np.asarray(hits, np.uint32)
    H, W = sky.shape
    m = c.copy()
    ln = np.ones((H, W), F)
    if census is not None:
        census.clear()
    if history is not None:
        partial = ~sky & (hits < np.uint32(spp))
        use = ~sky & (~partial if not flags & KEEP_PARTIAL else True)
        # 4. reproject and gather: rt_temporal.h's steps 3 and 4 with this P and n
        sw, sc, sl, ok, did = tref.gather(history, prev, P, n, use, plane_tol, normal_cos)
        # 5. clamp and blend
        valid = ok & (sw > 0)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            raw = sc / sw[..., None]
            hist = raw
            if np.isfinite(gamma):
                lo, hi, k = neighbourhood(c, gamma)
                hist = np.where(raw < lo, lo, np.where(raw > hi, hi, raw))
            mv, lv, t = tref.blend(c, hist, sl / sw, max_len)
        assert hist.dtype == F
        m = np.where(valid[..., None], mv, c)
        ln = np.where(valid, lv, F(1)).astype(F)
        if census is not None:
            census.update(did, valid=valid, use=use, partial=partial, saturated=valid & (t >= F(max_len)), hist=hist)
            if np.isfinite(gamma):
                v3 = valid[..., None]
                census.update(lo=lo, hi=hi, k=k, clamp_low=v3 & (raw < lo), clamp_high=v3 & ~(raw < lo) & (raw > hi),
                              clamp_idle=v3 & ~(raw < lo) & ~(raw > hi))
    out = m * F(spp)
    assert out.dtype == F
    return out, tref.pack_history(m, ln, P, sky, n)


def identity_inputs(w, h, spp, colour, hits=None):
    """Inputs that IDENTITY_RAYS and IDENTITY_VIEW map to their own pixel
    exactly: depth 1, n = (0, 0, 1), every sample a hit (or `hits`, (h, w)).
    colour: (h, w, 3) means; the sums are x spp."""
    hits = np.full((h, w), spp, np.uint32) if hits is None else np.asarray(hits, np.uint32)
    hf = hits.astype(F)
    return dict(cur=(np.asarray(colour, F) * F(spp)).astype(F), hits=hits, depth=hf.copy(),
                normal=(np.array([0, 0, 1], F) * hf[..., None]).astype(F))


def identity_positions(w, h, spp):
    """The position sums temporal_ref needs to see the same points as
    identity_inputs (every sample a hit): (i STEP, j STEP, 1) x spp."""
    yy, xx = np.mgrid[0:h, 0:w].astype(F)
    return (np.stack([xx * F(STEP), yy * F(STEP), np.ones_like(xx)], -1) * F(spp)).astype(F)


def synthetic_inputs(w, h, spp=4, seed=0, max_len=32):
    """-> (frame, history, view, rays): temporal_ref.synthetic_inputs' frame,
    history and previous view (see there for what they hold), with the frame's
    position sums replaced by depth sums and centre rays that put the same
    geometry under the pixel centres: the eye at (0, 0, 30), pixel (col, row)'s
    ray through (0.37 col, 0.21 row, 0), the depth the distance to that ray's
    point on the pixel's plane (+- 1e-4).  The positions behind the previous eye
    (w <= 0) become negative depths.  Pixel (0, 0), the one corner the view
    keeps on the frame, is made to find history (fully covered, its tap on its
    plane), so that a neighbourhood of four pixels is reached whatever the seed."""
    frame, hist, view = tref.synthetic_inputs(w, h, spp, seed, max_len)
    rng = np.random.default_rng(seed + 7919)
    yy, xx = np.mgrid[0:h, 0:w]
    X, Y = 0.37 * xx, 0.21 * yy
    left = xx < (w + 1) // 2
    s = np.where(left, 30.0 / (30.0 - 0.02 * X), 31.0 / (30.0 - 0.03 * Y))
    dist = s * np.sqrt(X * X + Y * Y + 900.0) + rng.normal(0, 1e-4, (h, w))
    hits = frame["hits"].copy()
    hits[0, 0] = spp
    behind = (rng.random((h, w)) < 0.03) & (hits > 0)
    behind[0, 0] = False
    normal = frame["normal"].copy()
    n00 = np.array([0.02, 0.0, 1.0]) / np.linalg.norm([0.02, 0.0, 1.0])
    normal[0, 0] = n00.astype(F) * F(spp)
    depth = (np.where(behind, -dist, dist).astype(F) * hits.astype(F)).astype(F)
    hist = hist.copy()
    hist[1, 0, 0] = (0.0, 0.0, 1e-4, 0.0)
    hist[2, 0, 0, :3] = n00
    rays = Rays(eye=(0.0, 0.0, tref.SYNTH_EYE_Z), d00=(0.0, 0.0, -tref.SYNTH_EYE_Z), du=(0.37, 0.0, 0.0),
                dv=(0.0, 0.21, 0.0))
    return dict(cur=frame["cur"].copy(), hits=hits, depth=depth, normal=normal), hist, view, rays
