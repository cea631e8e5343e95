"""numpy float32 restatement of guided upsampling (include/rt_upscale.h,
"Semantics"): the same operations in the same order as csrc/rt_upscale.hip,
vectorised over pixels, looping over the taps in the specified order.  Every
intermediate is a float32 array, so each numpy operation rounds once, like the
kernels' (no contraction there): the two agree bit for bit.

The guide preparation is post_ref's, the demodulation denoise_ref's, the rays
resolve_ref's, the projection temporal_ref's.  The options are the EFFECTIVE
ones (after the desc's "0 = default" rule): plane_tol inf = plane test off,
normal_cos -1 = normal test off."""
import numpy as np

import temporal_ref as tref
from denoise_ref import demod
from post_ref import F, _dot, guides
from resolve_ref import Rays, _v3, centre_rays

DEFAULTS = dict(plane_tol=0.1, normal_cos=-0.5)
NO_ALBEDO = 1
AOV = ("hits", "position", "normal", "albedo")


def prepare(hits, position, normal, albedo, spp, flags):
    """-> (n, P, sky, m) of one frame's rt_aov sums."""
    hits = np.asarray(hits, np.uint32)
    n, P, sky = guides(np.asarray(normal, F), np.asarray(position, F), hits)
    if flags & NO_ALBEDO:
        m = np.ones(hits.shape + (3,), F)
    else:
        m = demod(np.asarray(albedo, F), hits, spp)
    return n, P, sky, m


def planes(cur, lo, lo_spp, flags=0):
    """Launch 1 -> the scratch, (3, h, w, 4) float32."""
    n, P, sky, m = prepare(lo["hits"], lo["position"], lo["normal"], lo.get("albedo"), lo_spp, flags)
    u = (np.asarray(cur, F) / F(lo_spp)) / m
    assert u.dtype == F
    out = np.zeros((3,) + sky.shape + (4,), F)
    out[0, ..., :3], out[0, ..., 3] = u, sky
    out[1, ..., :3] = P
    out[2, ..., :3] = n
    return out


def map_pixels(lo_view, rays, w, h, W, H):
    """Step 2 -> (xi, yi, fx, fy, x_raw, y_raw): where the output's pixels lie
    in the low-resolution frame."""
    D = centre_rays(rays, W, H)
    _, xr, yr = tref.project_rel(lo_view, D)
    with np.errstate(invalid="ignore"):
        x = np.where(xr > 0, xr, F(0))
        x = np.where(x < F(w - 1), x, F(w - 1))
        y = np.where(yr > 0, yr, F(0))
        y = np.where(y < F(h - 1), y, F(h - 1))
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    assert x.dtype == y.dtype == fx.dtype == fy.dtype == F
    return xf.astype(np.int64), yf.astype(np.int64), fx, fy, xr, yr


def upscale_ref(cur, lo, hi, lo_spp, spp, lo_view, rays, plane_tol=0.1, normal_cos=-0.5, flags=0, census=None):
    """cur (h, w, 3) float32 sums, lo / hi dicts of the two frames' rt_aov sums
    (AOV; albedo not read with NO_ALBEDO) -> (out (H, W, 3) float32, stage
    (H, W) uint8).  census (a dict, optional) receives what the pixels and
    their taps did."""
    assert tuple(F(v) for v in rays.eye) == tuple(F(v) for v in lo_view.eye)
    pl = planes(cur, lo, lo_spp, flags)
    h, w = pl.shape[1:3]
    n, P, sky, m = prepare(hi["hits"], hi["position"], hi["normal"], hi.get("albedo"), spp, flags)
    H, W = sky.shape
    xi, yi, fx, fy, xr, yr = map_pixels(lo_view, rays, w, h, W, H)
    q = P - _v3(rays.eye)
    pt2 = F(plane_tol) * F(plane_tol)
    with np.errstate(invalid="ignore", over="ignore"):
        lim = pt2 * _dot(q, q)
    count = dict(left=0, right=0, top=0, bottom=0, sky_on_surface=0, surface_on_sky=0, plane=0, normal=0)

    def tap(tx, ty, guided, active):
        inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
        txc, tyc = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
        c0, Pt, nt = pl[0, tyc, txc], pl[1, tyc, txc], pl[2, tyc, txc]
        if not guided:
            return inside, c0[..., :3]
        tsky = c0[..., 3] != 0
        same = tsky == sky
        with np.errstate(invalid="ignore", over="ignore"):
            e = _dot(n, Pt[..., :3] - P)
            plane = (e * e <= lim) if np.isfinite(plane_tol) else np.ones((H, W), bool)
            g = _dot(n, nt[..., :3])
        facing = (g >= F(normal_cos)) if normal_cos != -1 else np.ones((H, W), bool)
        valid = inside & same & (sky | (plane & facing))
        count["left"] += int((active & (tx < 0)).sum())
        count["right"] += int((active & (tx >= w)).sum())
        count["top"] += int((active & (ty < 0)).sum())
        count["bottom"] += int((active & (ty >= h)).sum())
        surf = active & inside & ~sky
        count["sky_on_surface"] += int((surf & tsky).sum())
        count["surface_on_sky"] += int((active & inside & sky & ~tsky).sum())
        count["plane"] += int((surf & same & ~plane).sum())
        count["normal"] += int((surf & same & plane & ~facing).sum())
        return valid, c0[..., :3]

    def bilinear(guided, active):
        sw, sc = np.zeros((H, W), F), np.zeros((H, W, 3), F)
        taken, zero_b = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
        for dy in (0, 1):
            for dx in (0, 1):
                valid, u = tap(xi + dx, yi + dy, guided, active)
                b = (fx if dx else F(1) - fx) * (fy if dy else F(1) - fy)
                assert b.dtype == F
                sw = np.where(valid, sw + b, sw)
                sc = np.where(valid[..., None], sc + b[..., None] * u, sc)
                taken += valid
                zero_b |= valid & (b == 0)
        return sw, sc, taken, zero_b

    everywhere = np.ones((H, W), bool)
    sw, sc, taken1, zero_b = bilinear(True, everywhere)
    stage = np.ones((H, W), np.uint8)
    need2 = ~(sw > 0)
    sw2, sc2 = np.zeros((H, W), F), np.zeros((H, W, 3), F)
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            valid, u = tap(xi + dx, yi + dy, True, need2)
            sw2 = np.where(valid, sw2 + F(1), sw2)
            sc2 = np.where(valid[..., None], sc2 + u, sc2)
    need3 = need2 & ~(sw2 > 0)
    sw3, sc3, _, _ = bilinear(False, need3)
    stage[need2] = 2
    stage[need3] = 3
    sw = np.where(need3, sw3, np.where(need2, sw2, sw))
    sc = np.where(need3[..., None], sc3, np.where(need2[..., None], sc2, sc))
    assert (sw > 0).all()
    with np.errstate(over="ignore", invalid="ignore"):
        out = ((sc / sw[..., None]) * m) * F(lo_spp)
    assert out.dtype == F
    if census is not None:
        census.clear()
        census.update(count, stage=stage, taken1=taken1, zero_b_to_stage2=need2 & zero_b, x=xr, y=yr, xi=xi, yi=yi,
                      fx=fx, fy=fy, sky=sky, m=m, m_lo=prepare(lo["hits"], lo["position"], lo["normal"],
                                                                 lo.get("albedo"), lo_spp, flags)[3])
    return out, stage


def plain_bilinear(cur, lo_spp, lo_view, rays, W, H):
    """The plain filter the quality test compares with: the bilinear mix of the
    in-frame taps at the pass's own (x, y), in float64 -> means (H, W, 3)."""
    c = np.asarray(cur, np.float64) / lo_spp
    h, w = c.shape[:2]
    xi, yi, fx, fy, _, _ = map_pixels(lo_view, rays, w, h, W, H)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    sw, sc = np.zeros((H, W)), np.zeros((H, W, 3))
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = xi + dx, yi + dy
            inside = (tx < w) & (ty < h)
            b = np.where(inside, (fx if dx else 1 - fx) * (fy if dy else 1 - fy), 0.0)
            sw += b
            sc += b[..., None] * c[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]
    return sc / sw[..., None]


# ---- inputs ----------------------------------------------------------------------
SX, SY = 0.37, 0.21  # world size of a low-resolution pixel
EYE_Z = tref.SYNTH_EYE_Z
X0 = 0.3


def frame_pair(w, h, W, H):
    """-> (lo_view, rays, lo_xy, hi_xy): an eye at (0, 0, EYE_Z) looking down
    -z.  The view puts the world point (X, Y, 0) at the low-resolution pixel
    (X / SX - X0, Y / SY - X0); the rays of the output frame pass through
    (a i + ox, c j + oy, 0), a grid 1.1 times the low-resolution frame's
    extent that starts 0.05 w + 0.4 pixels before it: fractional coordinates
    everywhere, and off the frame on every border (both clamps).  lo_xy, hi_xy:
    the world (X, Y) under the two frames' pixels, (rows, cols, 2) float64."""
    a, c = 1.1 * SX * w / W, 1.1 * SY * h / H
    ox, oy = SX * (X0 - 0.05 * w - 0.4), SY * (X0 - 0.05 * h - 0.4)
    view = tref.View(eye=(0.0, 0.0, EYE_Z), px=(1 / SX, 0.0, 0.0), py=(0.0, 1 / SY, 0.0), pw=(0.0, 0.0, -1.0 / EYE_Z),
                     x0=X0, y0=X0)
    rays = Rays(eye=(0.0, 0.0, EYE_Z), d00=(ox, oy, -EYE_Z), du=(a, 0.0, 0.0), dv=(0.0, c, 0.0))
    ty, tx = np.mgrid[0:h, 0:w]
    jj, ii = np.mgrid[0:H, 0:W]
    return view, rays, np.stack([SX * (tx + X0), SY * (ty + X0)], -1), np.stack([a * ii + ox, c * jj + oy], -1)


def synthetic_inputs(w, h, W, H, lo_spp=4, spp=8, seed=0):
    """-> dict(cur, lo, hi, lo_view, rays, lo_spp, spp): a seeded pair of
    frames that reaches everything the pass branches on.  Two planes with a
    depth step of 5 between them (left: z = -0.02 X, right: z = -5 - 0.03 Y)
    under both frames (frame_pair).  Both frames have scattered sky pixels,
    partially covered pixels, pixels whose normals cancel and pixels with a
    black albedo (m at its 1e-3 floor); a block that is sky in both frames, a
    block that is sky in the low-resolution frame only and scattered sky
    pixels in the output only (stage 3 from both sides).  The low-resolution
    positions are off their plane by 1e-4 (kept by every tolerance), by 0.005
    (kept by the default 0.1 x 30, rejected by 1e-4 x 30) or by 5 (rejected by
    all); a tenth of its normals is turned by 90 degrees and another by 16
    (cos 0 and 0.96: kept by the default -0.5, rejected by 0.99), a twentieth
    is flipped (cos -1: rejected by the default too)."""
    rng = np.random.default_rng(seed)
    view, rays, lo_xy, hi_xy = frame_pair(w, h, W, H)
    xmid = SX * w / 2

    def geometry(xy):
        X, Y = xy[..., 0], xy[..., 1]
        left = X < xmid
        z = np.where(left, -0.02 * X, -5.0 - 0.03 * Y)
        nrm = np.where(left[..., None], np.array([0.02, 0.0, 1.0]), np.array([0.0, 0.03, 1.0]))
        return np.stack([X, Y, z], -1), nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)

    def in_block(xy, x0, x1, y0, y1):  # in units of the low-resolution frame's extent
        fx, fy = xy[..., 0] / (SX * w), xy[..., 1] / (SY * h)
        return (fx >= x0) & (fx < x1) & (fy >= y0) & (fy < y1)

    def frame(xy, s, extra_sky, scattered):
        rows, cols = xy.shape[:2]
        yy, xx = np.mgrid[0:rows, 0:cols]
        hits = rng.integers(1, s + 1, (rows, cols)).astype(np.uint32)
        hits[rng.random((rows, cols)) < 0.6] = s
        sky = in_block(xy, 0.15, 0.4, 0.55, 0.9) | extra_sky | (((3 * xx + 5 * yy + 1) % scattered) == 0)
        hits[sky] = 0
        pos, nrm = geometry(xy)
        pos = pos + rng.normal(0, 1e-4, (rows, cols, 3))
        alb = rng.random((rows, cols, 3)) * 0.9 + 0.05
        alb[(rng.random((rows, cols)) < 0.05)] = 0.0
        black = (alb == 0).all(-1)
        hits[black & ~sky] = s  # (a covered black pixel: a = 0, m = 1e-3)
        return hits, sky, pos, nrm, alb

    lo_hits, lo_sky, lo_pos, lo_nrm, lo_alb = frame(lo_xy, lo_spp, in_block(lo_xy, 0.6, 0.85, 0.1, 0.5), 13)
    hi_hits, hi_sky, hi_pos, hi_nrm, hi_alb = frame(hi_xy, spp, np.zeros((H, W), bool), 17)
    kind = rng.random((h, w))
    lo_pos[..., 2] += np.where(kind < 0.7, 0.0, np.where(kind < 0.85, 0.005, 5.0)) * rng.choice([-1.0, 1.0], (h, w))
    turn = rng.random((h, w))
    lo_nrm[turn < 0.1] = np.array([1.0, 0.0, 0.0])
    tilt = (turn >= 0.1) & (turn < 0.2)
    lo_nrm[tilt] = np.array([np.sin(np.radians(16.0)), 0.0, np.cos(np.radians(16.0))])
    flip = (turn >= 0.2) & (turn < 0.25)
    lo_nrm[flip] = -lo_nrm[flip]

    def sums(hits, pos, nrm, alb, cancel):
        hf = hits.astype(F)[..., None]
        normal = (nrm.astype(F) * hf).astype(F)
        normal[cancel & (hits > 0)] = 0
        return dict(hits=hits, position=(pos.astype(F) * hf).astype(F), normal=normal,
                    albedo=(alb.astype(F) * hf).astype(F))

    lo = sums(lo_hits, lo_pos, lo_nrm, lo_alb, rng.random((h, w)) < 0.04)
    hi = sums(hi_hits, hi_pos, hi_nrm, hi_alb, rng.random((H, W)) < 0.04)
    cur = (rng.gamma(2.0, 0.25, (h, w, 3)).astype(F) * F(lo_spp)).astype(F)
    return dict(cur=cur, lo=lo, hi=hi, lo_view=view, rays=rays, lo_spp=lo_spp, spp=spp)
