"""numpy float32 restatement of the guided a-trous denoiser (include/rt_denoise.h,
"Semantics"): the same operations in the same order as csrc/rt_denoise.hip,
vectorised over pixels, looping over the 25 taps in the specified order.  Every
intermediate is a float32 array, so each numpy operation rounds once, like the
kernel's (no contraction there): the two agree bit for bit.

The options are the EFFECTIVE ones (after the desc's "0 = default" rule):
normal_power 0 = no squaring, sigma_plane inf = term off, sigma_color 0 = term
off."""
import numpy as np

from post_ref import F, _dot, guides

K = (F(1 / 16), F(4 / 16), F(6 / 16), F(4 / 16), F(1 / 16))
DEFAULTS = dict(iterations=5, normal_power=6, sigma_plane=0.5, sigma_color=0.15)


def demod(albedo, hits, spp):
    """max(a, 1e-3f) per channel, a = (albedo_sum + float(spp - h)) / spp."""
    miss = (np.int64(spp) - hits.astype(np.int64)).astype(F)
    a = (albedo + miss[..., None]) / F(spp)
    return np.where(a > F(1e-3), a, F(1e-3)).astype(F)


def prepare(beauty, hits, position, normal, albedo, spp):
    """-> (u, n, P, sky, m): demodulated colour, unit normal, mean position,
    sky mask, and the albedo m the colour was divided by."""
    beauty, position, normal, albedo = (np.asarray(x, F) for x in (beauty, position, normal, albedo))
    hits = np.asarray(hits, np.uint32)
    m = demod(albedo, hits, spp)
    u = (beauty / F(spp)) / m
    n, P, sky = guides(normal, position, hits)
    return u.astype(F), n, P, sky, m


def iteration(u, n, P, sky, step, normal_power, sigma_plane, sigma2):
    """One a-trous pass at `step`; sigma2 = (sigma_color * 2^-i)^2 as float32, 0 = off."""
    H, W = sky.shape
    acc = np.zeros((H, W, 3), F)
    wsum = np.zeros((H, W), F)
    sigma_plane = F(sigma_plane)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            # the output pixels p whose tap q = p + (ox, oy) is inside the frame
            y0, y1 = max(0, -oy), min(H, H - oy)
            x0, x1 = max(0, -ox), min(W, W - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            ps = (slice(y0, y1), slice(x0, x1))
            qs = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            kk = K[dx + 2] * K[dy + 2]
            uq = u[qs]
            if dx == 0 and dy == 0:
                acc[ps] += kk * uq
                wsum[ps] += kk
                continue
            n_p, n_q, P_p, P_q, u_p = n[ps], n[qs], P[ps], P[qs], u[ps]
            both, one = sky[ps] & sky[qs], sky[ps] != sky[qs]
            wn = _dot(n_p, n_q)
            wn = np.where(wn > 0, wn, F(0)).astype(F)
            for _ in range(normal_power):
                wn = wn * wn
            wn = np.where(one, F(0), wn)
            wn = np.where(both, F(1), wn).astype(F)
            D = P_q - P_p
            dd = _dot(D, D)
            nd = _dot(n_p, D)
            with np.errstate(divide="ignore", invalid="ignore"):
                wp = F(1) - (np.abs(nd) / np.sqrt(dd)) / sigma_plane
            wp = np.where(wp > 0, wp, F(0))
            wp = np.where(dd > 0, wp, F(1))
            wp = np.where(both, F(1), wp).astype(F)
            if sigma2 != 0:
                e = u_p - uq
                d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                wc = F(1) / (F(1) + d / F(sigma2))
            else:
                wc = np.ones_like(wn)
            w = ((kk * wn) * wp) * wc
            assert w.dtype == F
            acc[ps] += w[..., None] * uq
            wsum[ps] += w
    return acc / wsum[..., None]


def synthetic_inputs(w, h, spp=16, seed=0):
    """A seeded frame with everything the filter branches on: a sky band on
    top (hits 0, zero sums), partially covered pixels (0 < hits < spp), two
    tilted planes with different normals and albedos (one with a zero albedo
    channel), a few pixels whose normals cancel to a zero sum, and noisy
    colour.  Sums as rt_render / rt_aov give them: float32, hits uint32."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    hits = rng.integers(1, spp + 1, (h, w)).astype(np.uint32)
    hits[rng.random((h, w)) < 0.6] = spp
    sky = yy < (h + 2) // 4 + (xx % 3 == 0)
    if h * w > 1:
        hits[sky] = 0
    left = xx < (w + 1) // 2
    unit = np.where(left[..., None], np.float32((0.6, 0.0, 0.8)), np.float32((0.0, 0.28, 0.96)))
    nrm = unit + rng.normal(0, 0.02, (h, w, 3))
    pos = np.stack([xx * 0.37, yy * 0.21, np.where(left, -0.75 * xx * 0.37, -0.29 * yy * 0.21)], -1)
    pos = pos + rng.normal(0, 0.003, (h, w, 3))
    alb = np.where(left[..., None], np.float32((0.8, 0.0, 0.3)), np.float32((0.2, 0.9, 0.6)))
    hf = hits.astype(F)[..., None]
    nrm, pos, alb = ((a.astype(F) * hf).astype(F) for a in (nrm, pos, alb))
    cancel = (rng.random((h, w)) < 0.04) & (hits > 0)
    nrm[cancel] = 0
    beauty = (rng.gamma(2.0, 0.25, (h, w, 3)) * (0.2 + alb / np.maximum(hf, 1))).astype(F) * F(spp)
    beauty[hits == 0] = (F((0.6, 0.75, 1.0)) * F(spp) + rng.normal(0, 0.01, 3).astype(F))
    return dict(beauty=np.ascontiguousarray(beauty, F), hits=hits, position=pos, normal=nrm, albedo=alb)


def sigma2_of(sigma_color, i):
    sg = F(sigma_color) * (F(1) / F(1 << i))
    return sg * sg


def filter_u(u, n, P, sky, iterations=5, normal_power=6, sigma_plane=0.5, sigma_color=0.15):
    """The iterations alone, on prepared buffers."""
    for i in range(iterations):
        u = iteration(u, n, P, sky, 1 << i, normal_power, sigma_plane, sigma2_of(sigma_color, i))
    return u


def denoise_ref(beauty, hits, position, normal, albedo, spp, iterations=5, normal_power=6, sigma_plane=0.5,
                sigma_color=0.15):
    """beauty, position, normal, albedo (H, W, 3) float32 sums, hits (H, W)
    uint32 -> the filtered sums (H, W, 3) float32."""
    u, n, P, sky, m = prepare(beauty, hits, position, normal, albedo, spp)
    u = filter_u(u, n, P, sky, iterations, normal_power, sigma_plane, sigma_color)
    out = (u * m) * F(spp)
    assert out.dtype == F
    return out
