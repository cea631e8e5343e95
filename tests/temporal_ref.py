"""numpy float32 restatement of temporal accumulation with reprojection
(include/rt_temporal.h, "Semantics"): the same operations in the same order as
csrc/rt_temporal.hip, vectorised over pixels, looping over the four taps in the
specified order.  Every intermediate is a float32 array, so each numpy
operation rounds once, like the kernel's (no contraction there): the two agree
bit for bit.

The options are the EFFECTIVE ones (after the desc's "0 = default" rule):
plane_tol inf = plane test off, normal_cos -1 = normal test off."""
from collections import namedtuple

import numpy as np

from post_ref import F, _dot, guides

DEFAULTS = dict(max_len=2, plane_tol=0.0003, normal_cos=0.9)

# rt_temporal_view; anything with these attributes (rtow.TemporalView too) is a view here
View = namedtuple("View", "eye px py pw x0 y0")
IDENTITY = View(eye=(0.0, 0.0, 0.0), px=(1.0, 0.0, 0.0), py=(0.0, 1.0, 0.0), pw=(0.0, 0.0, 1.0), x0=0.0, y0=0.0)


def _v3(v):
    return np.array([v[0], v[1], v[2]], F)


def project_rel(view, q):
    """The header's "View" in float32 for vectors relative to the eye: q
    (..., 3) -> (w, x, y)."""
    q = np.asarray(q, F)
    w = _dot(_v3(view.pw), q)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = _dot(_v3(view.px), q) / w - F(view.x0)
        y = _dot(_v3(view.py), q) / w - F(view.y0)
    assert q.dtype == w.dtype == x.dtype == y.dtype == F
    return w, x, y


def project(view, P):
    """The same for points: P (..., 3) -> (q, w, x, y) with q = P - eye."""
    q = np.asarray(P, F) - _v3(view.eye)
    return (q,) + project_rel(view, q)


def prepare(cur, hits, position, normal, spp):
    """-> (c, n, P, sky): mean colour, unit normal, mean position, sky mask."""
    cur, position, normal = (np.asarray(a, F) for a in (cur, position, normal))
    hits = np.asarray(hits, np.uint32)
    c = cur / F(spp)
    n, P, sky = guides(normal, position, hits)
    return c.astype(F), n, P, sky


def gather(history, prev, P, n, use, plane_tol, normal_cos):
    """Steps 3 and 4 for the pixels of the mask `use`: P (H, W, 3) projected
    through prev and the four taps around it, dy outer, dx inner -> (sw (H, W),
    sc (H, W, 3), sl (H, W), ok, census): the bilinear sums of the taps on the
    pixel's surface, the pixels whose projection lies on the frame, and what
    the pixels and their taps did (masks and counts)."""
    history = np.asarray(history, F)
    H, W = use.shape
    assert history.shape == (3, H, W, 4)
    q, w, x, y = project(prev, P)
    ok = use & (w > 0) & (x > F(-1)) & (x < F(W)) & (y > F(-1)) & (y < F(H))
    xs, ys = np.where(ok, x, F(0)), np.where(ok, y, F(0))  # (the rest is never used)
    xf, yf = np.floor(xs), np.floor(ys)
    fx, fy = xs - xf, ys - yf
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    d2 = _dot(q, q)
    pt2 = F(plane_tol) * F(plane_tol)
    with np.errstate(invalid="ignore", over="ignore"):
        lim = pt2 * d2
    sw, sl, sc = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W, 3), F)
    taken = np.zeros((H, W), np.int64)
    count = dict(off_frame=0, sky_tap=0, plane=0, normal=0)
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = xi + dx, yi + dy
            inside = ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            txc, tyc = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            rgbl, Pt, nt = history[0, tyc, txc], history[1, tyc, txc], history[2, tyc, txc]
            geo = inside & (Pt[..., 3] == 0)
            with np.errstate(invalid="ignore", over="ignore"):
                e = _dot(n, Pt[..., :3] - P)
                plane = (e * e <= lim) if np.isfinite(plane_tol) else np.ones((H, W), bool)
                g = _dot(n, nt[..., :3])
            same = (g >= F(normal_cos)) if normal_cos != -1 else np.ones((H, W), bool)
            take = geo & plane & same
            b = (fx if dx else F(1) - fx) * (fy if dy else F(1) - fy)
            assert b.dtype == F
            with np.errstate(invalid="ignore", over="ignore"):
                sw = np.where(take, sw + b, sw)
                sc = np.where(take[..., None], sc + b[..., None] * rgbl[..., :3], sc)
                sl = np.where(take, sl + b * rgbl[..., 3], sl)
            taken += take
            count["off_frame"] += int((ok & ~inside).sum())
            count["sky_tap"] += int((inside & ~geo).sum())
            count["plane"] += int((geo & ~plane).sum())
            count["normal"] += int((geo & plane & ~same).sum())
    return sw, sc, sl, ok, dict(count, ok=ok, taken=taken, w=w, x=x, y=y, xi=xi, yi=yi)


def blend(c, hist, hl, max_len):
    """Step 5 -> (mv, lv, t): the history's mean colour hist (clamped by the
    caller where it clamps) and length hl blended with the new colour c, the new
    length, and the length before its cap."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = hl + F(1)
        lv = np.where(t < F(max_len), t, F(max_len)).astype(F)
        a = F(1) / lv
        mv = hist + (c - hist) * a[..., None]
    assert mv.dtype == F and lv.dtype == F
    return mv, lv, t


def pack_history(m, ln, P, sky, n):
    """Step 6 -> history_out (3, H, W, 4)."""
    hout = np.zeros((3,) + sky.shape + (4,), F)
    hout[0, ..., :3], hout[0, ..., 3] = m, ln
    hout[1, ..., :3], hout[1, ..., 3] = P, sky
    hout[2, ..., :3] = n
    return hout


def temporal_ref(cur, hits, position, normal, spp, prev=None, history=None, max_len=2, plane_tol=0.0003,
                 normal_cos=0.9, census=None):
    """cur, position, normal (H, W, 3) float32 sums, hits (H, W) uint32, history
    (3, H, W, 4) float32 or None, prev a view -> (out (H, W, 3), history_out
    (3, H, W, 4)).  census (a dict, optional) receives what the pixels and
    their taps did: masks and counts for the tests that ask whether their
    inputs reach every branch."""
    c, n, P, sky = prepare(cur, hits, position, normal, spp)
    m = c.copy()
    ln = np.ones(sky.shape, F)
    if census is not None:
        census.clear()
    if history is not None:
        sw, sc, sl, ok, did = gather(history, prev, P, n, ~sky, plane_tol, normal_cos)
        valid = ok & (sw > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            mv, lv, t = blend(c, sc / sw[..., None], sl / sw, max_len)
        m = np.where(valid[..., None], mv, c)
        ln = np.where(valid, lv, F(1)).astype(F)
        if census is not None:
            census.update(did, valid=valid, saturated=valid & (t >= F(max_len)))
    out = m * F(spp)
    assert out.dtype == F
    return out, pack_history(m, ln, P, sky, n)


def orbit(lookfrom, lookat, degrees):
    """lookfrom turned about the vertical axis through lookat."""
    a = np.radians(degrees)
    d = np.asarray(lookfrom, np.float64) - np.asarray(lookat, np.float64)
    r = np.array([d[0] * np.cos(a) + d[2] * np.sin(a), d[1], -d[0] * np.sin(a) + d[2] * np.cos(a)])
    return tuple(float(v) for v in r + np.asarray(lookat, np.float64))


def identity_inputs(w, h, spp, colour, shift=(0.0, 0.0)):
    """Guides that the identity view maps to pixel (i + shift_x, j + shift_y)
    exactly: P = (i + shift_x, j + shift_y, 1), n = (0, 0, 1), every sample a
    hit.  colour: (h, w, 3) means; the sums are x spp."""
    yy, xx = np.mgrid[0:h, 0:w].astype(F)
    S = F(spp)
    pos = np.stack([xx + F(shift[0]), yy + F(shift[1]), np.ones_like(xx)], -1).astype(F) * S
    nrm = np.broadcast_to(np.array([0, 0, 1], F) * S, (h, w, 3)).copy()
    return dict(cur=(np.asarray(colour, F) * S).astype(F), hits=np.full((h, w), spp, np.uint32), position=pos,
                normal=nrm)


SYNTH_EYE_Z = 30.0


def synthetic_inputs(w, h, spp=4, seed=0, max_len=32):
    """-> (frame, history, view): a seeded frame, a history and a previous
    view that together reach everything the pass branches on.  Two planes
    with a depth step of 1 between them (left: z = -0.02 X, right: z = -1 -
    0.03 Y, with X = 0.37 col, Y = 0.21 row), seen from (0, 0, 30) through a
    view that maps a point of pixel (col, row) to about 1.06 (col, row) / w -
    0.7: fractional everywhere, off the frame by a part of a pixel on every
    border and by more than a pixel at the far ones.  The current frame has
    scattered sky pixels and a sky block, partially covered pixels, pixels
    whose normals cancel, and a few positions behind the previous eye (w <=
    0).  The history holds the same geometry with its own sky pixels,
    positions off the plane by 1e-4 (kept by every tolerance), by 0.005 (kept
    by the default 0.0003 x 30, rejected by 1e-4 x 30), by 0.02 (kept by a
    loose 0.01 x 30 only) or by 1 (rejected by all), some
    perpendicular normals, and lengths 1 .. max_len with many at max_len."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]

    def geometry(cols, rows):
        X, Y = 0.37 * cols, 0.21 * rows
        left = cols < (w + 1) // 2
        z = np.where(left, -0.02 * X, -1.0 - 0.03 * Y)
        nrm = np.where(left[..., None], np.array([0.02, 0.0, 1.0]), np.array([0.0, 0.03, 1.0]))
        nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
        return np.stack([X, Y, z], -1), nrm

    # the current frame
    hits = rng.integers(1, spp + 1, (h, w)).astype(np.uint32)
    hits[rng.random((h, w)) < 0.6] = spp
    sky = (3 * xx + 5 * yy + 1) % 13 == 0
    sky[h // 2:h // 2 + 2, w // 4:w // 2] = True
    hits[sky] = 0
    pos, nrm = geometry(xx, yy)
    pos = pos + rng.normal(0, 1e-4, (h, w, 3))
    behind = (rng.random((h, w)) < 0.03) & ~sky
    pos[behind, 2] = SYNTH_EYE_Z + 10.0
    hf = hits.astype(F)[..., None]
    position, normal = (pos.astype(F) * hf).astype(F), (nrm.astype(F) * hf).astype(F)
    normal[(rng.random((h, w)) < 0.04) & ~sky] = 0
    cur = (rng.gamma(2.0, 0.25, (h, w, 3)).astype(F) * F(spp)).astype(F)
    frame = dict(cur=cur, hits=hits, position=position, normal=normal)
    # the history
    hist = np.zeros((3, h, w, 4), F)
    hp, hn = geometry(xx, yy)
    kind = rng.random((h, w))
    off = np.where(kind < 0.6, 1e-4, np.where(kind < 0.75, 0.005, np.where(kind < 0.88, 0.02, 1.0))) * rng.choice([-1.0, 1.0], (h, w))
    hp[..., 2] += off
    turned = rng.random((h, w)) < 0.1
    hn[turned] = np.array([1.0, 0.0, 0.0])
    hsky = (5 * xx + 3 * yy + 2) % 11 == 0
    hist[0, ..., :3] = rng.gamma(2.0, 0.25, (h, w, 3))
    ln = rng.integers(1, max_len + 1, (h, w)).astype(F)
    ln[rng.random((h, w)) < 0.3] = max_len
    hist[0, ..., 3] = ln
    hist[1, ..., :3], hist[1, ..., 3] = hp, hsky
    hist[2, ..., :3] = hn
    hist[1, hsky, :3] = 0
    hist[2, hsky, :3] = 0
    view = View(eye=(0.0, 0.0, SYNTH_EYE_Z), px=(1.06 / 0.37, 0.0, 0.0), py=(0.0, 1.06 / 0.21, 0.0),
                pw=(0.0, 0.0, -1.0 / SYNTH_EYE_Z), x0=0.7, y0=0.7)
    return frame, hist, view
