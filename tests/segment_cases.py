"""Distance limits for rt_segment (include/rt_segment.h) on trace_cases' ray
lists, and what the pass must give for them (test infrastructure, no GPU).

The rays and the judge are trace_cases': rays_of(name) and the oracle's
rt_trace record per valid ray, want_of(name, interval).  A limit list gives
every ray a t_max, derived from the ray's own oracle distance t_o (world units
on the normalised ray): t_max = fl32(f t_o / |d|), in units of the unnormalised
direction, for f in FACTORS; a ray the oracle misses gets the world length
MISS_LENGTH f.  The "mixed" list cycles f per ray and puts +inf, 1e30, zero of
both signs, -1 and NaN at fixed indices spread over the waves of both blocks.

Expected, from the header's rules and the oracle's record alone:
  - an invalid ray, or a NaN t_max: RT_SEGMENT_INVALID;
  - t_max <= 0, or a limit at or below t_min (t_max <= 0.001): a miss, never
    traced;
  - a ray the oracle misses: a miss at every limit;
  - f >= 1.25 (and +inf, 1e30): the oracle's record;  f <= 0.75: a miss.
The band between 0.75 and 1.25 stands for the difference between the scan's
root, which the limit is compared with, and the refined root t_o; no limit of
the lists lies inside it (asserted).

One kind of ray does not fit the band, and stays in the lists: three
"surface-in" rays (final 29, final17 2, crowd 209; |d| = 1e-3, so t_min = 1e-6)
start on a sphere and go into it.  Their scan root is at or above t_min (it
is a candidate), their refined root is the exact answer, about 0: t_o =
1.3e-9, -7.7e-9 and 1.2e-8, a thousandth of t_min or less and once negative.
A limit of 2 t_o lies far below t_min (or below zero) and the header's rule
for such a limit applies: a miss, never traced.  The lists test exactly that;
the rays are hits at +inf and at 1e30 (DESIGN.md 17 has their roots).
near_zero_hits() names them and test_segment.py holds their number."""
import math

import numpy as np

import trace_cases as tc
import rtow

F32 = np.float32
FACTORS = (0.5, 0.75, 1.25, 2.0)
MISS_LENGTH = 3.0  # world length f MISS_LENGTH for a ray the oracle misses
T_MIN = 1e-3       # the pass's t_min in units of the unnormalised direction
# mixed list: index -> t_max; in waves 0, 1, 2, 3 and, in the second block, 4
SPECIAL = ((5, math.inf), (37, -0.0), (70, 0.0), (101, math.nan), (133, -1.0), (198, 1e30), (260, math.nan),
           (262, math.inf), (263, -math.inf))
NAMES = ("blocked", "id", "t", "position", "normal")

_LIMITS, _WANT = {}, {}


def dir_length(name):
    """|d| per ray in fp64 (1 for an invalid ray)."""
    L = tc.rays_of(name)
    with np.errstate(over="ignore", invalid="ignore"):
        ln = np.sqrt((L["d"].astype(np.float64) ** 2).sum(1))
    return np.where(L["valid"], ln, 1.0)


def _fma(a, b, c):
    """fl32(a b + c) for float32 arrays: the product is exact in fp64, the sum
    is rounded there first (a double rounding, a last-bit matter at most)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def normalised_length(d):
    """normalize3's l2 r in fp32, operation by operation: the length the pass
    multiplies t_max by (d: float32 (n, 3), valid directions)."""
    x, y, z = (np.ascontiguousarray(d[:, k], F32) for k in range(3))
    l2 = _fma(z, z, _fma(y, y, x * x))
    r = (np.uint32(0x5f375a86) - (l2.view(np.uint32) >> np.uint32(1))).astype(np.uint32).view(F32)
    h = F32(0.5) * l2
    for _ in range(3):
        r = r * _fma(-h, r * r, np.full_like(r, 1.5))
    return l2 * r


def limits_of(name, interval=0):
    """{f: t_max float32 (n,) for f in FACTORS, "mixed": ...}, read-only; t_o is
    the oracle's under that interval flag (a root at t_min itself is taken
    under one flag and not the other, and the ray's hit moves)."""
    if (name, interval) not in _LIMITS:
        L, w = tc.rays_of(name), tc.want_of(name, interval)
        n, ln = L["n"], dir_length(name)
        hit = L["valid"] & (w["id"] >= 0)
        world = np.where(hit, w["t"].astype(np.float64), MISS_LENGTH)  # the length f scales
        out = {}
        for f in FACTORS:
            out[f] = np.where(L["valid"], f * world / ln, 1.0).astype(F32)
        cyc = np.array(FACTORS)[np.arange(n) % len(FACTORS)]
        mixed = np.where(L["valid"], cyc * world / ln, 1.0).astype(F32)
        for i, v in SPECIAL:
            assert i < n and L["valid"][i] and i != tc.FAR_AT, (name, i)
            mixed[i] = v
        out["mixed"] = mixed
        for a in out.values():
            a.setflags(write=False)
        _LIMITS[name, interval] = out
    return _LIMITS[name, interval]


def classes_of(name, key, interval=0):
    """Per ray of limits_of(name, interval)[key]: "invalid", "never" (a valid ray that is
    a miss without a walk), "miss" (the oracle's miss), "kept", "cut"."""
    L, w = tc.rays_of(name), tc.want_of(name, interval)
    tm, ln = limits_of(name, interval)[key], dir_length(name)
    out = []
    for i in range(L["n"]):
        t = float(tm[i])
        if not L["valid"][i] or math.isnan(t):
            out.append("invalid")
        elif t <= 0.9 * T_MIN:
            out.append("never")
        elif w["id"][i] < 0:
            out.append("miss")
        elif w["t"][i] < 0.5 * T_MIN * ln[i]:
            # a near-zero hit (the header): its scan root is not known here, so only no limit at all is judged
            assert t * ln[i] >= 1e29, (name, key, i, t)
            out.append("kept")
        else:
            ratio = t * ln[i] / float(w["t"][i])  # the limit against t_o, both in world units
            if ratio <= 0.75 * (1 + 1e-6):
                out.append("cut")
            else:  # outside the band, and the limit clearly above t_min: the oracle's record
                assert t >= 1.1 * T_MIN and ratio >= 1.25 * (1 - 1e-6), (name, key, i, t, ratio)
                out.append("kept")
    return out


def want_of(name, key, interval=0):
    """What rt_segment must give for rays_of(name) with limits_of(name, interval)[key]:
    dict(blocked, id, t, position, normal), computed once."""
    k = (name, key, interval)
    if k not in _WANT:
        w, cls = tc.want_of(name, interval), classes_of(name, key, interval)
        n = len(cls)
        out = dict(blocked=np.zeros(n, np.uint8), id=np.full(n, rtow.SEGMENT_MISS, np.int32),
                   t=np.full(n, np.inf, F32), position=np.zeros((n, 3), F32), normal=np.zeros((n, 3), F32))
        for i, c in enumerate(cls):
            if c == "invalid":
                out["id"][i] = rtow.SEGMENT_INVALID
            elif c == "kept":
                out["blocked"][i] = 1
                for f in ("id", "t", "position", "normal"):
                    out[f][i] = w[f][i]
        for a in out.values():
            a.setflags(write=False)
        _WANT[k] = out
    return _WANT[k]


def unlimited_want(name, interval=0):
    """rt_trace's records with blocked: what t_max = NULL, +inf and 1e30 give."""
    w = tc.want_of(name, interval)
    out = {f: w[f] for f in ("id", "t", "position", "normal")}
    out["blocked"] = (w["id"] >= 0).astype(np.uint8)
    return out


def near_zero_hits(name):
    """The valid rays the oracle hits at a refined root below half of t_min
    (see the header): [(index, tag, t_o, t_min on the normalised ray)]."""
    L, w, ln = tc.rays_of(name), tc.want_of(name), dir_length(name)
    return [(i, L["tags"][i], float(w["t"][i]), T_MIN * ln[i]) for i in range(L["n"])
            if L["valid"][i] and w["id"][i] >= 0 and w["t"][i] < 0.5 * T_MIN * ln[i]]


def boundary_limits(name):
    """For the boundary test: (below, at, above), each float32 (n,).  `at` is
    fl32(t_o / len) for a ray the oracle hits at t_o > 0, len the fp32 length
    of normalised_length(); below and above are its float neighbours.  Every
    other ray has +inf in all three."""
    L, w = tc.rays_of(name), tc.want_of(name)
    sel = L["valid"] & (w["id"] >= 0) & (w["t"] > 0)
    at = np.full(L["n"], np.inf, F32)
    with np.errstate(all="ignore"):
        at[sel] = (w["t"][sel] / normalised_length(L["d"][sel])).astype(F32)
    assert np.isfinite(at[sel]).all() and (at[sel] > 0).all()
    below, above = np.nextafter(at, F32(0)), np.nextafter(at, F32(np.inf))
    below[~sel], above[~sel] = np.inf, np.inf
    return below, at, above
