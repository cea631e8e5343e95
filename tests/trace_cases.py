"""Ray batches for rt_trace (include/rt_trace.h) and their judge (test
infrastructure, no GPU): one seeded list of rays per scene of ray_fans.SCENES,
and for every valid ray the record of the oracle's chain restatement on a
single-ray camera.

The judge.  Ray i of a batch is rt_aov's sample of a lens-less primary ray
with the same origin and unnormalised direction bits.  ray_fans' header shows
how a hand-built camera gives every pixel one ray: horiz = vert = 0, so the
direction is fl32(corner - eye).  A ray here is therefore stored as (o,
corner): d = fl32(corner - o) is what rt_trace gets, and
fan(eye = o, corner, 0, 0) what oracle_lib.kernel_terminals(max_bounces = -1,
keep_dir = True) gets, on the 8 x 8 frame of ray_fans' single-ray cases; a
record's sphere, depth, P and N are the expected id, t, position and normal.
A zero component of d is +0 with corner[k] = o[k], and -0 with o[k] = +0 and
corner[k] = horiz[k] = vert[k] = -0 (ray_fans.single).

test_trace.py holds the lists to their coverage conditions on the CPU;
test_trace_gpu.py compares rt_trace with the records byte for byte.
"""
import math

import numpy as np

import oracle_lib
import ray_fans as rf
import rtow

F32 = np.float32
FRAME = (8, 8)  # ray_fans' single-ray frame
LENGTHS = (1e-3, 1.0, 1e3)  # |d| of the aimed rays, in turn
WAVE = 64
FAR_AT = 17  # the one far origin in the first, otherwise near wave
BLOCK = 256  # rtk::kBlock: every list is longer, so a batch fills more than one block
N_CENTRE, N_SKY = 70, 60
SEEDS = {"final": 1601, "final17": 1602, "five": 1603, "crowd": 1604}


class Rays:
    """A list under construction: origins, corners (d = fl32(corner - o)), the
    axes whose zero component is -0, a tag per ray; invalid rays carry their
    direction themselves."""

    def __init__(self):
        self.o, self.corner, self.neg, self.tag, self.raw_d = [], [], [], [], []

    def add(self, tag, o, step, neg=()):
        """The ray from fl32(o) along about `step`; a zero of step is an exact
        zero component (-0 on the axes in neg, which need o = +0 there)."""
        o = [float(F32(x)) for x in o]
        corner = [float(F32(F32(e) + F32(s))) if s != 0.0 else e for e, s in zip(o, step)]
        for k in neg:
            assert step[k] == 0.0 and o[k] == 0.0 and math.copysign(1.0, o[k]) > 0
            corner[k] = -0.0
        for k in range(3):  # (an eye of -0 would turn a +0 component's sign: not used)
            assert not (o[k] == 0.0 and math.copysign(1.0, o[k]) < 0)
        self.o.append(o), self.corner.append(corner), self.neg.append(tuple(neg)), self.tag.append(tag)
        self.raw_d.append(None)

    def add_exact(self, tag, o, corner):
        """The ray from o with d = fl32(corner - o), both given as float32 values."""
        self.o.append([float(x) for x in o]), self.corner.append([float(x) for x in corner])
        self.neg.append(()), self.tag.append(tag), self.raw_d.append(None)

    def add_invalid(self, tag, o, d):
        self.o.append([float(x) for x in o]), self.corner.append(None), self.neg.append(()), self.tag.append(tag)
        self.raw_d.append([float(x) for x in d])

    def __len__(self):
        return len(self.o)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _perp(v, rng):
    """A unit vector across v."""
    w = np.cross(v, rng.normal(size=3))
    return w / np.linalg.norm(w)


def _around(rng, ext, lo=0.3, hi=4.0):
    a = rng.uniform(0.0, 2.0 * math.pi)
    R = rng.uniform(ext + 1.0, ext + 4.0)
    return np.array((R * math.cos(a), rng.uniform(lo, hi), R * math.sin(a)))


def _near_rays(name, rng):
    """Everything but the far origins and the invalid forms."""
    sc = rf.scene_of(name)
    C = np.stack([sc.cx, sc.cy, sc.cz], 1).astype(np.float64)
    r = sc.radius.astype(np.float64)
    small = np.nonzero(np.abs(r) < 10.0)[0]
    big = np.nonzero(np.abs(r) >= 10.0)[0]  # the ground
    ext = float(np.abs(C[small][:, [0, 2]]).max())
    rays = Rays()
    k = 0

    def length():
        nonlocal k
        k += 1
        return LENGTHS[k % 3]

    # aimed at sphere centres from around the scene
    picks = list(rng.choice(small, min(N_CENTRE - 4, len(small)), replace=False)) + list(big)
    while len(picks) < N_CENTRE:
        picks += list(small)
    for i in picks[:N_CENTRE]:
        o = _around(rng, ext)
        rays.add("centre", o, length() * _unit(C[i] - o))
    # grazing: aimed at C + r (1 +- 1e-3) u, u across the line of sight
    for i in list(rng.choice(small, min(14, len(small)), replace=len(small) < 14)):
        o = _around(rng, ext)
        u = _perp(C[i] - o, rng)
        for s in (1.0 + 1e-3, 1.0 - 1e-3):
            rays.add("graze", o, length() * _unit(C[i] + abs(r[i]) * s * u - o))
    # into the sky
    for _ in range(N_SKY):
        o = _around(rng, ext, 0.2, 6.0)
        d = rng.normal(size=3)
        d[1] = abs(d[1]) + 0.3
        rays.add("sky", o + (0.0, 6.0, 0.0), length() * _unit(d))
    # origins inside glass spheres (positive radius)
    glass = [i for i in small if sc.kind[i] == rtow.RT_DIELECTRIC and r[i] > 0]
    for j in range(14 if glass else 0):
        i = glass[j % len(glass)]
        rays.add("inside-glass", C[i] + 0.5 * r[i] * _unit(rng.normal(size=3)), length() * _unit(rng.normal(size=3)))
    # origins inside a negative-radius shell: between the shell and its outer sphere, and within it
    for i in [i for i in small if r[i] < 0]:
        outer = [j for j in small if r[j] > 0 and np.allclose(C[j], C[i])]
        for _ in range(6):
            u = _unit(rng.normal(size=3))
            if outer:
                o = C[i] + 0.5 * (abs(r[i]) + r[outer[0]]) * u
                rays.add("in-shell", o, length() * _unit(C[i] - o + 0.2 * abs(r[i]) * _perp(u, rng)))
            rays.add("in-hollow", C[i] + 0.4 * abs(r[i]) * u, length() * _unit(rng.normal(size=3)))
    # origins on a sphere's surface, going out and going in
    for i in list(rng.choice(small, min(8, len(small)), replace=len(small) < 8)):
        u = _unit(rng.normal(size=3))
        u[1] = abs(u[1])
        p = C[i] + abs(r[i]) * u
        for sgn in (1.0, -1.0):
            rays.add("surface-out" if sgn > 0 else "surface-in", p, length() * _unit(sgn * u + 0.3 * _perp(u, rng)))
    # ... and on the ground far from its centre's axis
    for g in big:
        for dist in (3.0, 20.0, 0.09 * r[g], 0.3 * r[g]):
            a = rng.uniform(0.0, 2.0 * math.pi)
            x, z = C[g][0] + dist * math.cos(a), C[g][2] + dist * math.sin(a)
            p = np.array((x, C[g][1] + math.sqrt(r[g] ** 2 - dist ** 2), z))
            u = _unit(p - C[g])
            for sgn in (1.0, -1.0):
                rays.add("ground-out" if sgn > 0 else "ground-in", p, length() * _unit(sgn * u + 0.5 * _perp(u, rng)))
    # exactly axis-parallel, both signs of zero
    top = float((C[small][:, 1] + np.abs(r[small])).max()) + 1.0
    spots = [int(i) for i in rng.choice(small, 4, replace=len(small) < 4)]
    for i in spots:
        rays.add("axis-down", (C[i][0], top, C[i][2]), (0.0, -length(), 0.0))
        rays.add("axis+x", (-(ext + 2.0), C[i][1], C[i][2]), (length(), 0.0, 0.0))
        rays.add("axis-z", (C[i][0], C[i][1], ext + 2.0), (0.0, 0.0, -length()))
    rays.add("axis-down -0", (0.0, top, 0.0), (0.0, -1.0, 0.0), neg=(0, 2))
    rays.add("axis-down -0x", (0.0, top, C[spots[0]][2]), (0.0, -1e3, 0.0), neg=(0,))
    rays.add("axis+x -0z", (-(ext + 2.0), 0.05, 0.0), (1e-3, 0.0, 0.0), neg=(2,))
    rays.add("axis-z -0x", (0.0, 0.05, ext + 2.0), (0.0, 0.0, -1.0), neg=(0,))
    rays.add("axis-up -0", (0.0, top, 0.0), (0.0, 1.0, 0.0), neg=(0, 2))
    rays.add("axis-up", (0.3, top, 0.4), (0.0, 1e3, 0.0))
    return rays, ext


def _far_ray(rays, name, rng, ext, tag):
    oref = rf.oref_of(name)
    o = rng.uniform(1.2, 5.0) * oref * _unit(rng.normal(size=3) + (0.0, 1.5, 0.0))
    target = np.array((rng.uniform(-ext, ext), rng.uniform(-0.5, 3.0), rng.uniform(-ext, ext)))
    rays.add(tag, o, _unit(target - o))


INVALID = (("zero", (1.0, 2.0, 3.0), (0.0, 0.0, 0.0)),
           ("zero -0", (1.0, 2.0, 3.0), (-0.0, 0.0, -0.0)),
           ("nan origin", (math.nan, 2.0, 3.0), (0.0, -1.0, 0.0)),
           ("nan direction", (1.0, 2.0, 3.0), (0.0, math.nan, 0.0)),
           ("inf origin", (1.0, -math.inf, 3.0), (0.0, -1.0, 0.0)),
           ("inf direction", (1.0, 2.0, 3.0), (math.inf, -1.0, 0.0)),
           ("l2 overflows", (1.0, 4.0, 3.0), (3e19, -3e19, 1e19)))
INVALID_AT = (140, 141, 150, 163, 191, 192, 200)  # in the third and fourth wave, two pairs adjacent


def _build(name):
    rng = np.random.default_rng(SEEDS[name])
    near, ext = _near_rays(name, rng)
    order = rng.permutation(len(near))
    for o, corner in FROZEN.get(name, ()):
        near.add_exact("frozen-skip", [float.fromhex(x) for x in o], [float.fromhex(x) for x in corner])
        order = np.append(order, len(near) - 1)
    out = Rays()

    def take(j):
        out.o.append(near.o[j]), out.corner.append(near.corner[j]), out.neg.append(near.neg[j])
        out.tag.append(near.tag[j]), out.raw_d.append(None)

    # wave 0: origins within oref, one far origin at FAR_AT; wave 1: every origin beyond oref; then
    # the rest (the distant ground points among them), the invalid forms at INVALID_AT
    oref2 = float(rf.oref2_of(name))
    within = [j for j in order if sum(float(F32(x)) ** 2 for x in near.o[j]) < 0.9 * oref2]
    first = set(within[:WAVE - 1])
    it = iter(within[:WAVE - 1] + [j for j in order if j not in first])
    for i in range(WAVE):
        if i == FAR_AT:
            _far_ray(out, name, rng, ext, "far-one")
        else:
            take(next(it))
    for i in range(WAVE):
        _far_ray(out, name, rng, ext, "far-wave")
    inv = dict(zip(INVALID_AT, INVALID))
    for j in it:
        while len(out) in inv:
            out.add_invalid("invalid " + inv[len(out)][0], *inv[len(out)][1:])
        take(j)
    assert len(out) > BLOCK + 1 and len(out) % WAVE != 0, len(out)
    return out


# Rays that take the camera ray's spurious-root skip (RTO_EV_SKIP_TMIN), found
# by search_skips("final" / "five", 40, 7) below and frozen here as (origin,
# corner) in float32 hex: origins about t_min under a sphere's surface, going
# out.  The first of each scene then leaves the scene, the others hit another
# sphere (t = the distance walked + the second walk's root).  test_trace.py
# asserts that each still takes the skip.
FROZEN = {
    "final": ((("0x1.2f228ep+3", "0x1.01dc28p-2", "0x1.33bf8cp+3"), ("0x1.2ff222p+3", "0x1.46e3bp-1", "0x1.161fc6p+3")),
              (("0x1.23d1f4p+2", "0x1.73011ap-2", "0x1.bdb3dep-1"), ("0x1.fdf5cap+1", "0x1.2b11e6p+0", "0x1.768c56p-1")),
              (("0x1.23b114p+2", "0x1.71226ep-2", "0x1.bc02fep-1"), ("0x1.fdf5cap+1", "0x1.2b11e6p+0", "0x1.768c56p-1"))),
    "five": ((("0x1.287f68p+0", "0x1.f2b458p-4", "-0x1.75173p+0"), ("0x1.306398p+0", "0x1.0b8526p-1", "-0x1.30401ap+1")),
             (("-0x1.3ad33cp+0", "0x1.4b9ff2p-2", "-0x1.09faf4p+0"), ("-0x1.cdaf52p+0", "0x1.21956ep+0", "-0x1.2d7e22p+0")),
             (("-0x1.399f18p+0", "0x1.4edf8ap-2", "-0x1.0a387ap+0"), ("-0x1.cdaf52p+0", "0x1.21956ep+0", "-0x1.2d7e22p+0"))),
}
N_FROZEN = sum(len(v) for v in FROZEN.values())

_LISTS, _WANT = {}, {}


def rays_of(name):
    """The scene's batch: dict(o, d: float32 (n, 3); valid: bool (n,); tags;
    cams: the single-ray camera per valid ray, None for an invalid one)."""
    if name not in _LISTS:
        r = _build(name)
        n = len(r)
        o, d, valid, cams = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, bool), []
        for i in range(n):
            o[i] = r.o[i]
            if r.corner[i] is None:
                d[i] = r.raw_d[i]
                cams.append(None)
                continue
            h = [-0.0 if k in r.neg[i] else 0.0 for k in range(3)]
            cam = rf.fan(r.o[i], r.corner[i], h, h)
            d[i] = rf.direction_of(cam)
            for k in r.neg[i]:
                assert d[i][k] == 0 and np.signbit(d[i][k])
            valid[i] = True
            cams.append(cam)
        for a in (o, d, valid):
            a.setflags(write=False)
        _LISTS[name] = dict(o=o, d=d, valid=valid, tags=tuple(r.tag), cams=cams, n=n)
    return _LISTS[name]


def judge(scene, cam, interval=0):
    """The oracle's record for a single-ray camera: a 0-d TERMINAL."""
    p = rtow.make_params(FRAME[0], FRAME[1], 1, seed=1, flags=interval)
    return oracle_lib.kernel_terminals(scene, cam, p, -1, 0.0, keep_dir=True)[0, 0, 0]


def want_of(name, interval=0):
    """What rt_trace must give for rays_of(name) with that interval flag:
    dict(id, t, position, normal, events), computed once; an invalid ray has
    TRACE_INVALID, +inf and zeros."""
    key = (name, interval)
    if key not in _WANT:
        L, sc = rays_of(name), rf.scene_of(name)
        n = L["n"]
        w = dict(id=np.full(n, rtow.TRACE_INVALID, np.int32), t=np.full(n, np.inf, F32),
                 position=np.zeros((n, 3), F32), normal=np.zeros((n, 3), F32), events=np.zeros(n, np.uint32))
        for i in range(n):
            if not L["valid"][i]:
                continue
            rec = judge(sc, L["cams"][i], interval)
            w["id"][i] = rec["sphere"]
            w["events"][i] = rec["events"]
            if rec["sphere"] >= 0:
                w["t"][i], w["position"][i], w["normal"][i] = rec["depth"], rec["P"], rec["N"]
        for a in w.values():
            a.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


# The eight rays of the final scene's list that test_trace_gpu.py also sends
# through rt_aov: the first ray with the tag whose oracle record is of the kind.
AOV_CHECK = (("centre", "hit"), ("graze", "hit"), ("inside-glass", "hit"), ("ground-in", "hit"),
             ("axis-down", "hit"), ("axis+x -0z", "hit"), ("frozen-skip", "hit"), ("sky", "miss"),
             ("far-one", "hit"), ("frozen-skip", "miss"))


def aov_check_rays(name="final"):
    """[(index, tag, kind)] for AOV_CHECK on the oracle's records."""
    tags, ids = rays_of(name)["tags"], want_of(name)["id"]
    out = []
    for tag, kind in AOV_CHECK:
        idx = [i for i, t in enumerate(tags) if t == tag and (ids[i] >= 0) == (kind == "hit")]
        assert idx, (tag, kind)
        out.append((idx[0], tag, kind))
    return out


# ------------------------------------------------------- spurious-root search
def search_skips(name, calls, seed, depth=1e-3, spread=1.0, frame=(32, 16), spp=64):
    """Rays whose first walk ends in the spurious-root skip, searched with lens
    cameras: a lens spreads a frame's origins over a patch just under a
    sphere's surface, every ray aimed at one far corner, so that the exit root
    lies about t_min away.  Each call judges frame x spp candidates at once;
    oracle_lib.camera_origins gives the origin of a sample that took the skip,
    and fl32(corner - origin) its direction.  -> (candidates, [(o, d)])."""
    sc = rf.scene_of(name)
    rng = np.random.default_rng(seed)
    C = np.stack([sc.cx, sc.cy, sc.cz], 1).astype(np.float64)
    r = sc.radius.astype(np.float64)
    p = rtow.make_params(frame[0], frame[1], spp, seed=seed)
    found, tried = [], 0
    for _ in range(calls):
        i = int(rng.integers(0, sc.n))
        u = _unit(rng.normal(size=3))
        u[1] = abs(u[1])
        u = _unit(u)
        a = _perp(u, rng)
        b = np.cross(u, a)
        eye = C[i] + (abs(r[i]) - depth * rng.uniform(0.5, 1.5)) * u
        corner = eye + rng.choice(LENGTHS) * _unit(u + 0.5 * rng.uniform(-1, 1) * a)
        cam = rf.fan(eye, corner, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), lens_u=tuple(spread * math.sqrt(abs(r[i])) * 0.03 * a),
                     lens_v=tuple(spread * math.sqrt(abs(r[i])) * 0.03 * b))
        t = oracle_lib.kernel_terminals(sc, cam, p, -1, 0.0, keep_dir=True)
        tried += t.size
        hit = np.argwhere(t["events"] & oracle_lib.EVENTS["skip_tmin"])
        if len(hit):
            org = oracle_lib.camera_origins(cam, p)
            for row, col, s in hit[:4]:
                o = org[row, col, s]
                found.append((o.copy(), np.array(cam.corner[:], F32) - o, np.array(cam.corner[:], F32)))
    return tried, found
