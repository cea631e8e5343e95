"""Hand-built cameras that aim rays at the walks' edges (test infrastructure,
no GPU): exactly axis-parallel rays, rays in cell border planes and through
cell corners, eyes in the grid's empty ring and outside its box, and ray
origins beyond the bound the boxes' padding is valid for (oref).

rt_camera is a plain record: with has_lens = 0 every primary ray is
normalize(corner + fs horiz + ft vert - eye) from eye.  So
  horiz[k] = vert[k] = 0, corner[k] = eye[k]           gives d[k] = +0 exactly,
  corner[k] = horiz[k] = vert[k] = -0.0, eye[k] = +0.0  gives d[k] = -0
(x - x is +0 for every other x, so -0 needs an eye coordinate of +0), and
horiz = vert = 0 gives every pixel one ray (a single-ray camera: only the
bounces differ).  CASES is the one list test_ray_fans.py (the coverage
conditions, on the CPU oracle) and test_ray_fans_gpu.py (every walk of every
tracing code object against the oracle, bit for bit) share.

Also the two scene constructions several test files share: crowd() and
with_extra_spheres().
"""
import ctypes
import dataclasses
import math

import numpy as np

import oracle_lib
import rtow

CPU, GPU = rtow.RT_CAMERA_CPU, rtow.RT_CAMERA_GPU
NZ = -0.0
DEPTH = 50


# ------------------------------------------------------------------ scenes --

def crowd(rtow, cx, cz, radius, seed):
    """The ground and len(cx) small spheres of one radius resting on it (a
    layer scene: the construction of test_dense_layer_grid_build_paths)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    n_small = len(cx)
    kind = np.array([0] + [int(k) for k in rng.integers(0, 3, n_small)], np.uint32)
    return dataclasses.replace(
        rtow.final_scene(),
        cx=np.array([0.0] + list(cx), f32),
        cy=np.array([-1000.0] + [radius] * n_small, f32),
        cz=np.array([0.0] + list(cz), f32),
        radius=np.array([1000.0] + [radius] * n_small, f32),
        kind=kind,
        albedo=rng.uniform(0.2, 0.9, (n_small + 1, 3)).astype(f32),
        param=np.where(kind == 2, 1.5, 0.3).astype(f32))


def with_extra_spheres(rtow, scene, spheres):
    """scene + spheres [(x, y, z, r, kind, (r, g, b), param), ...] appended."""
    ex = list(zip(*spheres))
    f32 = np.float32
    return dataclasses.replace(
        scene,
        cx=np.concatenate([scene.cx, np.array(ex[0], f32)]),
        cy=np.concatenate([scene.cy, np.array(ex[1], f32)]),
        cz=np.concatenate([scene.cz, np.array(ex[2], f32)]),
        radius=np.concatenate([scene.radius, np.array(ex[3], f32)]),
        kind=np.concatenate([scene.kind, np.array(ex[4], np.uint32)]),
        albedo=np.concatenate([scene.albedo, np.array(ex[5], f32).reshape(-1, 3)]),
        param=np.concatenate([scene.param, np.array(ex[6], f32)]))


def _final17():
    """The final scene and 13 big spheres above it: 17 spheres off the layer,
    one more than layer mode takes, so RT_FLAG_ACCEL_BVH walks the plain BVH."""
    rng = np.random.default_rng(13)
    extra = [(float(rng.uniform(-9, 9)), 1.0 + float(rng.uniform(0, 1)), float(rng.uniform(-9, 9)),
              0.6 + 0.3 * float(rng.uniform()), i % 3, (0.7, 0.5, 0.3), 1.5 if i % 3 == 2 else 0.2) for i in range(13)]
    return with_extra_spheres(rtow, rtow.final_scene(), extra)


LATTICE = 0.75  # the crowd scene's lattice pitch


def _lattice_crowd():
    """A crowd on a jittered 9 x 9 lattice (pitch LATTICE, r = 0.1, jitter well
    inside r: a plane through a lattice line cuts all nine spheres of it) and
    seven more spheres heaped near one lattice point, which fill that cell past
    the item chain's four stages into the pointer loop."""
    rng = np.random.default_rng(90)
    ij = np.array([(i, j) for i in range(-4, 5) for j in range(-4, 5)], np.float64)
    cx = LATTICE * ij[:, 0] + rng.uniform(-0.04, 0.04, len(ij))
    cz = LATTICE * ij[:, 1] + rng.uniform(-0.04, 0.04, len(ij))
    heap = rng.uniform(-0.12, 0.12, (7, 2)) + (LATTICE * 1.5, -LATTICE * 0.5)
    return crowd(rtow, np.concatenate([cx, heap[:, 0]]), np.concatenate([cz, heap[:, 1]]), 0.1, 91)


SCENES = {"final": rtow.final_scene, "final17": _final17, "five": rtow.five_scene, "crowd": _lattice_crowd}
LAYER_SCENES = ("final", "crowd")  # layer mode with a grid: scan, layer BVH, grid in three placements
_SCENES, _INFO = {}, {}


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = SCENES[name]()
    return _SCENES[name]


def info_of(name):
    """rtow.accel_info of a scene (default grid options; every placement shares the geometry)."""
    if name not in _INFO:
        _INFO[name] = rtow.accel_info(scene_of(name))
    return _INFO[name]


def layer_spheres(scene):
    """Indices of the layer's spheres: those of the commonest (centre y, radius)."""
    key = np.stack([scene.cy, scene.radius], 1)
    vals, counts = np.unique(key, axis=0, return_counts=True)
    top = vals[np.argmax(counts)]
    return np.nonzero((key == top).all(1))[0]


def border(info, axis, k):
    """The walk's border between stored columns (rows) k - 1 and k,
    fmaf((float)k, grid_g, grid_x0) (grid_z0) in float32: the product is exact
    in float64 and so is the sum, so one rounding gives the fma's bits."""
    o = info["grid_x0" if axis == 0 else "grid_z0"]
    return np.float32(float(k) * float(info["grid_g"]) + float(o))


def oref_of(name):
    return info_of(name)["oref_milli"] / 1000.0


def oref2_of(name):
    """The float32 the host uploads: (float)(0.99 oref^2)."""
    return np.float32(0.99 * oref_of(name) * oref_of(name))


# ----------------------------------------------------------------- cameras --

def fan(eye, corner, horiz, vert, model=CPU, lens_u=None, lens_v=None):
    """An rtow.Camera field by field (float32 of each number, signs of zero kept)."""
    cam = rtow.Camera()
    cam.model = model
    cam.has_lens = 0 if lens_u is None and lens_v is None else 1
    for name, v in (("eye", eye), ("corner", corner), ("horiz", horiz), ("vert", vert),
                    ("lens_u", lens_u or (0.0, 0.0, 0.0)), ("lens_v", lens_v or (0.0, 0.0, 0.0))):
        setattr(cam, name, (ctypes.c_float * 3)(*[float(x) for x in v]))
    return cam


def sheet(eye, a, b, c, zero=(), neg=False, model=CPU, frame=(32, 16)):
    """A fan over the parallelogram a + fs (b - a) + ft (c - a), fs, ft in
    [0, 1]: the CPU model's pixels span it; the GPU model's fs, ft count
    pixels, so its steps are divided by the frame.  zero: the axes on which
    a, b, c and eye agree, forced to an exact zero component (neg: of -0,
    which needs eye = +0 there)."""
    eye, a, b, c = (np.array(v, np.float64) for v in (eye, a, b, c))
    h, v = b - a, c - a
    if model == GPU:
        h, v = h / frame[0], v / frame[1]
    corner = a.copy()
    for k in zero:
        assert a[k] == b[k] == c[k] == eye[k] and (not neg or eye[k] == 0.0), (k, eye, a, b, c)
        corner[k], h[k], v[k] = (NZ, NZ, NZ) if neg else (eye[k], 0.0, 0.0)
    return fan(eye, corner, h, v, model)


def single(eye, step, neg=()):
    """A single-ray camera: horiz = vert = 0, every pixel's ray is
    normalize(step) from eye; a zero of step is an exact zero component, of
    -0 on the axes in neg (eye = +0 there)."""
    eye = [float(np.float32(x)) for x in eye]
    corner = [float(np.float32(e) + np.float32(s)) if s != 0.0 else e for e, s in zip(eye, step)]
    h = [0.0, 0.0, 0.0]
    for k in neg:
        assert step[k] == 0.0 and eye[k] == 0.0 and not math.copysign(1.0, eye[k]) < 0
        corner[k], h[k] = NZ, NZ
    return fan(eye, corner, h, h)


def direction_of(cam):
    """float32 corner - eye: the host's view of a single-ray camera's direction
    before normalisation, and on a zero axis of any fan the sign of its zero."""
    return np.array(cam.corner[:], np.float32) - np.array(cam.eye[:], np.float32)


def _busiest(scene, axis, lo=-8.0, hi=8.0, reach=0.12):
    """The coordinate on `axis` (0: x, 2: z) in [lo, hi] whose plane cuts the
    most layer spheres within `reach` of their centres, and a layer sphere's
    own centre coordinate nearest to it."""
    c = (scene.cx if axis == 0 else scene.cz)[layer_spheres(scene)].astype(np.float64)
    grid = np.arange(lo, hi, 0.01)
    n = (np.abs(c[None, :] - grid[:, None]) < reach).sum(1)
    best = float(grid[np.argmax(n)])
    return best, float(c[np.argmin(np.abs(c - best))])


def _plane_fan(axis, at, y_eye, far, span, zero, neg=False, flip=False, model=CPU, y=(0.0, 0.4)):
    """A fan in the plane coordinate[axis] = at (an exact zero component on that
    axis): the eye at height y_eye and distance far along the other
    horizontal axis, looking back over [-span, span] of it at heights y."""
    other = 2 if axis == 0 else 0
    s = -1.0 if flip else 1.0

    def pt(u, h):
        p = [0.0, h, 0.0]
        p[axis], p[other] = at, u
        return p
    eye = pt(s * far, y_eye)
    return sheet(eye, pt(-s * span, y[0]), pt(s * span, y[0]), pt(-s * span, y[1]), zero, neg, model)


def _slab_fan(y, eye_xz, half, neg=False, model=CPU):
    """A dy = 0 fan at height y (eye and targets share it): from eye_xz over
    the square [-half, half]^2's far edges."""
    ex, ez = eye_xz
    eye = (ex, y, ez)
    return sheet(eye, (-half, y, -half), (half, y, -half * 0.2), (-half * 0.2, y, half), (1,), neg, model)


# ------------------------------------------------------------------- cases --
# name: dict(scene, cams [(label, Camera)], frame, spp, seed, and what it is for:
#   zero:   axes whose direction component is exactly 0 on every primary ray
#   neg:    True: ... as -0 (the host's corner - eye has its sign bit set there); "some": on some axis of
#           some of the cameras (single rays: those whose label says -0)
#   layer:  the fan is meant to walk the layer (>= 10 % first hits on >= 8 layer spheres, per camera)
#   border: (axis, [k per camera]): the eye's coordinate is border(info, axis, k)
#   may_miss: a camera of the case may hit nothing (above a layer with nothing over it: the walk is skipped)
#   far:    "whole" (every origin beyond oref2) or "mixed" (both sides in every 8x8 tile)
#   model:  the cameras' model (GPU: rendered with RT_FLAG_GPU_SEMANTICS)
# Frames: 32x16 for fans, 8x8 for single-ray cameras.

def _zero_fans(scene_name, model=CPU):
    """The one-zero-component fans of a layer scene, {case: dict}."""
    sc = scene_of(scene_name)
    lay = layer_spheres(sc)
    ext = float(max(np.abs(sc.cx[lay]).max(), np.abs(sc.cz[lay]).max()))
    r = float(sc.radius[lay[0]])
    far, span = ext + 2.0, ext + 0.5
    tag = "-gpu" if model == GPU else ""
    out = {}
    for axis, nm in ((0, "dx0"), (2, "dz0")):
        any_at, centre_at = _busiest(sc, axis, -0.7 * ext, 0.7 * ext, 0.6 * r)
        # (at 0 the final scene's big sphere at the world origin fills part of the view)
        mk = lambda at, neg=False, flip=False, ye=6.0 * r: _plane_fan(axis, at, ye, far, span, (axis,), neg, flip, model,
                                                                     (0.0, 2.0 * r))
        out[f"{scene_name}-{nm}-at0{tag}"] = dict(cams=[("+0", mk(0.0)), ("+0 back", mk(0.0, flip=True))], zero=(axis,))
        out[f"{scene_name}-{nm}-at0-neg{tag}"] = dict(cams=[("-0", mk(0.0, True)), ("-0 back", mk(0.0, True, True))],
                                                     zero=(axis,), neg=True)
        out[f"{scene_name}-{nm}-any{tag}"] = dict(cams=[("fwd", mk(any_at)), ("back", mk(any_at, flip=True)),
                                                       ("high", mk(any_at, ye=20.0 * r))], zero=(axis,), layer=True)
        out[f"{scene_name}-{nm}-centre{tag}"] = dict(cams=[("fwd", mk(centre_at)), ("back", mk(centre_at, flip=True))],
                                                    zero=(axis,), layer=True)
    half = 0.8 * ext
    eyes = ((far, 0.3 * ext), (-0.2 * ext, -far), (0.35 * ext, 0.15 * ext))
    out[f"{scene_name}-dy0-inside{tag}"] = dict(cams=[(str(i), _slab_fan(1.2 * r, e, half, model=model))
                                                     for i, e in enumerate(eyes)], zero=(1,), layer=True)
    out[f"{scene_name}-dy0-bottom{tag}"] = dict(cams=[("+0", _slab_fan(0.0, eyes[0], half, model=model)),
                                                     ("+0 b", _slab_fan(0.0, eyes[2], half, model=model))], zero=(1,))
    out[f"{scene_name}-dy0-bottom-neg{tag}"] = dict(cams=[("-0", _slab_fan(0.0, eyes[0], half, True, model)),
                                                         ("-0 b", _slab_fan(0.0, eyes[2], half, True, model))],
                                                   zero=(1,), neg=True)
    out[f"{scene_name}-dy0-above{tag}"] = dict(cams=[("above", _slab_fan(3.0 * r, eyes[0], half, model=model)),
                                                    ("high", _slab_fan(1.5, eyes[1], half, model=model))], zero=(1,),
                                              may_miss=True)
    for c in out.values():
        c.update(scene=scene_name, frame=(32, 16), spp=3, model=model)
    return out


def _two_zero(scene_name):
    """Single-ray cameras with two exact zero components, {case: dict}."""
    sc = scene_of(scene_name)
    lay = layer_spheres(sc)
    r, cy = float(sc.radius[lay[0]]), float(sc.cy[lay[0]])
    ext = float(max(np.abs(sc.cx[lay]).max(), np.abs(sc.cz[lay]).max())) + 1.0
    near = lay[np.argsort(np.hypot(sc.cx[lay] - 2.0, sc.cz[lay] + 1.5))[:3]]  # three layer spheres
    spots = [(float(sc.cx[i]), float(sc.cz[i])) for i in near] + [(2.13, -1.37)]
    down = [(f"down {x:.2f} {z:.2f}", single((x, 3.0, z), (0.0, -1.0, 0.0))) for x, z in spots]
    down += [("down 0 0 -0", single((0.0, 3.0, 0.0), (0.0, -1.0, 0.0), neg=(0, 2))),
             ("down 0 z -0x", single((0.0, 3.0, spots[0][1]), (0.0, -1.0, 0.0), neg=(0,)))]
    up = [(f"up {x:.2f} {z:.2f}", single((x, -0.5, z), (0.0, 1.0, 0.0))) for x, z in spots]
    up += [("up 0 0 -0", single((0.0, -0.5, 0.0), (0.0, 1.0, 0.0), neg=(0, 2)))]
    out = {f"{scene_name}-down": dict(cams=down, zero=(0, 2), neg="some"),
           f"{scene_name}-up": dict(cams=up, zero=(0, 2), neg="some")}
    for nm, axis, sgn in (("+x", 0, 1.0), ("-x", 0, -1.0), ("+z", 2, 1.0), ("-z", 2, -1.0)):
        other = 2 if axis == 0 else 0
        cams = []
        for i in near:
            for h in (cy, 0.3 * r):  # through the centres' height and near the ground
                eye, step = [0.0, h, 0.0], [0.0, 0.0, 0.0]
                eye[axis], eye[other] = -sgn * ext, float((sc.cz if axis == 0 else sc.cx)[i])
                step[axis] = sgn
                cams.append((f"{nm} {eye[other]:.2f} {h:.2f}", single(eye, step)))
        eye, step = [0.0, cy, 0.0], [0.0, 0.0, 0.0]
        eye[axis], step[axis] = -sgn * ext, sgn
        cams.append((f"{nm} -0", single(eye, step, neg=(other,))))  # in the plane through the world origin
        out[f"{scene_name}-along{nm}"] = dict(cams=cams, zero=tuple(sorted((1, other))), neg="some")
    for c in out.values():
        c.update(scene=scene_name, frame=(8, 8), spp=2, model=CPU)
    return out


def _grid_fans(scene_name):
    """Fans placed relative to the scene's layer grid, {case: dict}."""
    sc, info = scene_of(scene_name), info_of(scene_name)
    lay = layer_spheres(sc)
    r = float(sc.radius[lay[0]])
    nx, nz = info["grid_nx"], info["grid_nz"]
    g = float(info["grid_g"])
    xi, zi, x1, z1 = (float(info[k]) for k in ("grid_xi", "grid_zi", "grid_x1", "grid_z1"))
    ext = max(abs(xi), abs(zi), abs(x1), abs(z1))
    far, span = ext + 1.0, ext
    out = {}
    for axis, nm, n in ((0, "x", nx), (2, "z", nz)):
        ks = [2, n // 2, n - 2]  # interior borders of the stored cells (the listed ones are 1 .. n - 2)
        cams = []
        for k in ks:
            at = float(border(info, axis, k))
            for flip in (False, True):  # both signs of the other horizontal component
                cams.append((f"k={k} {'back' if flip else 'fwd'}",
                             _plane_fan(axis, at, 6.0 * r, far, span, (axis,), flip=flip, y=(0.0, 2.0 * r))))
        out[f"{scene_name}-border-{nm}"] = dict(cams=cams, zero=(axis,), border=(axis, [k for k in ks for _ in (0, 1)]),
                                               frame=(32, 16), spp=2)
    # an eye at a cell corner, a single 45-degree ray (dx == +-dz exactly) through cell corners
    kx, kz = nx // 2, nz // 2
    cx, cz = float(border(info, 0, kx)), float(border(info, 2, kz))
    cams = []
    for sx in (1.0, -1.0):
        for sz in (1.0, -1.0):
            for h, dy in ((0.5 * r, 0.0), (1.5 * r, -0.05)):
                cams.append((f"{sx:+.0f}{sz:+.0f} {dy}", single((cx, h, cz), (4.0 * sx, dy, 4.0 * sz))))
    out[f"{scene_name}-diagonal"] = dict(cams=cams, diagonal=True, frame=(8, 8), spp=2)
    # an eye in the ring, just outside the inner box, looking in; and one exactly on grid_xi with dx = 0
    y = (0.0, 2.0 * r)
    ring = [("ring -x", sheet((xi - 0.5 * g, 1.2 * r, 0.3), (xi + 6.0, y[0], -span), (xi + 6.0, y[0], span),
                               (xi + 6.0, y[1], -span))),
            ("ring +z", sheet((0.4, 1.6 * r, z1 + 0.5 * g), (-span, y[0], z1 - 6.0), (span, y[0], z1 - 6.0),
                               (-span, y[1], z1 - 6.0)))]
    out[f"{scene_name}-ring"] = dict(cams=ring, ring=True, frame=(32, 16), spp=3)
    on = [("on xi", _plane_fan(0, xi, 4.0 * r, far, span, (0,), y=y)),
          ("on xi back", _plane_fan(0, xi, 1.0 * r, far, span, (0,), flip=True, y=y))]
    out[f"{scene_name}-on-xi"] = dict(cams=on, zero=(0,), on_xi=True, frame=(32, 16), spp=2)
    # an eye outside the grid box whose centre ray passes through a corner of the inner box
    cams = []
    for (px, pz), (sx, sz) in (((xi, zi), (1.0, 1.0)), ((x1, zi), (-1.0, 1.0)), ((x1, z1), (-1.0, -0.5))):
        eye = np.array((px - 3.0 * sx, 1.5 * r, pz - 3.0 * sz))
        mid = eye + 4.0 * (np.array((px, r, pz)) - eye)  # the centre target: beyond the corner on that line
        side = np.array((sz, 0.0, -sx)) * 6.0
        a = mid - 0.5 * side - np.array((0.0, r, 0.0))
        cams.append((f"corner {sx:+.0f}{sz:+.1f}", sheet(eye, a, a + side, a + np.array((0.0, 2.0 * r, 0.0)))))
    out[f"{scene_name}-corner"] = dict(cams=cams, outside=True, frame=(32, 16), spp=3)
    for c in out.values():
        c.update(scene=scene_name, model=CPU)
    return out


def _far(scene_name, look=(13.0, 2.0, 3.0)):
    """Origins beyond oref: two whole-far pinholes and a lens straddling oref2."""
    oref = oref_of(scene_name)
    u = np.array(look) / np.linalg.norm(look)
    out = {}
    for nm, mul, vfov in (("far1.2", 1.2, 12.0), ("far5", 5.0, 3.0)):
        cam = rtow.camera_cpu(lookfrom=tuple(mul * oref * u), lookat=(0, 0, 0), vfov=vfov, aspect=2.0, aperture=0.0,
                              focus_dist=mul * oref)
        out[f"{scene_name}-{nm}"] = dict(cams=[(nm, cam)], far="whole")
    out[f"{scene_name}-far-mixed"] = dict(cams=[("mixed", mixed_camera(scene_name, math.sqrt(0.99), look))], far="mixed",
                                           look=look)
    for c in out.values():
        c.update(scene=scene_name, frame=(32, 16), spp=4, model=CPU)
    return out


def mixed_camera(scene_name, mul, look=(13.0, 2.0, 3.0)):
    """The CPU-model lens camera at mul * oref from the world origin, with
    lens_u of length 2 along the radial direction and lens_v of length 2
    across it: at mul = sqrt(0.99) its origins straddle oref2."""
    oref = oref_of(scene_name)
    u = np.array(look) / np.linalg.norm(look)
    across = np.cross(u, (0.0, 1.0, 0.0))
    across /= np.linalg.norm(across)
    base = rtow.camera_cpu(lookfrom=tuple(mul * oref * u), lookat=(0, 0, 0), vfov=14.0, aspect=2.0, aperture=0.0,
                           focus_dist=mul * oref)
    return fan(base.eye[:], base.corner[:], base.horiz[:], base.vert[:], CPU, tuple(2.0 * u), tuple(2.0 * across))


def _plain_bvh(scene_name):
    """Zero-component fans and single rays for a scene that walks the plain BVH."""
    sc = scene_of(scene_name)
    small = np.nonzero(np.abs(sc.radius) < 10.0)[0]
    pick = small[[0, len(small) // 2, -1]]  # three spheres to aim at: (x, y, z) of their centres
    spots3 = [(float(sc.cx[i]), float(sc.cy[i]), float(sc.cz[i])) for i in pick]
    spots = [(x, z) for x, _, z in spots3] + [(float(sc.cx[pick[0]]) + 0.13, float(sc.cz[pick[0]]) - 0.07)]
    ext = float(max(np.abs(sc.cx[small]).max(), np.abs(sc.cz[small]).max()))
    top_y = float((sc.cy[small] + np.abs(sc.radius[small])).max())
    ground = int(np.argmax(np.abs(sc.radius)))  # "up" rays start inside the ground sphere, just under its top
    floor, top = float(sc.cy[ground] + abs(sc.radius[ground])) - 0.5, top_y + 1.0
    eye_y, far, span, y = 0.6 * top_y, ext + 2.0, ext + 0.5, (0.0, top_y)
    out = {}
    for axis, nm in ((0, "dx0"), (2, "dz0")):
        mk = lambda at, neg=False, flip=False: _plane_fan(axis, at, eye_y, far, span, (axis,), neg, flip, y=y)
        at = spots[1][0 if axis == 0 else 1]
        out[f"{scene_name}-{nm}"] = dict(cams=[("at0", mk(0.0)), ("at0 back", mk(0.0, flip=True)), ("sphere", mk(at))],
                                        zero=(axis,))
        out[f"{scene_name}-{nm}-neg"] = dict(cams=[("-0", mk(0.0, True)), ("-0 back", mk(0.0, True, True))],
                                            zero=(axis,), neg=True)
    half = span
    out[f"{scene_name}-dy0"] = dict(cams=[("a", _slab_fan(0.5 * (y[0] + y[1]), (far, 0.3 * far), half)),
                                          ("b", _slab_fan(y[1] * 0.4, (-0.2 * far, far), half))], zero=(1,))
    out[f"{scene_name}-dy0-neg"] = dict(cams=[("-0", _slab_fan(0.0, (far, 0.3 * far), half, True))], zero=(1,), neg=True)
    for c in out.values():
        c.update(frame=(32, 16), spp=3)
    rays = [(f"down {x:.2f} {z:.2f}", single((x, top, z), (0.0, -1.0, 0.0))) for x, z in spots]
    rays += [(f"up {x:.2f} {z:.2f}", single((x, floor, z), (0.0, 1.0, 0.0))) for x, z in spots]
    rays += [("down -0", single((0.0, top, 0.0), (0.0, -1.0, 0.0), neg=(0, 2)))]
    out[f"{scene_name}-vertical"] = dict(cams=rays, zero=(0, 2), neg="some", frame=(8, 8), spp=2)
    rays = []
    for x, h, z in spots3[:2]:
        rays += [(f"+x {z:.2f}", single((-far, h, z), (1.0, 0.0, 0.0))),
                 (f"-x {z:.2f}", single((far, h, z), (-1.0, 0.0, 0.0)))]
    out[f"{scene_name}-along-x"] = dict(cams=rays, zero=(1, 2), frame=(8, 8), spp=2)
    rays = []
    for x, h, z in spots3[:2]:
        rays += [(f"+z {x:.2f}", single((x, h, -far), (0.0, 0.0, 1.0))),
                 (f"-z {x:.2f}", single((x, h, far), (0.0, 0.0, -1.0)))]
    out[f"{scene_name}-along-z"] = dict(cams=rays, zero=(0, 1), frame=(8, 8), spp=2)
    for c in out.values():
        c.update(scene=scene_name, model=CPU)
    return out


def _build():
    cases = {}
    for name in LAYER_SCENES:
        cases.update(_zero_fans(name))
        cases.update(_two_zero(name))
        cases.update(_grid_fans(name))
        cases.update(_far(name))
    cases.update(_zero_fans("final", GPU))
    for name in ("final17", "five"):
        cases.update(_plain_bvh(name))
        cases.update(_far(name, (13.0, 2.0, 3.0) if name == "final17" else (-2.0, 1.0, 3.0)))
    for i, c in enumerate(cases.values()):
        c.setdefault("seed", 500 + i)
    return cases


_CASES = None


def cases():
    """{name: case}, built once (it reads the scenes and their grids through librtow.so on the host)."""
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def cases_of(scene_name):
    return {k: c for k, c in cases().items() if c["scene"] == scene_name}


def params_of(case, interval=0, accel=0, extra_flags=0, max_depth=DEPTH):
    w, h = case["frame"]
    flags = accel | interval | extra_flags | (rtow.RT_FLAG_GPU_SEMANTICS if case["model"] == GPU else 0)
    return rtow.make_params(w, h, case["spp"], max_depth=max_depth, seed=case["seed"], flags=flags)


_WANT, _TERMS = {}, {}


def want_of(name, i, interval):
    """kernel_render of camera i of a case with that interval flag, computed once: (sums, segments)."""
    key = (name, i, interval)
    if key not in _WANT:
        c = cases()[name]
        img, segs = oracle_lib.kernel_render(scene_of(c["scene"]), c["cams"][i][1], params_of(c, interval))
        img.setflags(write=False)
        _WANT[key] = (img, segs)
    return _WANT[key]


def terminals_of(name, i, max_bounces, keep_dir=False):
    """kernel_terminals of camera i of a case (closed interval), computed once."""
    key = (name, i, int(max_bounces), bool(keep_dir))
    if key not in _TERMS:
        c = cases()[name]
        t = oracle_lib.kernel_terminals(scene_of(c["scene"]), c["cams"][i][1], params_of(c), max_bounces, 0.0, keep_dir)
        t.setflags(write=False)
        _TERMS[key] = t
    return _TERMS[key]
