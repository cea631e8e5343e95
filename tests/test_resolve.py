"""The clamped temporal resolve with centre reprojection (include/rt_resolve.h,
librtow_resolve.so), host side: the fifth library's exported surface, its
argument handling on paths that need no device, the accuracy of the centre rays
the host builds from a camera, and properties of the numpy restatement
(tests/resolve_ref.py) that the GPU tests compare the kernel with bit for bit
-- so that it is more than a mirror of it.  The pass itself runs in
test_resolve_gpu.py, which runs the check_* functions below on the device too."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import resolve_ref as ref
import temporal_ref as tref
from test_temporal import VIEW_FRAMES, _cameras, _targets64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
F = np.float32
SPP = 4
INF = float("inf")
OFF = dict(plane_tol=INF, normal_cos=-1.0, gamma=INF)


def test_resolve_library_exports_every_declared_symbol(rtow):
    """Every function include/rt_resolve.h declares is a defined text symbol
    of librtow_resolve.so, the header carries its own version, and the library
    needs librtow.so and not librtow_temporal.so."""
    with open(os.path.join(ROOT, "include", "rt_resolve.h")) as f:
        text = f.read()
    names = sorted(set(re.findall(DECL, text, re.M)))
    assert names == ["rt_resolve", "rt_resolve_async", "rt_resolve_rays_from_camera", "rt_resolve_version"], names
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.RESOLVE_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}$", out, re.M), n
    assert not re.search(r"\brt_temporal", out)
    assert re.search(r"^#define RT_RESOLVE_VERSION 1$", text, re.M)
    assert rtow.resolve_lib().rt_resolve_version() == rtow.RESOLVE_VERSION == 1
    needed = subprocess.run(["readelf", "-d", rtow.RESOLVE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "librtow.so" in needed and "librtow_temporal" not in needed


def test_resolve_lives_in_its_own_library_only(rtow):
    """The four other libraries export no rt_resolve* symbol, and their
    headers do not name one."""
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH, rtow.DENOISE_LIB_PATH, rtow.TEMPORAL_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert not re.search(r"\brt_resolve", out), path
    for header in ("rt.h", "rt_internal.h", "rt_aov.h", "rt_denoise.h", "rt_temporal.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            assert "rt_resolve" not in f.read(), header
    assert rtow.lib().rt_abi_version() == 6 and rtow.aov_lib().rt_aov_version() == 1
    assert rtow.denoise_lib().rt_denoise_version() == 1 and rtow.temporal_lib().rt_temporal_version() == 1


def test_resolve_mirrors_have_the_headers_layout(rtow):
    """rtow.ResolveRays is rt_resolve_rays (twelve floats) and rtow.ResolveDesc
    is rt_resolve_desc: nine 4-byte fields, the view, the rays, four bytes of
    padding, then seven pointers."""
    R, D = rtow.ResolveRays, rtow.ResolveDesc
    assert ctypes.sizeof(R) == 48
    assert [(f[0], getattr(R, f[0]).offset) for f in R._fields_] == [("eye", 0), ("d00", 12), ("du", 24), ("dv", 36)]
    assert ctypes.sizeof(D) == 144 + 7 * 8
    assert [f[0] for f in D._fields_] == ["width", "height", "spp", "max_len", "plane_tol", "normal_cos", "gamma",
                                          "flags", "reserved", "prev", "now", "cur", "hits", "depth", "normal",
                                          "history_in", "history_out", "out"]
    assert (D.plane_tol.offset, D.gamma.offset, D.flags.offset, D.reserved.offset, D.prev.offset, D.now.offset,
            D.cur.offset, D.out.offset) == (16, 24, 28, 32, 36, 92, 144, 192)
    assert rtow.RESOLVE_KEEP_PARTIAL == ref.KEEP_PARTIAL == 1
    with open(os.path.join(ROOT, "include", "rt_resolve.h")) as f:
        assert re.search(r"^#define RT_RESOLVE_KEEP_PARTIAL 1u", f.read(), re.M)


def _valid_desc(rtow, keep, w=8, h=4, spp=4, **options):
    """A desc whose pointers are real host arrays (never dereferenced: the
    calls below are rejected first)."""
    d = rtow.resolve_desc(w, h, spp, ref.IDENTITY_VIEW, ref.IDENTITY_RAYS, **options)
    for name in rtow.RESOLVE_BUFFERS:
        a = np.zeros((3, h, w, 4), np.float32)
        keep.append(a)
        setattr(d, name, a.ctypes.data)
    return d


def test_resolve_null_range_and_overlap_arguments_are_invalid(rtow):
    """NULL context / desc / buffer, a frame size, an spp or an option out of
    range or NaN, an unknown flag, reserved != 0, overlapping buffers:
    RT_ERR_INVALID from both entry points before any HIP call and before the
    context is touched (no device here; the stand-in for a context is never
    read).  out == cur: invalid for the device entry point (test_resolve_gpu.py
    has the synchronous one, which accepts it)."""
    L = rtow.resolve_lib()
    keep = []
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    ms = ctypes.c_double(-1.0)

    def rejected(d, c=ctx):
        p = ctypes.byref(d) if d is not None else None
        return (L.rt_resolve(c, p, ctypes.byref(ms)) == rtow.RT_ERR_INVALID and
                L.rt_resolve(c, p, None) == rtow.RT_ERR_INVALID and
                L.rt_resolve_async(c, p, None) == rtow.RT_ERR_INVALID)

    good = _valid_desc(rtow, keep)
    assert rejected(good, c=None) and rejected(None)
    for name in ("cur", "hits", "depth", "normal", "history_out"):
        d = _valid_desc(rtow, keep)
        setattr(d, name, None)
        assert rejected(d), name
    nan = float("nan")
    for field, values in (("width", (0, -1, 32769)), ("height", (0, -3, 32769)), ("spp", (0, -1)),
                          ("max_len", (-1, 1025)), ("plane_tol", (-0.1, nan, -INF)),
                          ("normal_cos", (-1.5, 1.25, nan, INF)), ("gamma", (-1.0, nan, -INF)),
                          ("flags", (2, 3, 0x80000000)), ("reserved", (1, -1))):
        for v in values:
            d = _valid_desc(rtow, keep)
            setattr(d, field, v)
            assert rejected(d), (field, v)
    for other in ("history_in", "cur", "out", "hits", "depth", "normal"):  # history_out on or across `other`
        for shift in (0, 16, -16):
            d = _valid_desc(rtow, keep)
            d.history_out = getattr(d, other) + shift
            assert rejected(d), (other, shift)
    for shift in (0, 16, -16):  # out on or across history_in
        d = _valid_desc(rtow, keep)
        d.out = d.history_in + shift
        assert rejected(d), ("out / history_in", shift)
    for shift in (16, -16):  # out across cur: both entry points
        d = _valid_desc(rtow, keep)
        d.out = d.cur + shift
        assert rejected(d), ("out / cur", shift)
    d = _valid_desc(rtow, keep)  # out == cur: the device entry point
    d.out = d.cur
    assert L.rt_resolve_async(ctx, ctypes.byref(d), None) == rtow.RT_ERR_INVALID
    for name in ("history_in", "history_out"):  # not 16-byte aligned: the device entry point only
        d = _valid_desc(rtow, keep)
        setattr(d, name, getattr(d, name) + 4)
        assert L.rt_resolve_async(ctx, ctypes.byref(d), None) == rtow.RT_ERR_INVALID, name
    assert ms.value == -1.0  # a rejected call writes nothing
    assert all(not a.any() for a in keep)
    assert standin.raw == bytes(64)


def test_resolve_python_options(rtow):
    """Unknown option or buffer names raise ValueError before any call; an
    option left out (or None) is the struct's 0 (= default), a given value
    means itself, an option of 0 raises; the rays are required."""
    class NoContext(rtow.Context):
        def __init__(self):  # no device: the name checks come before any call
            self._h = None

    ctx = NoContext()
    f = ref.identity_inputs(8, 4, SPP, np.zeros((4, 8, 3)))
    hist = np.zeros((3, 4, 8, 4), F)
    R, V = ref.IDENTITY_RAYS, ref.IDENTITY_VIEW
    with pytest.raises(ValueError):
        ctx.resolve(f["cur"], f, SPP, now_rays=R, alpha=0.2)
    with pytest.raises(ValueError):
        ctx.resolve(f["cur"], {"hits": f["hits"]}, SPP, now_rays=R)
    with pytest.raises(ValueError):
        ctx.resolve(f["cur"], f, SPP)  # no rays
    with pytest.raises(ValueError):
        ctx.resolve(f["cur"][:2], f, SPP, now_rays=R)
    with pytest.raises(ValueError):
        ctx.resolve(f["cur"], f, SPP, now_rays=R, history=hist)  # a history without its view
    with pytest.raises(ValueError):
        ctx.resolve(f["cur"], f, SPP, prev_view=V, now_rays=R, history=hist[:2])
    with pytest.raises(ValueError):
        ctx.resolve_async({"colour": 0}, 8, 4, SPP, None, R)
    with pytest.raises(ValueError):
        ctx.resolve_async({"position": 0}, 8, 4, SPP, None, R)  # rt_temporal's buffer, not this pass's
    with pytest.raises(ValueError):
        ctx.resolve_async({}, 8, 4, SPP, None, R, frames=3)
    for name in rtow.RESOLVE_DEFAULTS:
        with pytest.raises(ValueError):
            rtow.resolve_desc(8, 4, SPP, now_rays=R, **{name: 0})
    d = rtow.resolve_desc(8, 4, SPP, now_rays=R)
    assert (d.max_len, d.plane_tol, d.normal_cos, d.gamma, d.flags, d.reserved) == (0, 0.0, 0.0, 0.0, 0, 0)
    assert (list(d.now.d00), list(d.now.du), list(d.now.dv)) == ([0, 0, 1], [ref.STEP, 0, 0], [0, ref.STEP, 0])
    d = rtow.resolve_desc(8, 4, SPP, V, R, rtow.RESOLVE_KEEP_PARTIAL, max_len=3, plane_tol=INF, normal_cos=-1,
                          gamma=INF)
    assert (d.max_len, d.plane_tol, d.normal_cos, d.gamma, d.flags) == (3, INF, -1.0, INF, 1)
    assert (list(d.prev.px), list(d.prev.pw), d.prev.x0) == ([2.0 ** 20, 0, 0], [0, 0, 1], 0.0)
    d = rtow.resolve_desc(8, 4, SPP, now_rays=R, max_len=None, gamma=0.5)
    assert (d.max_len, d.gamma) == (0, 0.5)
    assert rtow.RESOLVE_DEFAULTS == ref.DEFAULTS
    assert rtow.RESOLVE_BUFFERS == ("cur", "hits", "depth", "normal", "history_in", "history_out", "out")


# ---- the rays -------------------------------------------------------------------
@pytest.mark.parametrize("frame", VIEW_FRAMES, ids=lambda f: "%dx%d" % f)
def test_rays_pass_through_the_pixel_the_view_returns(rtow, frame):
    """The cameras, frame sizes and pixels of test_temporal.py's view-accuracy
    test: the point eye + t normalize(D), D the fp32 centre ray as the kernel
    forms it, at t = 0.5, 1 and 3 times eye -> target, rounded to fp32,
    projected through rtow.temporal_view of the same camera, lands on (col,
    row) within that test's bound, 2^-7 pixel."""
    w, h = frame
    rng = np.random.default_rng(w)
    cols = np.concatenate([[0, w - 1, 0, w - 1, w // 2], rng.integers(0, w, 200)])
    rows = np.concatenate([[0, 0, h - 1, h - 1, h // 2], rng.integers(0, h, 200)])
    for name, cam in _cameras(rtow, w, h):
        rays, view = rtow.resolve_rays(cam, w, h), rtow.temporal_view(cam, w, h)
        assert list(rays.eye) == list(cam.eye)
        d00, du, dv = (np.array(list(v), F) for v in (rays.d00, rays.du, rays.dv))
        D = (d00 + cols.astype(F)[:, None] * du) + rows.astype(F)[:, None] * dv
        assert D.dtype == F
        D = D.astype(np.float64)
        u = D / np.linalg.norm(D, axis=-1, keepdims=True)
        eye = np.array(list(cam.eye), np.float64)
        dist = np.linalg.norm(_targets64(rtow, cam, w, h, cols, rows) - eye, axis=-1, keepdims=True)
        worst = 0.0
        for k in (0.5, 1.0, 3.0):
            P = (eye + k * dist * u).astype(F)
            _, wv, x, y = tref.project(view, P)
            assert (wv > 0).all(), name
            worst = max(worst, float(np.abs(x - cols).max()), float(np.abs(y - rows).max()))
        print(f"rays {w}x{h} {name}: worst deviation {worst:.3e} pixel (bound {2.0 ** -7:.3e})")
        assert worst <= 2.0 ** -7, (name, worst)


def test_rays_builder_rejects_what_the_view_builder_rejects(rtow):
    L = rtow.resolve_lib()
    cam = rtow.camera_cpu()
    out = rtow.ResolveRays()
    before = bytes(out)

    def status(c, w=64, h=36, o=out):
        return L.rt_resolve_rays_from_camera(ctypes.byref(c) if c is not None else None, w, h,
                                             ctypes.byref(o) if o is not None else None)

    assert status(cam) == 0 and bytes(out) != before
    out = rtow.ResolveRays()
    assert status(None, o=out) == rtow.RT_ERR_INVALID and status(cam, o=None) == rtow.RT_ERR_INVALID
    for w, h in ((0, 36), (64, 0), (-2, 36), (32769, 36), (64, 32769), (1, 36), (64, 1)):
        assert status(cam, w, h, out) == rtow.RT_ERR_INVALID, (w, h)
    assert bytes(out) == before
    gpu = rtow.camera_gpu(64, 36)
    ok = rtow.ResolveRays()
    assert status(gpu, 1, 1, ok) == 0  # the GPU model has no W-1
    assert (list(ok.du), list(ok.dv)) == (list(gpu.horiz), list(gpu.vert))
    assert list(ok.d00) == [float(F(np.float64(c) - np.float64(e))) for c, e in zip(gpu.corner, gpu.eye)]

    def broken(edit):
        c = rtow.Camera.from_buffer_copy(cam)
        edit(c)
        return c

    def setv(field, values):
        return lambda c: setattr(c, field, (ctypes.c_float * 3)(*values))

    cases = {
        "model": lambda c: setattr(c, "model", 7),
        "nan eye": setv("eye", (float("nan"), 0, 0)),
        "inf corner": setv("corner", (INF, 0, 0)),
        "inf horiz": setv("horiz", (INF, 0, 0)),
        "nan vert": setv("vert", (0, float("nan"), 0)),
    }
    for name, edit in cases.items():
        assert status(broken(edit), o=out) == rtow.RT_ERR_INVALID, name
    assert bytes(out) == before  # a rejected call writes nothing


# ---- properties of the restatement (and, through test_resolve_gpu.py, of the device) ----
W, H = 13, 7
ID = dict(rays=ref.IDENTITY_RAYS)


def colours(n, seed=3):
    rng = np.random.default_rng(seed)
    return [(rng.random((H, W, 3)) * 2).astype(F) for _ in range(n)]


def check_running_mean(step, max_len):
    """With the identity pair every pixel finds its own history with weights
    1, 0, 0, 0: with the clamp off the mean follows h + (c - h) * (1 / len) bit
    for bit and len = min(N, max_len) exactly."""
    cols = colours(6)
    hist = mean = None
    for i, col in enumerate(cols):
        f = ref.identity_inputs(W, H, SPP, col)
        out, hist = step(spp=SPP, prev=None if hist is None else ref.IDENTITY_VIEW, history=hist, max_len=max_len,
                         gamma=INF, **ID, **f)
        c = (col * F(SPP)).astype(F) / F(SPP)
        ln = F(min(i + 1, max_len))
        mean = c if mean is None else mean + (c - mean) * (F(1) / ln)
        assert mean.dtype == F
        assert np.array_equal(hist[0, ..., 3], np.full((H, W), ln)), i
        assert hist[0, ..., :3].tobytes() == mean.tobytes(), i
        assert out.tobytes() == (mean * F(SPP)).tobytes(), i
        yy, xx = np.mgrid[0:H, 0:W]
        assert np.array_equal(hist[1, ..., 0], (xx * ref.STEP).astype(F)) and np.array_equal(hist[1, ..., 2], np.ones((H, W)))
        assert np.array_equal(hist[1, ..., 3], np.zeros((H, W))) and np.array_equal(hist[2, ..., 2], np.ones((H, W)))


@pytest.mark.parametrize("max_len", [1, 3, 32])
def test_ref_running_mean(max_len):
    check_running_mean(ref.resolve_ref, max_len)


def check_partial_restarts(step):
    """A pixel with hits = spp - 1 restarts (len 1, m = c) while its
    neighbours accumulate; with KEEP_PARTIAL it accumulates like them."""
    c0, c1 = colours(2, seed=5)
    _, hist = step(spp=SPP, **ID, **ref.identity_inputs(W, H, SPP, c0))
    hits = np.full((H, W), SPP, np.uint32)
    hits[2, 5] = hits[6, 12] = SPP - 1
    part = hits < SPP
    f = ref.identity_inputs(W, H, SPP, c1, hits)
    c = f["cur"] / F(SPP)
    m0 = hist[0, ..., :3]
    blend = m0 + (c - m0) * (F(1) / F(2))
    _, h1 = step(spp=SPP, prev=ref.IDENTITY_VIEW, history=hist, gamma=INF, **ID, **f)
    assert np.array_equal(h1[0, ..., 3], np.where(part, F(1), F(2)))
    assert h1[0, ..., :3].tobytes() == np.where(part[..., None], c, blend).tobytes()
    _, h2 = step(spp=SPP, prev=ref.IDENTITY_VIEW, history=hist, gamma=INF, flags=ref.KEEP_PARTIAL, **ID, **f)
    assert np.array_equal(h2[0, ..., 3], np.full((H, W), 2, F)) and h2[0, ..., :3].tobytes() == blend.tobytes()


def test_ref_partial_restarts():
    check_partial_restarts(ref.resolve_ref)


def check_flat_neighbourhood(step):
    """A flat cur has sd = 0 (0.75, 0.5, 0.25: every sum of up to nine of
    them, and of their squares, is exact), so lo = hi = c and a history of any
    other colour comes out as exactly cur, whatever max_len; the length still
    counts."""
    flat = np.broadcast_to(np.array([0.75, 0.5, 0.25], F), (H, W, 3))
    _, hist = step(spp=SPP, **ID, **ref.identity_inputs(W, H, SPP, colours(1, seed=7)[0]))
    hist = hist.copy()
    hist[0, ..., :3] = colours(1, seed=8)[0] * F(50) - F(20)
    f = ref.identity_inputs(W, H, SPP, flat)
    for max_len in (1, 3, 32):
        out, h1 = step(spp=SPP, prev=ref.IDENTITY_VIEW, history=hist, max_len=max_len, **ID, **f)
        assert h1[0, ..., :3].tobytes() == flat.tobytes(), max_len
        assert out.tobytes() == f["cur"].tobytes(), max_len
        assert np.array_equal(h1[0, ..., 3], np.full((H, W), min(2, max_len), F))


def test_ref_flat_neighbourhood():
    check_flat_neighbourhood(ref.resolve_ref)


def _bounds(c, i, j, gamma):
    """lo, hi, k of pixel (col i, row j), pixel by pixel (not resolve_ref's code)."""
    m1, m2, k = np.zeros(3, F), np.zeros(3, F), 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if 0 <= i + dx < W and 0 <= j + dy < H:
                cq = c[j + dy, i + dx]
                m1, m2, k = m1 + cq, m2 + cq * cq, k + 1
    mu = m1 / F(k)
    v = m2 / F(k) - mu * mu
    sd = np.sqrt(np.where(v > 0, v, F(0)))
    lo, hi = mu - F(gamma) * sd, mu + F(gamma) * sd
    assert lo.dtype == F and hi.dtype == F
    return lo, hi, k


def check_clamp(step):
    """A history colour inside [lo, hi] is untouched (the bits of gamma =
    +inf); one above hi enters the blend as exactly hi and one below lo as
    exactly lo; corner pixels take their bounds from 4 pixels, edge pixels
    from 6, the others from 9."""
    c0, c1 = colours(2, seed=9)
    gamma = 1.5
    f = ref.identity_inputs(W, H, SPP, c1)
    c = f["cur"] / F(SPP)
    lo, hi, ks = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F), np.zeros((H, W), int)
    for j in range(H):
        for i in range(W):
            lo[j, i], hi[j, i], ks[j, i] = _bounds(c, i, j, gamma)
    assert ks[0, 0] == ks[H - 1, W - 1] == 4 and ks[0, 3] == ks[3, 0] == ks[H - 1, 5] == 6 and ks[3, 3] == 9
    assert sorted(np.unique(ks)) == [4, 6, 9] and (hi > lo).all()
    _, hist = step(spp=SPP, **ID, **ref.identity_inputs(W, H, SPP, c0))
    half = F(1) / F(2)

    def run(colour, **opt):
        h = hist.copy()
        h[0, ..., :3] = colour
        return step(spp=SPP, prev=ref.IDENTITY_VIEW, history=h, **opt, **ID, **f)[1]

    inside = (lo + (hi - lo) * half).astype(F)
    assert ((inside >= lo) & (inside <= hi)).all()
    a, b = run(inside, gamma=gamma), run(inside, gamma=INF)
    assert a.tobytes() == b.tobytes()
    assert a[0, ..., :3].tobytes() == (inside + (c - inside) * half).tobytes()
    above = run(hi + F(1), gamma=gamma)
    assert above[0, ..., :3].tobytes() == (hi + (c - hi) * half).tobytes()
    below = run(lo - F(1), gamma=gamma)
    assert below[0, ..., :3].tobytes() == (lo + (c - lo) * half).tobytes()
    mixed = np.stack([hi[..., 0] + F(1), inside[..., 1], lo[..., 2] - F(1)], -1)  # per channel
    want = np.stack([hi[..., 0], inside[..., 1], lo[..., 2]], -1)
    assert run(mixed, gamma=gamma)[0, ..., :3].tobytes() == (want + (c - want) * half).tobytes()
    assert np.array_equal(above[0, ..., 3], np.full((H, W), 2, F))


def test_ref_clamp():
    check_clamp(ref.resolve_ref)


def test_ref_histories_pass_between_temporal_and_resolve():
    """A history written by temporal_ref is accepted here, and a history
    written here is accepted by temporal_ref: with the identity pair (and the
    matching position sums for temporal_ref) every pixel accumulates, bit for
    bit the blend of the other pass's mean."""
    c0, c1 = colours(2, seed=11)
    pos = ref.identity_positions(W, H, SPP)
    f0, f1 = ref.identity_inputs(W, H, SPP, c0), ref.identity_inputs(W, H, SPP, c1)
    c = f1["cur"] / F(SPP)

    def temporal(f, **kw):
        return tref.temporal_ref(f["cur"], f["hits"], pos, f["normal"], SPP, **kw)

    _, ht = temporal(f0)
    _, hr = ref.resolve_ref(spp=SPP, **ID, **f0)
    assert ht.tobytes() == hr.tobytes()  # the same three planes from either pass
    for h1 in (ref.resolve_ref(spp=SPP, prev=ref.IDENTITY_VIEW, history=ht, gamma=INF, **ID, **f1)[1],
               temporal(f1, prev=ref.IDENTITY_VIEW, history=hr)[1]):
        m0 = ht[0, ..., :3]
        assert np.array_equal(h1[0, ..., 3], np.full((H, W), 2, F))
        assert h1[0, ..., :3].tobytes() == (m0 + (c - m0) * (F(1) / F(2))).tobytes()
    # and with real options: the default tests and the clamp accept the other pass's history too
    _, h2 = ref.resolve_ref(spp=SPP, prev=ref.IDENTITY_VIEW, history=ht, **ID, **f1)
    assert np.array_equal(h2[0, ..., 3], np.full((H, W), 2, F))


def test_resolve_synthetic_inputs_reach_every_branch():
    """The seeded frame, history, view and rays of the GPU bit-equality test
    reach what the pass branches on (at 67x37, the frame the other sizes
    repeat)."""
    w, h = 67, 37
    frame, hist, view, rays = ref.synthetic_inputs(w, h, SPP, seed=1000 * w + h)
    hits = frame["hits"]
    assert (hits == 0).any() and ((hits > 0) & (hits < SPP)).any() and (hits == SPP).any()
    assert ((hits > 0) & (frame["normal"] == 0).all(-1)).any()  # a zero normal sum on geometry
    seen = {}
    for name, opt in (("defaults", {}), ("long", dict(max_len=32)), ("half", dict(gamma=0.5)),
                      ("keep", dict(flags=ref.KEEP_PARTIAL)), ("loose", dict(plane_tol=0.01)),
                      ("tight", dict(plane_tol=1e-4)), ("off", OFF)):
        c = {}
        ref.resolve_ref(spp=SPP, rays=rays, prev=view, history=hist, census=c, **opt, **frame)
        seen[name] = c
    c = seen["defaults"]
    geo = hits > 0
    assert c["partial"].any() and not (c["partial"] & c["ok"]).any()  # partial pixels restart ...
    assert (seen["keep"]["partial"] & seen["keep"]["valid"]).any()  # ... and keep their history when asked to
    assert (geo & ~(c["w"] > 0)).any()  # behind the previous eye
    assert (c["use"] & (c["w"] > 0) & ~c["ok"]).any()  # projected off the frame
    ok = c["ok"]
    assert (ok & (c["xi"] == -1)).any() and (ok & (c["xi"] == w - 1)).any()  # taps off the left / right border
    assert (ok & (c["yi"] == -1)).any() and (ok & (c["yi"] == h - 1)).any()  # top / bottom
    assert c["off_frame"] and c["sky_tap"] and c["plane"] and c["normal"]
    assert {1, 2, 3, 4} <= set(np.unique(c["taken"][c["valid"]]))
    assert (ok & ~c["valid"]).any()  # every tap rejected
    for name in ("defaults", "half"):
        s = seen[name]
        for kind in ("clamp_low", "clamp_high", "clamp_idle"):  # in every channel
            assert s[kind].any(axis=(0, 1)).all(), (name, kind)
        assert {4.0, 6.0, 9.0} <= set(np.unique(s["k"][s["valid"]])), name
    assert seen["half"]["clamp_idle"].sum() < c["clamp_idle"].sum()
    assert "k" not in seen["off"]  # the neighbourhood step is left out
    assert c["saturated"].any()  # (all of them at max_len = 2)
    assert seen["long"]["saturated"].any() and (seen["long"]["valid"] & ~seen["long"]["saturated"]).any()
    assert seen["tight"]["plane"] > c["plane"] >= seen["loose"]["plane"] > 0 and seen["tight"]["valid"].any()
    assert seen["off"]["plane"] == 0 and seen["off"]["normal"] == 0 and seen["off"]["sky_tap"]
