"""Temporal accumulation with reprojection (include/rt_temporal.h,
librtow_temporal.so), host side: the fourth library's exported surface, its
argument handling on paths that need no device, the accuracy of the view the
host builds from a camera, and properties of the numpy restatement
(tests/temporal_ref.py) that the GPU tests compare the kernel with bit for bit
-- so that it is more than a mirror of it.  The pass itself runs in
test_temporal_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
F = np.float32
SPP = 4
INF = float("inf")
OFF = dict(plane_tol=INF, normal_cos=-1.0)


def test_temporal_library_exports_every_declared_symbol(rtow):
    """Every function include/rt_temporal.h declares is a defined text symbol
    of librtow_temporal.so, and the header carries its own version."""
    with open(os.path.join(ROOT, "include", "rt_temporal.h")) as f:
        text = f.read()
    names = sorted(set(re.findall(DECL, text, re.M)))
    assert names == ["rt_temporal", "rt_temporal_async", "rt_temporal_history_bytes", "rt_temporal_version",
                     "rt_temporal_view_from_camera"], names
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.TEMPORAL_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}$", out, re.M), n
    assert re.search(r"^#define RT_TEMPORAL_VERSION 1$", text, re.M)
    assert rtow.temporal_lib().rt_temporal_version() == rtow.TEMPORAL_VERSION == 1


def test_temporal_lives_in_its_own_library_only(rtow):
    """The three other libraries export no rt_temporal* symbol, and their
    headers do not declare one."""
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH, rtow.DENOISE_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert not re.search(r"\brt_temporal", out), path
    for header in ("rt.h", "rt_internal.h", "rt_aov.h", "rt_denoise.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            assert "rt_temporal" not in f.read(), header
    assert rtow.lib().rt_abi_version() == 6 and rtow.aov_lib().rt_aov_version() == 1
    assert rtow.denoise_lib().rt_denoise_version() == 1


def test_temporal_mirrors_have_the_headers_layout(rtow):
    """rtow.TemporalView is rt_temporal_view (fourteen floats) and
    rtow.TemporalDesc is rt_temporal_desc: eight 4-byte fields, the view, then
    seven pointers."""
    V, D = rtow.TemporalView, rtow.TemporalDesc
    assert ctypes.sizeof(V) == 56
    assert [(f[0], getattr(V, f[0]).offset) for f in V._fields_] == [("eye", 0), ("px", 12), ("py", 24), ("pw", 36),
                                                                     ("x0", 48), ("y0", 52)]
    assert ctypes.sizeof(D) == 32 + 56 + 7 * 8
    assert [f[0] for f in D._fields_] == ["width", "height", "spp", "max_len", "plane_tol", "normal_cos", "reserved",
                                          "prev", "cur", "hits", "position", "normal", "history_in", "history_out",
                                          "out"]
    assert (D.plane_tol.offset, D.reserved.offset, D.prev.offset, D.cur.offset, D.out.offset) == (16, 24, 32, 88, 136)


def _valid_desc(rtow, keep, w=8, h=4, spp=4, **options):
    """A desc whose pointers are real host arrays (never dereferenced: the
    calls below are rejected first)."""
    d = rtow.temporal_desc(w, h, spp, ref.IDENTITY, **options)
    for name in rtow.TEMPORAL_BUFFERS:
        a = np.zeros((3, h, w, 4), np.float32)
        keep.append(a)
        setattr(d, name, a.ctypes.data)
    return d


def test_temporal_null_range_and_overlap_arguments_are_invalid(rtow):
    """NULL context / desc / buffer, a frame size, an spp or an option out of
    range or NaN, reserved != 0, overlapping histories: RT_ERR_INVALID from
    both entry points before any HIP call and before the context is touched
    (no device here; the stand-in for a context is never read)."""
    L = rtow.temporal_lib()
    keep = []
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    ms = ctypes.c_double(-1.0)

    def rejected(d, c=ctx):
        p = ctypes.byref(d) if d is not None else None
        return (L.rt_temporal(c, p, ctypes.byref(ms)) == rtow.RT_ERR_INVALID and
                L.rt_temporal(c, p, None) == rtow.RT_ERR_INVALID and
                L.rt_temporal_async(c, p, None) == rtow.RT_ERR_INVALID)

    good = _valid_desc(rtow, keep)
    assert rejected(good, c=None) and rejected(None)
    for name in ("cur", "hits", "position", "normal", "history_out"):
        d = _valid_desc(rtow, keep)
        setattr(d, name, None)
        assert rejected(d), name
    nan = float("nan")
    for field, values in (("width", (0, -1, 32769)), ("height", (0, -3, 32769)), ("spp", (0, -1)),
                          ("max_len", (-1, 1025)), ("plane_tol", (-0.1, nan, -INF)),
                          ("normal_cos", (-1.5, 1.25, nan, INF))):
        for v in values:
            d = _valid_desc(rtow, keep)
            setattr(d, field, v)
            assert rejected(d), (field, v)
    for k in (0, 1):
        d = _valid_desc(rtow, keep)
        d.reserved[k] = 1
        assert rejected(d), ("reserved", k)
    for other in ("history_in", "cur", "out"):  # history_out == other, and overlapping it from either side
        for shift in (0, 16, -16):
            d = _valid_desc(rtow, keep)
            d.history_out = getattr(d, other) + shift
            assert rejected(d), (other, shift)
    d = _valid_desc(rtow, keep)  # history_out not 16-byte aligned: the device path only
    d.history_out += 4
    assert L.rt_temporal_async(ctx, ctypes.byref(d), None) == rtow.RT_ERR_INVALID
    assert ms.value == -1.0  # a rejected call writes nothing
    assert all(not a.any() for a in keep)
    assert standin.raw == bytes(64)
    assert L.rt_temporal_history_bytes(67, 37) == 48 * 67 * 37
    assert L.rt_temporal_history_bytes(3840, 2160) == 48 * 3840 * 2160
    for w, h in ((0, 4), (4, 0), (-1, 4), (32769, 1), (1, 32769)):
        assert L.rt_temporal_history_bytes(w, h) == 0


def test_temporal_python_options(rtow):
    """Unknown option or buffer names raise ValueError before any call; an
    option left out (or None) is the struct's 0 (= default), a given value
    means itself."""
    class NoContext(rtow.Context):
        def __init__(self):  # no device: the name checks come before any call
            self._h = None

    ctx = NoContext()
    f = ref.identity_inputs(8, 4, SPP, np.zeros((4, 8, 3)))
    hist = np.zeros((3, 4, 8, 4), F)
    with pytest.raises(ValueError):
        ctx.temporal(f["cur"], f, SPP, alpha=0.2)
    with pytest.raises(ValueError):
        ctx.temporal(f["cur"], {"hits": f["hits"]}, SPP)
    with pytest.raises(ValueError):
        ctx.temporal(f["cur"][:2], f, SPP)
    with pytest.raises(ValueError):
        ctx.temporal(f["cur"], f, SPP, history=hist)  # a history without its view
    with pytest.raises(ValueError):
        ctx.temporal(f["cur"], f, SPP, prev_view=ref.IDENTITY, history=hist[:2])
    with pytest.raises(ValueError):
        ctx.temporal_async({"colour": 0}, 8, 4, SPP, None)
    with pytest.raises(ValueError):
        ctx.temporal_async({}, 8, 4, SPP, None, frames=3)
    for name in rtow.TEMPORAL_DEFAULTS:
        with pytest.raises(ValueError):
            rtow.temporal_desc(8, 4, SPP, **{name: 0})
    d = rtow.temporal_desc(8, 4, SPP)
    assert (d.max_len, d.plane_tol, d.normal_cos, list(d.reserved)) == (0, 0.0, 0.0, [0, 0])
    d = rtow.temporal_desc(8, 4, SPP, ref.IDENTITY, max_len=3, plane_tol=INF, normal_cos=-1, )
    assert (d.max_len, d.plane_tol, d.normal_cos) == (3, INF, -1.0)
    assert (list(d.prev.px), list(d.prev.py), list(d.prev.pw), d.prev.x0) == ([1, 0, 0], [0, 1, 0], [0, 0, 1], 0.0)
    d = rtow.temporal_desc(8, 4, SPP, max_len=None, normal_cos=0.5)
    assert (d.max_len, d.normal_cos) == (0, 0.5)
    assert rtow.TEMPORAL_DEFAULTS == ref.DEFAULTS


# ---- the view ------------------------------------------------------------------
VIEW_FRAMES = ((67, 37), (400, 225), (3840, 2160))
LOOKFROM, LOOKAT = (13.0, 2.0, 3.0), (0.0, 0.0, 0.0)


def _cameras(rtow, w, h):
    for deg in (0.0, 7.0):
        frm = ref.orbit(LOOKFROM, LOOKAT, deg)
        yield f"cpu, {deg} deg", rtow.camera_cpu(lookfrom=frm, lookat=LOOKAT, aspect=w / h)
        yield f"gpu, {deg} deg", rtow.camera_gpu(w, h, lookfrom=frm, lookat=LOOKAT)


def _targets64(rtow, cam, w, h, cols, rows):
    """camera_dir's target of the pixel centres (u1 = u2 = 0.5), in fp64 from
    the camera's fp32 fields (the CPU model's 1/(W-1) rounded to fp32 as the
    device holds it)."""
    corner, horiz, vert = (np.array(list(v), np.float64) for v in (cam.corner, cam.horiz, cam.vert))
    if cam.model == rtow.RT_CAMERA_CPU:
        fs = (cols + 0.5) * np.float64(F(1.0 / (w - 1)))
        ft = ((h - 1 - rows) + 0.5) * np.float64(F(1.0 / (h - 1)))
    else:
        fs, ft = cols.astype(np.float64), rows.astype(np.float64)
    return corner + fs[:, None] * horiz + ft[:, None] * vert


@pytest.mark.parametrize("frame", VIEW_FRAMES, ids=lambda f: "%dx%d" % f)
def test_view_returns_the_pixel_a_point_was_seen_through(rtow, frame):
    """Points at 0.5, 1 and 3 times eye -> target on the centre rays of the
    corner pixels, the centre pixel and 200 random ones, rounded to fp32 as
    the feature pass stores them: the fp32 formula of the header gives (col,
    row) back within 2^-7 pixel, and w > 0.  (A larger error would move the
    bilinear weights by about a percent; fp32 leaves about 12 bits below a
    4096-wide coordinate.)"""
    w, h = frame
    rng = np.random.default_rng(w)
    cols = np.concatenate([[0, w - 1, 0, w - 1, w // 2], rng.integers(0, w, 200)])
    rows = np.concatenate([[0, 0, h - 1, h - 1, h // 2], rng.integers(0, h, 200)])
    for name, cam in _cameras(rtow, w, h):
        view = rtow.temporal_view(cam, w, h)
        eye = np.array(list(cam.eye), np.float64)
        assert list(view.eye) == list(cam.eye)
        target = _targets64(rtow, cam, w, h, cols, rows)
        worst = 0.0
        for k in (0.5, 1.0, 3.0):
            P = (eye + k * (target - eye)).astype(F)
            _, wv, x, y = ref.project(view, P)
            assert (wv > 0).all(), name
            worst = max(worst, float(np.abs(x - cols).max()), float(np.abs(y - rows).max()))
        print(f"view {w}x{h} {name}: worst deviation {worst:.3e} pixel (bound {2.0 ** -7:.3e})")
        assert worst <= 2.0 ** -7, (name, worst)


def test_view_builder_rejects_what_it_cannot_project(rtow):
    L = rtow.temporal_lib()
    cam = rtow.camera_cpu()
    out = rtow.TemporalView()
    before = bytes(out)

    def status(c, w=64, h=36, o=out):
        return L.rt_temporal_view_from_camera(ctypes.byref(c) if c is not None else None, w, h,
                                              ctypes.byref(o) if o is not None else None)

    assert status(cam) == 0 and bytes(out) != before
    out = rtow.TemporalView()
    assert status(None, o=out) == rtow.RT_ERR_INVALID and status(cam, o=None) == rtow.RT_ERR_INVALID
    for w, h in ((0, 36), (64, 0), (-2, 36), (32769, 36), (64, 32769), (1, 36), (64, 1)):
        assert status(cam, w, h, out) == rtow.RT_ERR_INVALID, (w, h)
    gpu = rtow.camera_gpu(64, 36)
    assert status(gpu, 1, 1, out) == 0  # the GPU model has no W-1
    out = rtow.TemporalView()

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
        "zero horiz": setv("horiz", (0, 0, 0)),
        "vert parallel to horiz": lambda c: setattr(c, "vert", c.horiz),
        "eye in the image plane": lambda c: setattr(c, "eye", c.corner),
    }
    for name, edit in cases.items():
        assert status(broken(edit), o=out) == rtow.RT_ERR_INVALID, name
    assert bytes(out) == before  # a rejected call writes nothing


# ---- properties of the restatement ---------------------------------------------
W, H = 13, 7


def colours(n, seed=3):
    rng = np.random.default_rng(seed)
    return [(rng.random((H, W, 3)) * 2).astype(F) for _ in range(n)]


def run_frames(step, cols, max_len, shift=(0.0, 0.0)):
    """Feed the frames one after the other through `step` (temporal_ref, or
    the device's equivalent); -> the list of (out, history) per frame."""
    res, hist = [], None
    for c in cols:
        f = ref.identity_inputs(W, H, SPP, c, shift)
        out, hist = step(spp=SPP, prev=None if hist is None else ref.IDENTITY, history=hist, max_len=max_len, **f)
        res.append((out, hist))
    return res


def check_running_mean(step, max_len):
    """1. With the identity view every pixel finds its own history with
    weights 1, 0, 0, 0: the mean follows h + (c - h) * (1 / len) bit for bit
    and len = min(N, max_len) exactly."""
    cols = colours(6)
    res = run_frames(step, cols, max_len)
    mean = None
    for i, (c, (out, hist)) in enumerate(zip(cols, res)):
        n = i + 1
        c = (c * F(SPP)).astype(F) / F(SPP)
        ln = F(min(n, max_len))
        mean = c if mean is None else mean + (c - mean) * (F(1) / ln)
        assert mean.dtype == F
        assert np.array_equal(hist[0, ..., 3], np.full((H, W), ln)), n
        assert hist[0, ..., :3].tobytes() == mean.tobytes(), n
        assert out.tobytes() == (mean * F(SPP)).tobytes(), n
        assert np.array_equal(hist[1, ..., 3], np.zeros((H, W))) and np.array_equal(hist[2, ..., 2], np.ones((H, W)))


@pytest.mark.parametrize("max_len", [1, 3, 32])
def test_ref_running_mean(max_len):
    check_running_mean(ref.temporal_ref, max_len)


def check_shift(step):
    """2. P = (i + 1, j, 1): every pixel takes its right neighbour's history
    exactly; column W-1 projects to x = W, outside the frame, and restarts."""
    c0, c1 = colours(2, seed=5)
    _, hist = step(spp=SPP, **ref.identity_inputs(W, H, SPP, c0))
    out, h1 = step(spp=SPP, prev=ref.IDENTITY, history=hist, **ref.identity_inputs(W, H, SPP, c1, (1.0, 0.0)))
    m0, c = hist[0, ..., :3], (c1 * F(SPP)).astype(F) / F(SPP)
    want = m0[:, 1:] + (c[:, :-1] - m0[:, 1:]) * (F(1) / F(2))
    assert h1[0, :, :-1, :3].tobytes() == want.tobytes()
    assert np.array_equal(h1[0, :, :-1, 3], np.full((H, W - 1), 2, F))
    assert np.array_equal(h1[0, :, -1, 3], np.ones(H, F)) and h1[0, :, -1, :3].tobytes() == c[:, -1].tobytes()
    assert out.tobytes() == (h1[0, ..., :3] * F(SPP)).tobytes()


def test_ref_shift():
    check_shift(ref.temporal_ref)


def check_disocclusion(step, kind):
    """3. A history whose right half has the perpendicular normal (1, 0, 0),
    or lies 1 further along z: the right half restarts exactly, the left half
    accumulates; with both tests off everything accumulates."""
    c0, c1 = colours(2, seed=9)
    _, hist = step(spp=SPP, **ref.identity_inputs(W, H, SPP, c0))
    hist = hist.copy()
    right = np.zeros((H, W), bool)
    right[:, W // 2:] = True
    if kind == "normal":
        hist[2, right, :3] = F((1, 0, 0))
    else:
        hist[1, right, 2] += F(1)
    f = ref.identity_inputs(W, H, SPP, c1)
    c = f["cur"] / F(SPP)
    m0 = hist[0, ..., :3]
    blend = m0 + (c - m0) * (F(1) / F(2))
    _, h1 = step(spp=SPP, prev=ref.IDENTITY, history=hist, **f)
    assert np.array_equal(h1[0, ..., 3], np.where(right, F(1), F(2)))
    assert h1[0, ..., :3].tobytes() == np.where(right[..., None], c, blend).tobytes()
    _, h2 = step(spp=SPP, prev=ref.IDENTITY, history=hist, **OFF, **f)
    assert np.array_equal(h2[0, ..., 3], np.full((H, W), 2, F)) and h2[0, ..., :3].tobytes() == blend.tobytes()


@pytest.mark.parametrize("kind", ["normal", "depth"])
def test_ref_disocclusion(kind):
    check_disocclusion(ref.temporal_ref, kind)


def test_ref_sky():
    """4. A history sky tap is never gathered (whatever colour and length it
    holds, with both tests off too), and a current sky pixel restarts."""
    c0, c1 = colours(2, seed=11)
    _, hist = ref.temporal_ref(spp=SPP, **ref.identity_inputs(W, H, SPP, c0))
    hsky = np.zeros((H, W), bool)
    hsky[2:4, 3:9] = True
    hist[1, hsky, 3] = 1
    hist[0, hsky] = F((1e6, 1e6, 1e6, 1000))
    f = ref.identity_inputs(W, H, SPP, c1)
    csky = np.zeros((H, W), bool)
    csky[4:6, 1:5] = True
    for k in ("position", "normal"):
        f[k][csky] = 0
    f["hits"][csky] = 0
    c = f["cur"] / F(SPP)
    for opt in ({}, OFF):
        out, h1 = ref.temporal_ref(spp=SPP, prev=ref.IDENTITY, history=hist, **opt, **f)
        restart = hsky | csky
        assert np.array_equal(h1[0, ..., 3], np.where(restart, F(1), F(2)))
        assert h1[0, restart, :3].tobytes() == c[restart].tobytes()
        assert np.array_equal(h1[1, ..., 3], csky.astype(F))
        assert not h1[1, csky, :3].any() and not h1[2, csky].any()
        assert out.max() < 1e3
    # half a pixel next to a sky tap: the other tap alone, renormalised
    f = ref.identity_inputs(W, H, SPP, c1, (0.5, 0.0))
    _, h1 = ref.temporal_ref(spp=SPP, prev=ref.IDENTITY, history=hist, **OFF, **f)
    assert np.array_equal(h1[0, 2:4, 2, 3], np.full(2, 2, F)) and (h1[0, 2:4, 2, :3] < 10).all()
    assert np.array_equal(h1[0, 2:4, 3:8, 3], np.ones((2, 5), F))  # both taps sky


def test_ref_half_pixel():
    """5. P = (i + 0.5, j, 1): the history is the mean of the two horizontal
    neighbours' histories, against fp64 within 8 * 2^-24 relative (two
    products, two sums, a division, and the blend's three operations)."""
    c0, c1 = colours(2, seed=13)
    _, hist = ref.temporal_ref(spp=SPP, **ref.identity_inputs(W, H, SPP, c0))
    f = ref.identity_inputs(W, H, SPP, c1, (0.5, 0.0))
    _, h1 = ref.temporal_ref(spp=SPP, prev=ref.IDENTITY, history=hist, **f)
    m0 = hist[0, ..., :3].astype(np.float64)
    c = (f["cur"] / F(SPP)).astype(np.float64)
    hist64 = 0.5 * (m0[:, :-1] + m0[:, 1:])
    want = hist64 + (c[:, :-1] - hist64) * 0.5
    rel = np.abs(h1[0, :, :-1, :3] - want) / np.maximum(np.abs(hist64), np.abs(c[:, :-1]))
    print("half pixel: max relative deviation", rel.max(), "bound", 8 * 2.0 ** -24)
    assert rel.max() <= 8 * 2.0 ** -24
    assert np.array_equal(h1[0, :, :-1, 3], np.full((H, W - 1), 2, F))
    # column W-1 has its left tap only: that pixel's own history, renormalised
    own = hist[0, :, -1, :3]
    assert h1[0, :, -1, :3].tobytes() == (own + (f["cur"][:, -1] / F(SPP) - own) * F(0.5)).tobytes()


def test_synthetic_inputs_reach_every_branch():
    """The seeded frame, history and view of the GPU bit-equality test reach
    what the pass branches on (at 67x37, the frame the other sizes repeat)."""
    w, h = 67, 37
    frame, hist, view = ref.synthetic_inputs(w, h, SPP, seed=1000 * w + h)
    hits = frame["hits"]
    assert (hits == 0).any() and ((hits > 0) & (hits < SPP)).any() and (hits == SPP).any()
    assert ((hits > 0) & (frame["normal"] == 0).all(-1)).any()  # a zero normal sum on geometry
    seen = {}
    for name, opt in (("defaults", {}), ("long", dict(max_len=32)), ("tight", dict(plane_tol=1e-4)),
                      ("loose", dict(plane_tol=0.01)), ("off", OFF)):
        c = {}
        ref.temporal_ref(spp=SPP, prev=view, history=hist, census=c, **opt, **frame)
        seen[name] = c
    c = seen["defaults"]
    geo = hits > 0
    assert (geo & ~(c["w"] > 0)).any()  # behind the previous eye
    assert (geo & (c["w"] > 0) & ~c["ok"]).any()  # projected off the frame
    ok = c["ok"]
    assert (ok & (c["xi"] == -1)).any() and (ok & (c["xi"] == w - 1)).any()  # taps off the left / right border
    assert (ok & (c["yi"] == -1)).any() and (ok & (c["yi"] == h - 1)).any()  # top / bottom
    assert c["off_frame"] and c["sky_tap"] and c["plane"] and c["normal"]
    assert {1, 2, 3, 4} <= set(np.unique(c["taken"][c["valid"]]))
    assert (ok & ~c["valid"]).any()  # every tap rejected
    assert c["saturated"].any() and (seen["long"]["valid"] & ~seen["long"]["saturated"]).any()
    assert seen["long"]["saturated"].any()
    assert seen["tight"]["plane"] > c["plane"] > seen["loose"]["plane"] > 0 and seen["tight"]["valid"].any()
    assert seen["off"]["plane"] == 0 and seen["off"]["normal"] == 0 and seen["off"]["sky_tap"]
