"""The guided a-trous denoiser (include/rt_denoise.h, librtow_denoise.so), host
side: the third library's exported surface, its argument handling on paths that
need no device, and properties of the numpy restatement (tests/denoise_ref.py)
that the GPU tests compare the kernels with bit for bit -- so that it is more
than a mirror of them.  The filter itself runs in test_denoise_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
EPS = 2.0 ** -24


def bound(iterations):
    """Relative rounding bound of `iterations` passes over a flat field: per
    pass 25 products and 25 adds on each of the two sums and one divide, each
    half an ulp at most (27 * 2^-24 with room), plus the four roundings of the
    demodulation and the remodulation."""
    return (27 * iterations + 4) * EPS


def flat_inputs(h, w, spp, normal=(0.0, 0.0, 1.0), albedo=(0.5, 0.25, 1.0), colour=(0.3, 0.7, 0.11)):
    """Every sample of every pixel hit a plane z = 0 with one normal and one
    albedo; the colour is the same everywhere.  n.D = 0 exactly on that plane."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    hits = np.full((h, w), spp, np.uint32)
    pos = np.stack([xx * 0.25, yy * 0.25, np.zeros_like(xx)], -1).astype(np.float32) * np.float32(spp)
    nrm = np.broadcast_to(np.float32(normal) * np.float32(spp), (h, w, 3)).copy()
    alb = np.broadcast_to(np.float32(albedo) * np.float32(spp), (h, w, 3)).copy()
    beauty = np.broadcast_to(np.float32(colour) * np.float32(spp), (h, w, 3)).copy()
    return dict(beauty=beauty, hits=hits, position=pos, normal=nrm, albedo=alb)


def edge_inputs(h, w, spp, kind):
    """Left half: plane z = 0, normal +z, u = 1 (beauty = albedo).  Right half,
    u = 0: kind "normal" -- the same plane's points with the perpendicular
    normal +x; kind "sky" -- no hits at all."""
    f = flat_inputs(h, w, spp, albedo=(0.5, 0.5, 0.5), colour=(0.5, 0.5, 0.5))
    right = np.zeros((h, w), bool)
    right[:, w // 2:] = True
    f["beauty"][right] = 0.0
    if kind == "normal":
        f["normal"][right] = np.float32((1.0, 0.0, 0.0)) * np.float32(spp)
    else:
        for k in ("position", "normal", "albedo"):
            f[k][right] = 0.0
        f["hits"][right] = 0
    return f, right


def test_denoise_library_exports_every_declared_symbol(rtow):
    """Every function include/rt_denoise.h declares is a defined text symbol
    of librtow_denoise.so, and the header carries its own version."""
    with open(os.path.join(ROOT, "include", "rt_denoise.h")) as f:
        text = f.read()
    names = sorted(set(re.findall(DECL, text, re.M)))
    assert names == ["rt_denoise", "rt_denoise_async", "rt_denoise_scratch_bytes", "rt_denoise_version"], names
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.DENOISE_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}$", out, re.M), n
    assert re.search(r"^#define RT_DENOISE_VERSION 1$", text, re.M)
    assert rtow.denoise_lib().rt_denoise_version() == rtow.DENOISE_VERSION == 1


def test_denoise_lives_in_its_own_library_only(rtow):
    """librtow.so and librtow_aov.so export no rt_denoise* symbol, and the
    other headers do not declare one."""
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert not re.search(r"\brt_denoise", out), path
    for header in ("rt.h", "rt_internal.h", "rt_aov.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            assert not [n for n in re.findall(DECL, f.read(), re.M) if "denoise" in n], header
    assert rtow.lib().rt_abi_version() == 6 and rtow.aov_lib().rt_aov_version() == 1


def test_denoise_desc_mirror_has_the_headers_layout(rtow):
    """rtow.DenoiseDesc is rt_denoise_desc: eight 4-byte fields, then six pointers."""
    D = rtow.DenoiseDesc
    assert ctypes.sizeof(D) == 32 + 6 * 8
    assert [f[0] for f in D._fields_] == ["width", "height", "spp", "iterations", "normal_power", "sigma_plane",
                                          "sigma_color", "reserved", "beauty", "hits", "position", "normal",
                                          "albedo", "out"]
    assert D.beauty.offset == 32 and D.out.offset == 72


def _valid_desc(rtow, keep, w=8, h=4, spp=4, **options):
    """A desc whose pointers are real host arrays (never dereferenced: the
    calls below are rejected first)."""
    d = rtow.denoise_desc(w, h, spp, **options)
    for name in rtow.DENOISE_INPUTS + ("out",):
        a = np.zeros((h, w, 3), np.float32)
        keep.append(a)
        setattr(d, name, a.ctypes.data)
    return d


def test_denoise_null_range_and_size_arguments_are_invalid(rtow):
    """NULL context / desc / scratch / buffer, a frame size, an spp or an
    option out of range: RT_ERR_INVALID from both entry points before any HIP
    call and before the context is touched (no device here; the stand-in for
    a context is never read)."""
    L = rtow.denoise_lib()
    keep = []
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    scratch = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    ms = ctypes.c_double(-1.0)

    def rejected(d, c=ctx, s=scratch):
        p = ctypes.byref(d) if d is not None else None
        return (L.rt_denoise(c, p, ctypes.byref(ms)) == rtow.RT_ERR_INVALID and
                L.rt_denoise(c, p, None) == rtow.RT_ERR_INVALID and
                L.rt_denoise_async(c, p, s, None) == rtow.RT_ERR_INVALID)

    good = _valid_desc(rtow, keep)
    assert rejected(good, c=None) and rejected(None)
    assert L.rt_denoise_async(ctx, ctypes.byref(good), None, None) == rtow.RT_ERR_INVALID
    assert L.rt_denoise_async(ctx, ctypes.byref(good), ctypes.c_void_p(scratch.value | 4), None) == \
        rtow.RT_ERR_INVALID  # scratch not 16-byte aligned
    for name in rtow.DENOISE_INPUTS + ("out",):
        d = _valid_desc(rtow, keep)
        setattr(d, name, None)
        assert rejected(d), name
    for field, values in (("width", (0, -1, 32769)), ("height", (0, -3, 32769)), ("spp", (0, -1)),
                          ("iterations", (-1, 9)), ("normal_power", (-2, 11)), ("reserved", (1,)),
                          ("sigma_plane", (-0.1, float("nan"))),
                          ("sigma_color", (-0.5, float("nan"), float("inf")))):
        for v in values:
            d = _valid_desc(rtow, keep)
            setattr(d, field, v)
            assert rejected(d), (field, v)
    assert ms.value == -1.0  # a rejected call writes nothing
    assert L.rt_denoise_scratch_bytes(67, 37) == 64 * 67 * 37
    assert L.rt_denoise_scratch_bytes(3840, 2160) == 64 * 3840 * 2160
    for w, h in ((0, 4), (4, 0), (-1, 4), (32769, 1), (1, 32769)):
        assert L.rt_denoise_scratch_bytes(w, h) == 0


def test_denoise_python_options(rtow):
    """Unknown option or buffer names raise ValueError before any call; an
    option left out is the struct's 0 (= default), a given value means itself
    (0 squarings, colour term off)."""
    class NoContext(rtow.Context):
        def __init__(self):  # no device: the name checks come before any call
            self._h = None

    ctx = NoContext()
    f = flat_inputs(4, 8, 4)
    with pytest.raises(ValueError):
        ctx.denoise(f["beauty"], f, 4, sigma=1.0)
    with pytest.raises(ValueError):
        ctx.denoise(f["beauty"], {"hits": f["hits"]}, 4)
    with pytest.raises(ValueError):
        ctx.denoise(f["beauty"][:2], f, 4)
    with pytest.raises(ValueError):
        ctx.denoise_async({"colour": 0}, 8, 4, 4, 0)
    with pytest.raises(ValueError):
        ctx.denoise_async({}, 8, 4, 4, 0, passes=3)
    with pytest.raises(ValueError):
        rtow.denoise_desc(8, 4, 4, iterations=0)
    d = rtow.denoise_desc(8, 4, 4)
    assert (d.iterations, d.normal_power, d.sigma_plane, d.sigma_color) == (0, 0, 0.0, 0.0)
    d = rtow.denoise_desc(8, 4, 4, iterations=3, normal_power=0, sigma_plane=float("inf"), sigma_color=0)
    assert (d.iterations, d.normal_power, d.sigma_plane, d.sigma_color) == (3, -1, float("inf"), -1.0)
    d = rtow.denoise_desc(8, 4, 4, normal_power=4, sigma_color=0.25, sigma_plane=None)
    assert (d.normal_power, d.sigma_plane, d.sigma_color) == (4, 0.0, 0.25)
    assert rtow.DENOISE_DEFAULTS == ref.DEFAULTS


# ---- properties of the restatement -------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_ref_flat_field_is_kept(iterations):
    """(a) equal guides, constant colour: the output is the input within the
    rounding bound."""
    f = flat_inputs(23, 31, 16)
    out = ref.denoise_ref(spp=16, iterations=iterations, **f)
    rel = np.abs(out.astype(np.float64) - f["beauty"]) / f["beauty"]
    print("flat field: max relative deviation", rel.max(), "bound", bound(iterations))
    assert rel.max() <= bound(iterations)


@pytest.mark.parametrize("kind", ["normal", "sky"])
@pytest.mark.parametrize("iterations", [1, 5])
def test_ref_edges_stop_the_filter(kind, iterations):
    """(b) perpendicular normals (or geometry against sky), u = 1 on the left
    and 0 on the right: nothing crosses -- the right is exactly 0, the left 1
    within the bound of (a)."""
    f, right = edge_inputs(22, 30, 16, kind)
    out = ref.denoise_ref(spp=16, iterations=iterations, **f)
    assert np.all(out[right] == 0.0)
    rel = np.abs(out[~right].astype(np.float64) - f["beauty"][~right]) / f["beauty"][~right]
    print("edge", kind, ": max relative deviation on the left", rel.max(), "bound", bound(iterations))
    assert rel.max() <= bound(iterations)


def spline_cascade64(u, iterations):
    """An independent fp64 statement of the plain filter: the separable
    B3-spline (1, 4, 6, 4, 1) / 16 with holes, rows then columns, the frame's
    border handled by renormalising with the same cascade step of ones."""
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0

    def blur(a, axis, step):
        out = np.zeros_like(a)
        n = a.shape[axis]
        idx = np.arange(n)
        for j, kj in enumerate(k):
            src = idx + (j - 2) * step
            ok = (src >= 0) & (src < n)
            take = np.take(a, np.clip(src, 0, n - 1), axis=axis)
            shape = [1] * a.ndim
            shape[axis] = n
            out += kj * take * ok.reshape(shape)
        return out

    u = u.astype(np.float64)
    for i in range(iterations):
        s = 1 << i
        ones = np.ones(u.shape[:2] + (1,))
        u = blur(blur(u, 1, s), 0, s) / blur(blur(ones, 1, s), 0, s)
    return u


@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_ref_plain_spline_and_variance(iterations):
    """(c) colour term off, no normal squaring, every point on one plane,
    random colour: the filter is the plain B3-spline cascade; and (d) it
    lowers the variance."""
    h, w, spp = 37, 45, 4
    f = flat_inputs(h, w, spp, albedo=(1.0, 1.0, 1.0))
    rng = np.random.default_rng(7)
    f["beauty"] = (rng.random((h, w, 3)).astype(np.float32) * np.float32(2.0)) * np.float32(spp)
    out = ref.denoise_ref(spp=spp, iterations=iterations, normal_power=0, sigma_color=0.0, **f)
    mean_in = f["beauty"].astype(np.float64) / spp
    want = spline_cascade64(mean_in, iterations)
    err = np.abs(out.astype(np.float64) / spp - want).max()
    span = mean_in.max() - mean_in.min()
    print("plain spline: max deviation", err, "bound", bound(iterations) * span)
    assert err <= bound(iterations) * span
    assert (out.astype(np.float64) / spp).var() < mean_in.var()
