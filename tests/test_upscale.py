"""Guided upsampling of a low-resolution frame (include/rt_upscale.h,
librtow_upscale.so), host side: the sixth library's exported surface, its
argument handling on paths that need no device, and properties of the numpy
restatement (tests/upscale_ref.py) that the GPU tests compare the kernels with
bit for bit -- so that it is more than a mirror of them.  The pass itself runs
in test_upscale_gpu.py, which runs the check_* functions below on the device
too."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import resolve_ref as rref
import upscale_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
F = np.float32
INF = float("inf")
OFF = dict(plane_tol=INF, normal_cos=-1.0)


def _nm(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


def test_upscale_library_exports_every_declared_symbol(rtow):
    """Every function include/rt_upscale.h declares is a defined text symbol of
    librtow_upscale.so, the header carries its own version, and the library
    needs librtow.so and no other pass library."""
    with open(os.path.join(ROOT, "include", "rt_upscale.h")) as f:
        text = f.read()
    names = sorted(set(re.findall(DECL, text, re.M)))
    assert names == ["rt_upscale", "rt_upscale_async", "rt_upscale_scratch_bytes", "rt_upscale_version"], names
    out = _nm(rtow.UPSCALE_LIB_PATH)
    for n in names:
        assert re.search(rf"\bT {n}$", out, re.M), n
    assert not re.search(r"\brt_(temporal|resolve|denoise|aov)", out)
    assert re.search(r"^#define RT_UPSCALE_VERSION 1$", text, re.M)
    assert rtow.upscale_lib().rt_upscale_version() == rtow.UPSCALE_VERSION == 1
    needed = subprocess.run(["readelf", "-d", rtow.UPSCALE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "librtow.so" in needed
    for other in ("librtow_aov", "librtow_denoise", "librtow_temporal", "librtow_resolve"):
        assert other not in needed, other


def test_upscale_lives_in_its_own_library_only(rtow):
    """The five other libraries export no rt_upscale* symbol, and their
    headers do not name one."""
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH, rtow.DENOISE_LIB_PATH, rtow.TEMPORAL_LIB_PATH,
                 rtow.RESOLVE_LIB_PATH):
        assert not re.search(r"\brt_upscale", _nm(path)), path
    for header in ("rt.h", "rt_internal.h", "rt_aov.h", "rt_denoise.h", "rt_temporal.h", "rt_resolve.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            assert "rt_upscale" not in f.read(), header
    assert rtow.lib().rt_abi_version() == 6 and rtow.aov_lib().rt_aov_version() == 1
    assert rtow.denoise_lib().rt_denoise_version() == 1 and rtow.temporal_lib().rt_temporal_version() == 1
    assert rtow.resolve_lib().rt_resolve_version() == 1


def test_upscale_mirror_has_the_headers_layout(rtow):
    """rtow.UpscaleDesc is rt_upscale_desc: ten 4-byte fields, the view (56
    bytes), the rays (48), then eleven pointers."""
    D = rtow.UpscaleDesc
    assert ctypes.sizeof(rtow.TemporalView) == 56 and ctypes.sizeof(rtow.ResolveRays) == 48
    assert ctypes.sizeof(D) == 144 + 11 * 8
    assert [f[0] for f in D._fields_] == ["lo_width", "lo_height", "lo_spp", "width", "height", "spp", "plane_tol",
                                          "normal_cos", "flags", "reserved", "lo_view", "rays", "cur", "hits_lo",
                                          "position_lo", "normal_lo", "albedo_lo", "hits_hi", "position_hi",
                                          "normal_hi", "albedo_hi", "out", "stage"]
    assert (D.lo_spp.offset, D.width.offset, D.spp.offset, D.plane_tol.offset, D.normal_cos.offset, D.flags.offset,
            D.reserved.offset, D.lo_view.offset, D.rays.offset, D.cur.offset, D.albedo_lo.offset, D.hits_hi.offset,
            D.out.offset, D.stage.offset) == (8, 12, 20, 24, 28, 32, 36, 40, 96, 144, 176, 184, 216, 224)
    with open(os.path.join(ROOT, "include", "rt_upscale.h")) as f:
        text = f.read()
    assert re.search(r"^#define RT_UPSCALE_NO_ALBEDO 1u", text, re.M)
    assert rtow.UPSCALE_NO_ALBEDO == ref.NO_ALBEDO == 1
    # the header's struct names the fields in the mirror's order
    body = text[text.index("typedef struct {"):text.index("} rt_upscale_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*?(\w+)\s*[,;]", body)
    assert fields == [f[0] for f in D._fields_], fields


def _valid_desc(rtow, keep, w=8, h=4, W=16, H=8, flags=0, **options):
    """A desc whose pointers are real host arrays (never dereferenced: the
    calls below are rejected first)."""
    d = rtow.upscale_desc(w, h, 4, W, H, 8, rref.IDENTITY_VIEW, rref.IDENTITY_RAYS, flags, **options)
    for name in rtow.UPSCALE_BUFFERS:
        a = np.zeros((H, W, 3), np.float32)
        keep.append(a)
        setattr(d, name, a.ctypes.data)
    return d


def test_upscale_null_range_overlap_and_eye_arguments_are_invalid(rtow):
    """Every rejection the header lists: RT_ERR_INVALID from both entry points
    before any HIP call and before the context is touched (no device here; the
    stand-in for a context is never read), with every buffer left as it was."""
    L = rtow.upscale_lib()
    keep = []
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    ms = ctypes.c_double(-1.0)
    scratch = np.zeros(48 * 8 * 4 + 16, np.uint8)
    keep.append(scratch)
    sp = (scratch.ctypes.data + 15) & ~15

    def rejected_async(d, c=ctx, s=sp):
        return L.rt_upscale_async(c, ctypes.byref(d) if d is not None else None, s, None) == rtow.RT_ERR_INVALID

    def rejected(d, c=ctx):
        p = ctypes.byref(d) if d is not None else None
        return (L.rt_upscale(c, p, ctypes.byref(ms)) == rtow.RT_ERR_INVALID and
                L.rt_upscale(c, p, None) == rtow.RT_ERR_INVALID and rejected_async(d, c))

    good = _valid_desc(rtow, keep)
    assert rejected(good, c=None) and rejected(None)
    required = [n for n in rtow.UPSCALE_BUFFERS if n != "stage"]
    for name in required:
        d = _valid_desc(rtow, keep)
        setattr(d, name, None)
        assert rejected(d), name
    for name in required:  # with NO_ALBEDO the others still may not (test_upscale_gpu.py runs it without albedos)
        if not name.startswith("albedo"):
            d = _valid_desc(rtow, keep, flags=rtow.UPSCALE_NO_ALBEDO)
            setattr(d, name, None)
            assert rejected(d), name
    nan = float("nan")
    for field, values in (("lo_width", (0, -1, 32769)), ("lo_height", (0, -3, 32769)), ("lo_spp", (0, -1)),
                          ("width", (0, -1, 32769)), ("height", (0, -3, 32769)), ("spp", (0, -1)),
                          ("plane_tol", (-0.1, nan, -INF)), ("normal_cos", (-1.5, 1.25, nan, INF, -INF)),
                          ("flags", (2, 3, 0x80000000)), ("reserved", (1, -1))):
        for v in values:
            d = _valid_desc(rtow, keep)
            setattr(d, field, v)
            assert rejected(d), (field, v)
    # a NULL or misaligned scratch: the device entry point
    d = _valid_desc(rtow, keep)
    assert rejected_async(d, s=None) and rejected_async(d, s=sp + 4) and rejected_async(d, s=sp + 8)
    # out, stage and scratch against each other and against everything the pass reads
    inputs = [n for n in rtow.UPSCALE_BUFFERS if n not in ("out", "stage")]
    for target in ("out", "stage"):
        for other in inputs + [n for n in ("out", "stage") if n != target]:
            for shift in (0, 16, -16):
                d = _valid_desc(rtow, keep)
                setattr(d, target, getattr(d, other) + shift)
                assert rejected(d), (target, other, shift)
    for other in rtow.UPSCALE_BUFFERS:
        for shift in (0, 16, -16):
            d = _valid_desc(rtow, keep)
            assert rejected_async(d, s=getattr(d, other) + shift), ("scratch", other, shift)
    # the two cameras must share the eye, bit for bit
    for k, v in ((0, 1e-30), (1, 1.0), (2, -0.0)):
        d = _valid_desc(rtow, keep)
        d.rays.eye[k] = v
        assert rejected(d), ("eye", k, v)
    d = _valid_desc(rtow, keep)
    d.lo_view.eye[1] = 2.0
    assert rejected(d)
    assert ms.value == -1.0  # a rejected call writes nothing
    assert all(not a.any() for a in keep)
    assert standin.raw == bytes(64)


def test_upscale_scratch_bytes(rtow):
    L = rtow.upscale_lib()
    assert L.rt_upscale_scratch_bytes(1, 1) == 48 and L.rt_upscale_scratch_bytes(33, 17) == 48 * 33 * 17
    assert L.rt_upscale_scratch_bytes(1920, 1080) == 48 * 1920 * 1080
    assert L.rt_upscale_scratch_bytes(32768, 32768) == 48 * 32768 * 32768
    for w, h in ((0, 4), (4, 0), (-1, 4), (32769, 4), (4, 32769)):
        assert L.rt_upscale_scratch_bytes(w, h) == 0, (w, h)
    assert rtow.upscale_scratch_bytes(5, 3) == 48 * 15


def test_upscale_python_options(rtow):
    """Unknown option or buffer names raise ValueError before any call; an
    option left out (or None) is the struct's 0 (= default), a given value
    means itself, an option of 0 raises; the view and the rays are required;
    flags go in as flags=."""
    class NoContext(rtow.Context):
        def __init__(self):  # no device: the name checks come before any call
            self._h = None

    ctx = NoContext()
    s = ref.synthetic_inputs(5, 3, 10, 6)
    V, R = s["lo_view"], s["rays"]
    args = (s["cur"], s["lo"], 4, s["hi"], 8)
    with pytest.raises(ValueError):
        ctx.upscale(*args, V, R, sharpness=0.2)
    with pytest.raises(ValueError):
        ctx.upscale(*args)  # no view, no rays
    with pytest.raises(ValueError):
        ctx.upscale(*args, V)
    with pytest.raises(ValueError):
        ctx.upscale(s["cur"], {"hits": s["lo"]["hits"]}, 4, s["hi"], 8, V, R)
    with pytest.raises(ValueError):
        ctx.upscale(s["cur"], s["lo"], 4, {k: v for k, v in s["hi"].items() if k != "albedo"}, 8, V, R)
    with pytest.raises(ValueError):
        ctx.upscale(s["cur"][:2], s["lo"], 4, s["hi"], 8, V, R)
    with pytest.raises(ValueError):
        ctx.upscale_async({"colour": 0}, 5, 3, 4, 10, 6, 8, V, R, 0)
    with pytest.raises(ValueError):
        ctx.upscale_async({"history_in": 0}, 5, 3, 4, 10, 6, 8, V, R, 0)  # rt_resolve's buffer, not this pass's
    with pytest.raises(ValueError):
        ctx.upscale_async({}, 5, 3, 4, 10, 6, 8, V, R, 0, gamma=1.0)
    for name in rtow.UPSCALE_DEFAULTS:
        with pytest.raises(ValueError):
            rtow.upscale_desc(5, 3, 4, 10, 6, 8, V, R, **{name: 0})
    d = rtow.upscale_desc(5, 3, 4, 10, 6, 8, V, R)
    assert (d.lo_width, d.lo_height, d.lo_spp, d.width, d.height, d.spp) == (5, 3, 4, 10, 6, 8)
    assert (d.plane_tol, d.normal_cos, d.flags, d.reserved) == (0.0, 0.0, 0, 0)
    assert list(d.rays.eye) == list(d.lo_view.eye) == [0.0, 0.0, ref.EYE_Z]
    assert list(d.rays.du) == [F(v) for v in R.du] and d.lo_view.x0 == F(ref.X0)
    d = rtow.upscale_desc(5, 3, 4, 10, 6, 8, V, R, rtow.UPSCALE_NO_ALBEDO, plane_tol=INF, normal_cos=-1)
    assert (d.plane_tol, d.normal_cos, d.flags) == (INF, -1.0, 1)
    d = rtow.upscale_desc(5, 3, 4, 10, 6, 8, V, R, flags=1, plane_tol=None, normal_cos=0.5)
    assert (d.plane_tol, d.normal_cos, d.flags) == (0.0, 0.5, 1)
    assert rtow.UPSCALE_DEFAULTS == ref.DEFAULTS
    assert rtow.UPSCALE_BUFFERS == ("cur", "hits_lo", "position_lo", "normal_lo", "albedo_lo", "hits_hi",
                                    "position_hi", "normal_hi", "albedo_hi", "out", "stage")


# ---- properties of the restatement (and, through test_upscale_gpu.py, of the device) ----
def ulps(a, b):
    """Distance in units of the last place between two float32 arrays of one sign."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _colour(h, w, seed):
    return (np.random.default_rng(seed).random((h, w, 3)) * 2 + 0.01).astype(F)


def check_identity(step):
    """Same size, the exact identity pair of rays and view (resolve_ref), equal
    guides, no demodulation, spp powers of two: every pixel maps to itself
    with weights 1, 0, 0, 0; out is cur bit for bit and stage is 1 everywhere."""
    w, h, spp = 13, 7, 4
    f = rref.identity_inputs(w, h, spp, _colour(h, w, 3))
    aov = dict(hits=f["hits"], normal=f["normal"], position=rref.identity_positions(w, h, spp))
    for opt in ({}, OFF):
        out, stage = step(f["cur"], aov, aov, spp, spp, rref.IDENTITY_VIEW, rref.IDENTITY_RAYS, flags=ref.NO_ALBEDO,
                          **opt)
        assert out.tobytes() == f["cur"].tobytes()
        assert (stage == 1).all()
    # a different spp of the output's guides changes nothing: out is in the low-resolution frame's sum contract
    f8 = rref.identity_inputs(w, h, 8, _colour(h, w, 3))
    aov8 = dict(hits=f8["hits"], normal=f8["normal"], position=rref.identity_positions(w, h, 8))
    out, stage = step(f["cur"], aov, aov8, spp, 8, rref.IDENTITY_VIEW, rref.IDENTITY_RAYS, flags=ref.NO_ALBEDO)
    assert out.tobytes() == f["cur"].tobytes() and (stage == 1).all()


def test_ref_identity():
    check_identity(ref.upscale_ref)


def check_demodulation(step):
    """A low-resolution irradiance u that is one constant (0.75; the albedo
    means are 1/4, 1/2 and 1, so cur = u m S and u itself are exact): out is
    (u m_hi) S to within 4 ulp whatever the bilinear weights (1 to 4 taps in
    the frame, fractional everywhere), with the tests off and every pixel a
    surface."""
    w, h, W, H, lo_spp, spp = 9, 5, 23, 11, 4, 8
    s = ref.synthetic_inputs(w, h, W, H, lo_spp, spp, seed=5)
    rng = np.random.default_rng(6)
    lo, hi = dict(s["lo"]), dict(s["hi"])
    lo["hits"], hi["hits"] = np.full((h, w), lo_spp, np.uint32), np.full((H, W), spp, np.uint32)
    m_lo = rng.choice([0.25, 0.5, 1.0], (h, w, 3)).astype(F)
    lo["albedo"] = m_lo * F(lo_spp)
    cur = (F(0.75) * m_lo) * F(lo_spp)
    out, stage = step(cur, lo, hi, lo_spp, spp, s["lo_view"], s["rays"], **OFF)
    m_hi = ref.prepare(hi["hits"], hi["position"], hi["normal"], hi["albedo"], spp, 0)[3]
    assert (m_hi == F(1e-3)).any() and (m_hi > F(0.05)).any()
    want = (F(0.75) * m_hi) * F(lo_spp)
    assert want.dtype == F and (stage == 1).all()
    worst = int(ulps(out, want).max())
    print(f"demodulation: worst distance {worst} ulp (bound 4)")
    assert worst <= 4


def test_ref_demodulation():
    check_demodulation(ref.upscale_ref)


def _edge_inputs():
    """Two exact planes under frame_pair's frames at 12x6 -> 31x15: A (z = 0,
    n = (0, 0, 1)) and B (z = -5, n = (0.6, 0, -0.8)): 5 apart in depth against
    a tolerance of 0.1 x 30, cos -0.8 apart in direction against -0.5.  The
    low-resolution frame is A left of its column 5 and B from there on; the
    output frame is A up to where it maps to column 9.5: its rightmost A
    pixels have nothing but B among their sixteen taps.  cur is 1 on A and 0
    on B."""
    w, h, W, H, lo_spp, spp = 12, 6, 31, 15, 4, 8
    view, rays, lo_xy, hi_xy = ref.frame_pair(w, h, W, H)

    def frame(xy, on_a, s):
        P = np.concatenate([xy, np.where(on_a, 0.0, -5.0)[..., None]], -1)
        n = np.where(on_a[..., None], np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, -0.8]))
        return dict(hits=np.full(on_a.shape, s, np.uint32), position=(P.astype(F) * F(s)).astype(F),
                    normal=(n.astype(F) * F(s)).astype(F))

    lo_a = np.mgrid[0:h, 0:w][1] < 5
    hi_a = hi_xy[..., 0] / ref.SX - ref.X0 < 9.5
    cur = np.where(lo_a[..., None], F(lo_spp), F(0)) * np.ones(3, F)
    return dict(cur=cur.astype(F), lo=frame(lo_xy, lo_a, lo_spp), hi=frame(hi_xy, hi_a, spp), lo_view=view, rays=rays,
                lo_spp=lo_spp, spp=spp), lo_a, hi_a


def check_edges(step):
    """An output pixel on A with at least one A tap among its sixteen comes out
    free of B, exactly (1 x S); one with none comes out as the plain bilinear
    value of its in-frame taps, and stage == 3.  Worked out here pixel by
    pixel, not with upscale_ref's code."""
    s, lo_a, hi_a = _edge_inputs()
    out, stage = step(s["cur"], s["lo"], s["hi"], s["lo_spp"], s["spp"], s["lo_view"], s["rays"], flags=ref.NO_ALBEDO)
    h, w = lo_a.shape
    H, W = hi_a.shape
    xi, yi, fx, fy, _, _ = ref.map_pixels(s["lo_view"], s["rays"], w, h, W, H)
    c = s["cur"] / F(s["lo_spp"])
    seen = {1: 0, 2: 0, 3: 0}
    for j in range(H):
        for i in range(W):
            if not hi_a[j, i]:
                continue
            near = [(xi[j, i] + dx, yi[j, i] + dy) for dy in (-1, 0, 1, 2) for dx in (-1, 0, 1, 2)]
            a_taps = [t for t in near if 0 <= t[0] < w and 0 <= t[1] < h and lo_a[t[1], t[0]]]
            if a_taps:
                assert stage[j, i] in (1, 2), (i, j)
                assert out[j, i].tobytes() == np.full(3, s["lo_spp"], F).tobytes(), (i, j, out[j, i])
            else:
                sw, sc = F(0), np.zeros(3, F)
                for dy in (0, 1):
                    for dx in (0, 1):
                        tx, ty = xi[j, i] + dx, yi[j, i] + dy
                        if tx < w and ty < h:
                            b = (fx[j, i] if dx else F(1) - fx[j, i]) * (fy[j, i] if dy else F(1) - fy[j, i])
                            sw, sc = sw + b, sc + b * c[ty, tx]
                assert stage[j, i] == 3, (i, j)
                assert out[j, i].tobytes() == ((sc / sw) * F(s["lo_spp"])).astype(F).tobytes(), (i, j)
            seen[int(stage[j, i])] += 1
    assert all(seen.values()), seen  # A pixels reach every stage
    # and the B side: an output pixel on B takes no A tap either
    b_near_b = ~hi_a & (stage < 3)
    assert b_near_b.any() and not out[b_near_b].any()


def test_ref_edges():
    check_edges(ref.upscale_ref)


SYNTH = (33, 17, 67, 37)


def synthetic(shape=SYNTH):
    w, h, W, H = shape
    return ref.synthetic_inputs(w, h, W, H, seed=1000 * w + W)


def check_sky(step):
    """On the synthetic frames with cur = 1 on the low-resolution sky and 0 on
    its surfaces: a sky pixel that stage 1 or 2 produced holds exactly 1 x S,
    so it took no surface tap; and a surface pixel from those stages holds
    exactly 0, so it took no sky tap."""
    s = synthetic()
    lo_sky = s["lo"]["hits"] == 0
    cur = (np.where(lo_sky[..., None], F(s["lo_spp"]), F(0)) * np.ones(3, F)).astype(F)
    out, stage = step(cur, s["lo"], s["hi"], s["lo_spp"], s["spp"], s["lo_view"], s["rays"], flags=ref.NO_ALBEDO)
    sky = s["hi"]["hits"] == 0
    guided = stage < 3
    assert (sky & (stage == 1)).any() and (sky & (stage == 2)).any() and (sky & (stage == 3)).any()
    assert (out[sky & guided] == F(s["lo_spp"])).all()
    assert (~sky & guided).any() and not out[~sky & guided].any()


def test_ref_sky():
    check_sky(ref.upscale_ref)


def test_upscale_synthetic_inputs_reach_every_branch():
    """The seeded frames of the GPU bit-equality test reach what the pass
    branches on (at 33x17 -> 67x37, the pair the other shapes repeat)."""
    s = synthetic()
    w, h, W, H = SYNTH
    args = (s["cur"], s["lo"], s["hi"], s["lo_spp"], s["spp"], s["lo_view"], s["rays"])
    seen = {}
    for name, opt in (("defaults", {}), ("off", OFF), ("tight", dict(plane_tol=1e-4)), ("facing", dict(normal_cos=0.99)),
                      ("no_albedo", dict(flags=ref.NO_ALBEDO))):
        c = {}
        out, stage = ref.upscale_ref(*args, census=c, **opt)
        assert np.isfinite(out).all(), name
        seen[name] = c
    c = seen["defaults"]
    assert {1, 2, 3} <= set(np.unique(c["stage"]))  # every stage
    for reason in ("left", "right", "top", "bottom", "sky_on_surface", "surface_on_sky", "plane", "normal"):
        assert c[reason] > 0, reason  # every reason for rejection
    first = c["stage"] == 1
    assert {1, 2, 3, 4} <= set(np.unique(c["taken1"][first]))  # one to four valid stage-1 taps
    assert c["zero_b_to_stage2"].any()  # a valid tap with b == 0 sends the pixel on
    assert (c["x"] < 0).any() and (c["x"] > w - 1).any() and (c["y"] < 0).any() and (c["y"] > h - 1).any()  # both clamps
    inner = (c["x"] > 0) & (c["x"] < w - 1) & (c["y"] > 0) & (c["y"] < h - 1)
    assert inner.any() and (c["fx"][inner] > 0).all()
    assert (c["m"] == F(1e-3)).any() and (c["m_lo"] == F(1e-3)).any()  # m at its floor in both frames
    assert (seen["no_albedo"]["m"] == 1).all()
    hits = s["hi"]["hits"]
    assert (hits == 0).any() and ((hits > 0) & (hits < s["spp"])).any() and (hits == s["spp"]).any()
    assert ((hits > 0) & (s["hi"]["normal"] == 0).all(-1)).any()  # a zero normal sum on geometry
    assert seen["tight"]["plane"] > c["plane"] > 0 and seen["facing"]["normal"] > c["normal"] > 0
    assert seen["off"]["plane"] == 0 and seen["off"]["normal"] == 0 and seen["off"]["sky_on_surface"] > 0
    assert (seen["off"]["stage"] == 1).sum() > first.sum()
