"""Closest hits within a per-ray distance limit (include/rt_segment.h,
librtow_segment.so), host side: the tenth library's exported surface, its
argument checks on paths that need no device, Context.visible's argument
handling, and the coverage conditions of tests/segment_cases.py's limit lists
on the CPU oracle's records.  The pass itself is checked on the GPU in
test_segment_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
import ray_fans as rf
import segment_cases as sg
import trace_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(DECL, f.read(), re.M)))


def _exports(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


# ---- surface ----------------------------------------------------------------
def test_segment_library_exports_every_declared_symbol(rtow):
    names = _declared("rt_segment.h")
    assert names == ["rt_segment", "rt_segment_async", "rt_segment_version"], names
    out = _exports(rtow.SEGMENT_LIB_PATH)
    for n in names:
        assert re.search(rf"\bT {n}$", out, re.M), n
    with open(os.path.join(ROOT, "include", "rt_segment.h")) as f:
        text = f.read()
    assert re.search(r"^#define RT_SEGMENT_VERSION 1$", text, re.M)
    assert re.search(r"^#define RT_SEGMENT_MISS \(-1\)", text, re.M)
    assert re.search(r"^#define RT_SEGMENT_INVALID \(-2\)", text, re.M)
    assert rtow.segment_lib().rt_segment_version() == rtow.SEGMENT_VERSION == 1
    assert (rtow.SEGMENT_MISS, rtow.SEGMENT_INVALID) == (rtow.TRACE_MISS, rtow.TRACE_INVALID) == (-1, -2)


def test_segment_leaves_the_render_abi_and_the_other_passes_alone(rtow):
    """A header and a library more: rt.h and rt_internal.h declare what they
    declared, no other library exports rt_segment*, and the new one exports
    nothing of another pass."""
    pub, internal = _declared("rt.h"), _declared("rt_internal.h")
    assert len(pub) == 21 and len(internal) == 10, (pub, internal)
    assert rtow.lib().rt_abi_version() == 6 == rtow.ABI_VERSION
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH, rtow.TRACE_LIB_PATH):
        assert not re.search(r"\brt_segment", _exports(path)), path
    assert not re.search(r"\brt_(aov|guides|route|denoise|temporal|resolve|upscale|trace)", _exports(rtow.SEGMENT_LIB_PATH))


def test_segment_structures_match_the_header(rtow):
    assert ctypes.sizeof(rtow.SegmentRays) == 32 and rtow.SegmentRays.t_max.offset == 24
    assert rtow.SegmentRays.origin.offset == 8 and rtow.SegmentRays.direction.offset == 16
    assert ctypes.sizeof(rtow.SegmentHits) == 40
    assert [f[0] for f in rtow.SegmentHits._fields_] == ["blocked", "id", "t", "position", "normal"] == list(sg.NAMES)
    assert [f[0] for f in rtow.SEGMENT_FIELDS] == list(sg.NAMES) and rtow.SEGMENT_FIELDS[0][1] == np.uint8
    assert rtow.SEGMENT_FIELDS[1:] == rtow.TRACE_FIELDS


# ---- rejections ---------------------------------------------------------------
def test_segment_rejections_come_before_any_hip_call(rtow):
    """A NULL context, rays or hits, a NULL origin or direction, n above
    2^31 - 1, and an output overlapping an input (t_max's 4n bytes included) or
    another output (blocked's n bytes included): RT_ERR_INVALID from both entry
    points before any HIP call and before the context is read (no device here;
    the stand-in for a context is never touched), the outputs and kernel_ms
    left as they were."""
    L = rtow.segment_lib()
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    n = 10
    o = np.zeros((n, 3), np.float32)
    d = np.ones((n, 3), np.float32)
    tm = np.full(n, 2, np.float32)
    out = {"blocked": np.full(n, 7, np.uint8), "id": np.full(n, 7, np.int32), "t": np.full(n, 7, np.float32),
           "position": np.full((n, 3), 7, np.float32), "normal": np.full((n, 3), 7, np.float32)}
    ms = ctypes.c_double(-1.0)

    def rays(n=n, origin=o.ctypes.data, direction=d.ctypes.data, t_max=tm.ctypes.data):
        return rtow.SegmentRays(n=n, origin=origin, direction=direction, t_max=t_max)

    def hits(**over):
        h = rtow.SegmentHits()
        for k, a in out.items():
            setattr(h, k, a.ctypes.data)
        for k, v in over.items():
            setattr(h, k, v)
        return h

    def both(c, r, h):
        rp = ctypes.byref(r) if r is not None else None
        hp = ctypes.byref(h) if h is not None else None
        return (L.rt_segment(c, rp, hp, 0, ctypes.byref(ms)), L.rt_segment(c, rp, hp, 0, None),
                L.rt_segment_async(c, rp, hp, 0, None))

    bad = (rtow.RT_ERR_INVALID,) * 3
    assert both(None, rays(), hits()) == bad
    assert both(ctx, None, hits()) == bad
    assert both(ctx, rays(), None) == bad
    assert both(ctx, rays(origin=None), hits()) == bad
    assert both(ctx, rays(direction=None), hits()) == bad
    assert both(ctx, rays(n=2 ** 31), hits()) == bad
    assert both(ctx, rays(n=2 ** 40, t_max=None), hits()) == bad
    # an output on an input, on its last byte, on t_max, and on another output
    assert both(ctx, rays(), hits(position=o.ctypes.data)) == bad
    assert both(ctx, rays(), hits(normal=d.ctypes.data)) == bad
    assert both(ctx, rays(), hits(id=o.ctypes.data + 12 * n - 1)) == bad
    assert both(ctx, rays(), hits(t=tm.ctypes.data)) == bad
    assert both(ctx, rays(), hits(blocked=tm.ctypes.data + 4 * n - 1)) == bad
    assert both(ctx, rays(), hits(id=tm.ctypes.data + 4 * n - 1)) == bad
    assert both(ctx, rays(), hits(blocked=d.ctypes.data + 5)) == bad
    assert both(ctx, rays(), hits(t=out["id"].ctypes.data)) == bad
    assert both(ctx, rays(), hits(id=out["blocked"].ctypes.data + n - 1)) == bad
    assert both(ctx, rays(), hits(blocked=out["normal"].ctypes.data + 12 * n - 1)) == bad
    assert both(ctx, rays(), hits(normal=out["position"].ctypes.data + 12 * n - 4)) == bad
    assert ms.value == -1.0
    assert standin.raw == b"\0" * 64
    for a in out.values():
        assert (a == 7).all()
    assert not o.any() and (d == 1).all() and (tm == 2).all()


def _recording_context(rtow):
    """A Context without a device whose segment() records visible()'s call
    and reports every second ray blocked."""
    class NoContext(rtow.Context):
        def __init__(self):
            self._h = None
            self.calls = []

        def segment(self, o, d, t_max=None, which=None, flags=0):
            self.calls.append((np.array(o), np.array(d), t_max, which, flags))
            return {"blocked": (np.arange(len(o)) % 2).astype(np.uint8), "kernel_ms": 0.0}
    return NoContext()


def test_segment_python_checks_names_and_shapes(rtow):
    class NoContext(rtow.Context):
        def __init__(self):
            self._h = None

    ctx = NoContext()
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        ctx.segment(o, o, which=("id", "albedo"))
    with pytest.raises(ValueError):
        ctx.segment(o, np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError):
        ctx.segment(np.zeros(12, np.float32), np.zeros(12, np.float32))
    with pytest.raises(ValueError):
        ctx.segment(o, o, t_max=np.ones(5, np.float32))
    with pytest.raises(ValueError):
        ctx.segment(o, o, t_max=np.ones((4, 1), np.float32))
    with pytest.raises(ValueError):
        ctx.segment_async({"origin": 0, "direction": 0, "depth": 0}, 4)
    with pytest.raises(ValueError):
        ctx.segment_async({"origin": 0, "t_max": 0, "blocked": 0}, 4)
    for n in (-1, rtow.TRACE_MAX_RAYS + 1):
        with pytest.raises(ValueError):
            ctx.segment_async({"origin": 0, "direction": 0, "blocked": 0}, n)


def test_visible_builds_the_segment_from_its_points(rtow):
    """visible(a, b, shrink) asks segment() for d = b - a in float32 with
    t_max = 1 - shrink and `blocked` alone, and returns ~blocked as bools; a
    single point pairs with every point of the other argument."""
    ctx = _recording_context(rtow)
    a = np.array([[0, 0, 0], [1, 2, 3], [4, 5, 6]], np.float64)
    b = np.array([[1, 1, 1], [3, 2, 1], [4, 5, 7]], np.float64)
    v = ctx.visible(a, b)
    assert v.dtype == bool and v.tolist() == [True, False, True]
    o, d, t_max, which, flags = ctx.calls[-1]
    assert o.dtype == d.dtype == np.float32 and o.tolist() == a.tolist() and d.tolist() == (b - a).tolist()
    assert np.float32(t_max) == np.float32(1.0) - np.float32(1e-3) and which == ("blocked",) and flags == 0
    ctx.visible(a, b, shrink=0.25, flags=rtow.RT_FLAG_ACCEL_BVH)
    assert np.float32(ctx.calls[-1][2]) == np.float32(0.75) and ctx.calls[-1][4] == rtow.RT_FLAG_ACCEL_BVH
    ctx.visible(a, b, shrink=0)
    assert np.float32(ctx.calls[-1][2]) == 1.0
    assert ctx.visible((0, 10, 0), b).shape == (3,) and ctx.calls[-1][0].tolist() == [[0, 10, 0]] * 3
    assert ctx.visible(a, (0, 10, 0)).shape == (3,) and ctx.calls[-1][1].tolist() == ([0, 10, 0] - a).tolist()
    assert ctx.visible((0, 0, 0), (0, 10, 0)).shape == (1,)
    n_calls = len(ctx.calls)
    for bad in ((a, b[:2]), (a[:, :2], b[:, :2]), (a.reshape(1, 3, 3), b), (np.zeros(4), b)):
        with pytest.raises(ValueError):
            ctx.visible(*bad)
    for shrink in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ctx.visible(a, b, shrink=shrink)
    assert len(ctx.calls) == n_calls


# ---- the lists ------------------------------------------------------------------
def test_limit_lists_have_the_shape_the_gpu_tests_rely_on(rtow):
    assert sg.FACTORS == (0.5, 0.75, 1.25, 2.0)
    for name in rf.SCENES:
        L, lim = tc.rays_of(name), sg.limits_of(name)
        assert sorted(map(str, lim)) == sorted(map(str, sg.FACTORS + ("mixed",)))
        n = L["n"]
        m = lim["mixed"]
        assert all(a.shape == (n,) and a.dtype == np.float32 for a in lim.values())
        # the special values, in four waves of the first block and in the second block
        at = [i for i, _ in sg.SPECIAL]
        assert len(set(i // tc.WAVE for i in at)) >= 5 and max(at) >= tc.BLOCK and not set(at) & set(tc.INVALID_AT)
        for i, v in sg.SPECIAL:
            assert m[i].tobytes() == np.float32(v).tobytes(), (name, i)
        vals = [v for _, v in sg.SPECIAL]
        assert np.inf in vals and 0.0 in vals and -1.0 in vals and 1e30 in vals and any(v != v for v in vals)
        # f cycles per ray in the mixed list: every factor list lends it rays
        plain = np.ones(n, bool)
        plain[at] = False
        plain &= L["valid"]
        for k, f in enumerate(sg.FACTORS):
            sel = plain & (np.arange(n) % len(sg.FACTORS) == k)
            assert sel.sum() >= 50 and m[sel].tobytes() == lim[f][sel].tobytes(), (name, f)


def test_limit_lists_meet_their_coverage_conditions_on_the_oracle(rtow):
    """Per scene, in the mixed list and under both interval flags: rays whose
    hit is kept, rays cut to a miss, rays never traced, all present; over the
    factor lists f >= 1.25 keeps every hit the oracle has and f <= 0.75 cuts
    every one -- but the near-zero hits of the cases' header, which are never
    traced at any factor: three of them, and they stay in the lists."""
    near = {name: sg.near_zero_hits(name) for name in rf.SCENES}
    print(near)
    assert sum(len(v) for v in near.values()) == 3
    assert all(tag == "surface-in" and abs(t) < 0.02 * tmin for v in near.values() for _, tag, t, tmin in v)
    for name in rf.SCENES:
        L = tc.rays_of(name)
        nz = [i for i, _, _, _ in near[name]]
        for interval in (0, 1):
            w = tc.want_of(name, interval)
            hit = L["valid"] & (w["id"] >= 0)
            cls = np.array(sg.classes_of(name, "mixed", interval))
            count = {c: int((cls == c).sum()) for c in ("kept", "cut", "never", "miss", "invalid")}
            print(name, interval, count)
            assert count["kept"] >= 30 and count["cut"] >= 30 and count["miss"] >= 10, (name, count)
            assert count["never"] >= 3 and count["invalid"] == len(tc.INVALID) + 2, (name, count)
            got = sg.want_of(name, "mixed", interval)
            assert (got["blocked"] == (cls == "kept")).all() and (got["id"][cls == "invalid"] == rtow.SEGMENT_INVALID).all()
            assert ((got["id"] >= 0) == (got["blocked"] == 1)).all() and np.isinf(got["t"][got["blocked"] == 0]).all()
            for f in sg.FACTORS:
                cf = np.array(sg.classes_of(name, f, interval))
                traced_hit = hit.copy()
                traced_hit[nz] = False
                # (a hit about t_min away is cut below t_min: never traced, a miss all the same)
                ok = (cf[traced_hit] == "kept") if f > 1 else np.isin(cf[traced_hit], ("cut", "never"))
                assert ok.all() and (f > 1 or (cf[traced_hit] == "cut").sum() >= 100), (name, f)
                assert (cf[nz] == "never").all() and (cf[L["valid"] & ~hit] == "miss").all(), (name, f)
                assert (cf[~L["valid"]] == "invalid").all()


def test_frozen_skip_rays_are_kept_and_cut(rtow):
    """The frozen spurious-root rays that go on to hit another sphere are in
    both classes: kept at f >= 1.25 (both walks' roots below what is left of
    the limit) and cut at f <= 0.75 (the second walk's root is not)."""
    kept = cut = 0
    for name in tc.FROZEN:
        L, w = tc.rays_of(name), tc.want_of(name)
        idx = [i for i, t in enumerate(L["tags"]) if t == "frozen-skip" and w["id"][i] >= 0]
        assert idx and ((w["events"][idx] & oracle_lib.EVENTS["skip_tmin"]) != 0).all()
        for key in sg.FACTORS + ("mixed",):
            cls = sg.classes_of(name, key)
            kept += sum(cls[i] == "kept" for i in idx)
            cut += sum(cls[i] == "cut" for i in idx)
        assert {sg.classes_of(name, 2.0)[i] for i in idx} == {"kept"} and {sg.classes_of(name, 0.5)[i] for i in idx} == {"cut"}
    assert kept >= 2 and cut >= 2


def test_normalised_length_is_the_length(rtow):
    """segment_cases' fp32 restatement of normalize3's l2 r, which the boundary
    test's limits divide by, against |d| in fp64."""
    for name in rf.SCENES:
        L = tc.rays_of(name)
        d = L["d"][L["valid"]]
        ln = sg.normalised_length(d)
        ref = np.sqrt((d.astype(np.float64) ** 2).sum(1))
        assert ln.dtype == np.float32 and (np.abs(ln / ref - 1.0) < 1e-6).all(), name
        below, at, above = sg.boundary_limits(name)
        sel = np.isfinite(at)
        assert sel.sum() >= 100 and (below[sel] < at[sel]).all() and (at[sel] < above[sel]).all()
