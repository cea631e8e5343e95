"""Guide buffers of each pixel's dominant specular route (include/rt_route.h,
librtow_route.so), host side: the eighth library's exported surface and
dependencies, the struct mirrors, every rejection (before any HIP call, with
the context and the buffers untouched), the Python option rules, and the
properties of the numpy restatement (tests/route_ref.py) that the GPU tests
compare the pass with.  The pass itself is checked in test_route_gpu.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import route_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
OTHER_PASSES = ("aov", "denoise", "temporal", "resolve", "upscale", "guides")
OTHER_HEADERS = ("rt.h", "rt_internal.h", "rt_aov.h", "rt_denoise.h", "rt_temporal.h", "rt_resolve.h", "rt_upscale.h",
                 "rt_guides.h", "rt_turn_table.h")


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _other_libs(rtow):
    return (rtow.LIB_PATH, rtow.AOV_LIB_PATH, rtow.DENOISE_LIB_PATH, rtow.TEMPORAL_LIB_PATH, rtow.RESOLVE_LIB_PATH,
            rtow.UPSCALE_LIB_PATH, rtow.GUIDES_LIB_PATH)


# ---- surface and mirrors ---------------------------------------------------
def test_route_library_exports_exactly_the_headers_functions(rtow):
    text = _header("rt_route.h")
    names = sorted(set(re.findall(DECL, text, re.M)))
    assert names == ["rt_route", "rt_route_async", "rt_route_state_bytes", "rt_route_version"], names
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.ROUTE_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted(re.findall(r"\bT (rt_\w+)$", out, re.M))
    assert exported == names
    assert not re.search(r"\brt_(%s)" % "|".join(OTHER_PASSES), out)
    assert re.search(r"^#define RT_ROUTE_VERSION 1$", text, re.M)
    assert re.search(r"^#define RT_ROUTE_STATE_BYTES_PER_PIXEL 64$", text, re.M)
    assert rtow.route_lib().rt_route_version() == rtow.ROUTE_VERSION == 1
    assert '#include "rt_guides.h"' not in text


def test_route_library_needs_librtow_and_no_pass_library(rtow):
    needed = subprocess.run(["readelf", "-d", rtow.ROUTE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "librtow.so" in needed
    for other in OTHER_PASSES:
        assert "librtow_" + other not in needed, other


def test_route_leaves_the_other_libraries_and_headers_alone(rtow):
    """The seven other libraries export and need nothing of rt_route, and their
    headers do not name it; the render ABI is what it was."""
    for path in _other_libs(rtow):
        out = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        assert "rt_route" not in out, path
        needed = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
        assert "librtow_route" not in needed, path
    for h in OTHER_HEADERS:
        assert "rt_route" not in _header(h), h
    assert rtow.lib().rt_abi_version() == 6 == rtow.ABI_VERSION


def test_route_mirrors_have_the_headers_layout(rtow):
    O, B = rtow.RouteOptions, rtow.RouteBuffers
    assert ctypes.sizeof(O) == 12
    assert [(f[0], getattr(O, f[0]).offset) for f in O._fields_] == [("max_bounces", 0), ("max_fuzz", 4),
                                                                      ("reserved", 8)]
    assert ctypes.sizeof(B) == 72
    names = [f[0] for f in B._fields_]
    assert names == ["hits", "id", "depth", "position", "normal", "albedo", "route", "matched", "state"]
    assert [getattr(B, n).offset for n in names] == [8 * i for i in range(9)]
    assert names[:6] == [f[0] for f in rtow.AovBuffers._fields_]
    assert [(n, np.dtype(dt), ch) for n, dt, ch in rtow.ROUTE_FIELDS[6:]] == [("route", np.dtype(np.uint32), 1),
                                                                              ("matched", np.dtype(np.uint32), 1)]
    text = _header("rt_route.h")
    body = re.search(r"typedef struct \{[^}]*\} rt_route_buffers;", text, re.S).group(0)
    assert re.findall(r"\*(\w+);", body) == names
    body = re.search(r"typedef struct \{[^}]*\} rt_route_options;", text, re.S).group(0)
    assert re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M) == [("int32_t", "max_bounces"), ("float", "max_fuzz"),
                                                            ("uint32_t", "reserved")]


def test_route_state_bytes(rtow):
    f = rtow.route_lib().rt_route_state_bytes
    assert rtow.ROUTE_STATE_BYTES_PER_PIXEL == 64
    assert f(67, 37) == 64 * 67 * 37 and f(1, 1) == 64 and f(3840, 2160) == 64 * 3840 * 2160
    assert f(46341, 46341) == 64 * 46341 * 46341  # past 2^31 pixels, past 2^37 bytes: no 32-bit product
    assert f(0, 5) == 0 and f(5, 0) == 0 and f(-1, 5) == 0


# ---- rejections -------------------------------------------------------------
def test_route_rejections_come_before_any_hip_call(rtow):
    """rt_guides' rejections, a NULL or misaligned state, a state pointer in
    the buffers of the async call, and a state overlapping any output:
    RT_ERR_INVALID before any HIP call and before the context is touched (no
    device here; the stand-in for a context is never read), with every buffer,
    the state and kernel_ms left as they were."""
    L = rtow.route_lib()
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    cam = rtow.camera_cpu(aspect=2.0)
    w, h = 16, 8
    prm = rtow.make_params(w, h, 1)
    keep, bufs = [], rtow.RouteBuffers()
    for name, dt, ch in rtow.ROUTE_FIELDS:
        a = np.zeros((h, w) + ((3,) if ch == 3 else ()), dt)
        keep.append(a)
        setattr(bufs, name, a.ctypes.data)
    raw = np.zeros(64 * w * h + 32, np.uint8)  # host memory stands in for the device state: it is never reached
    base = (raw.ctypes.data + 15) // 16 * 16
    state = ctypes.c_void_p(base)
    ms = ctypes.c_double(-1.0)
    c, p, b = ctypes.byref(cam), ctypes.byref(prm), ctypes.byref(bufs)
    inv = rtow.RT_ERR_INVALID

    def rejected(*args):  # both entry points
        return (L.rt_route(*args, ctypes.byref(ms)) == inv and L.rt_route(*args, None) == inv and
                L.rt_route_async(*args, state, None) == inv)

    ok = ctypes.byref(rtow.RouteOptions())
    for args in ((None, c, p, ok, b), (ctx, None, p, ok, b), (ctx, c, None, ok, b), (ctx, c, p, ok, None),
                 (ctx, c, p, None, None), (None, None, None, None, None)):
        assert rejected(*args)
    bad = [rtow.RouteOptions(max_bounces=-2), rtow.RouteOptions(max_bounces=65),
           rtow.RouteOptions(max_bounces=-2147483648), rtow.RouteOptions(max_bounces=2147483647),
           rtow.RouteOptions(max_fuzz=math.nan), rtow.RouteOptions(max_fuzz=-1e-30),
           rtow.RouteOptions(max_fuzz=-math.inf), rtow.RouteOptions(reserved=1),
           rtow.RouteOptions(max_bounces=3, max_fuzz=0.5, reserved=0x80000000)]
    for o in bad:
        assert rejected(ctx, c, p, ctypes.byref(o), b), (o.max_bounces, o.max_fuzz, o.reserved)
    # the state of the async call: NULL, misaligned, named in the buffers too
    for st in (None, ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 8), ctypes.c_void_p(base + 1)):
        assert L.rt_route_async(ctx, c, p, ok, b, st, None) == inv
    with_state = rtow.RouteBuffers.from_buffer_copy(bufs)
    with_state.state = base
    assert L.rt_route_async(ctx, c, p, ok, ctypes.byref(with_state), state, None) == inv
    # a state that shares bytes with an output: its first byte, its last, and an output inside it
    nbytes = 64 * w * h
    for name, dt, ch in rtow.ROUTE_FIELDS:
        size = np.dtype(dt).itemsize * ch * w * h
        for at in (base, base + nbytes - 16, base - size + 16, base + (nbytes // 2) // 16 * 16):
            over = rtow.RouteBuffers.from_buffer_copy(bufs)
            setattr(over, name, at)
            assert L.rt_route_async(ctx, c, p, ok, ctypes.byref(over), state, None) == inv, (name, at - base)
            over.state = base  # the synchronous form's own state pointer, overlapping likewise
            assert L.rt_route(ctx, c, p, ok, ctypes.byref(over), None) == inv, (name, at - base)
    assert ms.value == -1.0  # a rejected call writes nothing
    assert all(not a.any() for a in keep) and not raw.any()
    assert standin.raw == bytes(64)


def test_route_python_option_rules(rtow):
    """rt_guides' rules: None is the default (the struct's 0), a value means
    itself, max_bounces = 0 is spelled -1; bad values and unknown buffer names
    raise before any call."""
    o = rtow.route_options()
    assert isinstance(o, rtow.RouteOptions) and (o.max_bounces, o.max_fuzz, o.reserved) == (0, 0.0, 0)
    assert rtow.route_options(max_bounces=0).max_bounces == -1
    assert rtow.route_options(max_bounces=1).max_bounces == 1
    assert rtow.route_options(max_bounces=64).max_bounces == 64
    assert rtow.route_options(max_fuzz=0.25).max_fuzz == 0.25
    assert math.isinf(rtow.route_options(max_fuzz=math.inf).max_fuzz)
    for kw in (dict(max_bounces=-1), dict(max_bounces=65), dict(max_bounces=1.5), dict(max_bounces=True),
               dict(max_bounces=math.inf), dict(max_bounces=math.nan), dict(max_fuzz=-0.1), dict(max_fuzz=math.nan)):
        with pytest.raises(ValueError):
            rtow.route_options(**kw)

    class NoContext(rtow.Context):
        def __init__(self):  # no device: the checks come before any call
            self._h = None

    ctx = NoContext()
    cam, prm = rtow.camera_cpu(), rtow.make_params(16, 8, 1)
    with pytest.raises(ValueError):
        ctx.route(cam, prm, which=("hits", "bounces"))
    with pytest.raises(ValueError):
        ctx.route_async(cam, prm, {"state": 0}, 0)
    with pytest.raises(ValueError):
        ctx.route(cam, prm, max_bounces=65)
    with pytest.raises(ValueError):
        ctx.route_async(cam, prm, {"hits": 0}, 0, max_fuzz=-1.0)


# ---- the restatement --------------------------------------------------------
def _majority_sequences(rng, count, length):
    """Random key sequences in which key 7 holds a strict majority of the hit
    samples, with misses sprinkled in; keys[S, count], hit[S, count]."""
    keys = rng.integers(1, 6, size=(length, count)).astype(np.uint32)
    hit = rng.random((length, count)) < 0.8
    for j in range(count):
        idx = np.flatnonzero(hit[:, j])
        if len(idx) == 0:
            hit[0, j], idx = True, np.array([0])
        major = rng.choice(idx, size=len(idx) // 2 + 1, replace=False)
        keys[major, j] = 7
    return keys, hit


def _scalar_vote(keys, hit):
    """The header's table, one pixel, plain Python."""
    key = votes = n = hits = 0
    adopted, floor = -1, 0
    for s, (k, h) in enumerate(zip(keys.tolist(), hit.tolist())):
        if not h:
            continue
        hits += 1
        if votes == 0:
            key, votes, n, adopted = k, 1, 1, s
        elif k == key:
            votes, n = votes + 1, n + 1
        else:
            votes -= 1
        floor = min(floor, votes)
    return key, votes, n, hits, adopted, floor


def test_select_returns_the_majority_key():
    rng = np.random.default_rng(15)
    for length in (1, 2, 5, 16, 33):
        keys, hit = _majority_sequences(rng, 200, length)
        r = route_ref.select(keys, hit)
        assert np.all(r["key"] == 7)
        assert np.array_equal(r["hits"], hit.sum(0).astype(np.uint32))
        for j in range(keys.shape[1]):
            key, votes, n, hits, adopted, floor = _scalar_vote(keys[:, j], hit[:, j])
            assert (r["key"][j], r["votes"][j], r["n"][j], r["hits"][j], r["adopted"][j]) == \
                (key, votes, n, hits, adopted)
            assert floor == 0  # the votes never underflow
            since = hit[adopted:, j] & (keys[adopted:, j] == 7)  # the key's count since its last adoption
            assert n == since.sum() and np.array_equal(np.flatnonzero(r["member"][:, j]) - adopted,
                                                       np.flatnonzero(since))
        assert np.all(r["votes"] >= 1) and np.all(r["n"] <= r["hits"]) and np.all(r["votes"] <= r["n"])


def test_select_without_a_majority_and_with_one_key():
    rng = np.random.default_rng(3)
    keys = rng.integers(1, 4, size=(16, 500)).astype(np.uint32)
    hit = rng.random((16, 500)) < 0.7
    r = route_ref.select(keys, hit)
    for j in range(500):
        assert (r["key"][j], r["votes"][j], r["n"][j], r["hits"][j], r["adopted"][j], 0) == \
            _scalar_vote(keys[:, j], hit[:, j])
    assert (r["changes"] > 0).any() and (r["votes"] == 0).any()
    one = route_ref.select(np.full((16, 500), 5, np.uint32), hit)  # a sequence of one key: n = hits
    assert np.array_equal(one["n"], one["hits"]) and np.array_equal(one["votes"], one["hits"])
    assert not one["changes"].any() and np.array_equal(one["member"], hit)
    assert np.all(one["key"][one["hits"] > 0] == 5) and np.all(one["key"][one["hits"] == 0] == 0)
    none = route_ref.select(keys, np.zeros_like(hit))  # no hit sample: the initial state
    assert not none["key"].any() and not none["hits"].any() and np.all(none["adopted"] == -1)
    k = route_ref.route_key(np.array([0, 0, 3, 64]), np.array([0, 1, 1, 0]))
    assert k.dtype == np.uint32 and k.tolist() == [1, 2, 8, 129]


def test_finalize_copies_scales_and_zeroes():
    rng = np.random.default_rng(8)
    m = 4000
    hits = rng.integers(1, 65, m).astype(np.uint32)
    n = np.minimum(hits, rng.integers(1, 65, m)).astype(np.uint32)
    n[:1000] = hits[:1000]
    hits[-500:] = n[-500:] = 0
    scale = np.exp(rng.uniform(-20, 20, (m, 1)))
    sums = {k: (rng.standard_normal((m, c)) * scale).astype(np.float32).squeeze() for k, c in
            (("depth", 1), ("position", 3), ("normal", 3), ("albedo", 3))}
    for a in sums.values():
        a[-500:] = 0.0
    sums["depth"][:3] = (-0.0, np.float32(1e-45), np.float32(3e38))  # copied whatever they are
    ident = rng.integers(-1, 400, m).astype(np.int32)
    key = np.where(hits > 0, rng.integers(1, 131, m), 0).astype(np.uint32)
    state = route_ref.make_state(key, np.ones(m, np.uint32), n, hits, sums["depth"], sums["position"], sums["normal"],
                                 sums["albedo"], ident)
    back = route_ref.split_state(state)
    assert np.array_equal(back["id"], ident) and back["depth"].tobytes() == sums["depth"].tobytes()
    out = route_ref.finalize(state)
    assert np.array_equal(out["hits"], hits) and np.array_equal(out["id"], ident)
    assert np.array_equal(out["matched"], n) and np.array_equal(out["route"], key - np.uint32(1))
    assert np.all(out["route"][hits == 0] == 0xFFFFFFFF)
    whole, part = n == hits, (n < hits)
    assert whole[:1000].all() and part.sum() > 500
    for name in route_ref.FEATURES:
        got, x = out[name], sums[name]
        assert got.dtype == np.float32
        assert got[whole].tobytes() == x[whole].tobytes(), name  # n == hits copies bits
        assert not got[hits == 0].any()
        shape = (-1,) + (1,) * (x.ndim - 1)
        want = x[part].astype(np.float64) / n[part].astype(np.float64).reshape(shape) * \
            hits[part].astype(np.float64).reshape(shape)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got[part].astype(np.float64) - want) <= 2.0 * ulp), name  # two roundings
