"""Closest-hit queries for ray batches (include/rt_trace.h, librtow_trace.so),
host side: the ninth library's exported surface, its argument checks on paths
that need no device, its gfx950 code's memory instructions, and the coverage
conditions of tests/trace_cases.py's ray lists on the CPU oracle's records.
The pass itself is checked on the GPU in test_trace_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib
import ray_fans as rf
import trace_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
EV = oracle_lib.EVENTS


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(DECL, f.read(), re.M)))


# ---- surface ----------------------------------------------------------------
def test_trace_library_exports_every_declared_symbol(rtow):
    names = _declared("rt_trace.h")
    assert names == ["rt_trace", "rt_trace_async", "rt_trace_version"], names
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.TRACE_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}$", out, re.M), n
    with open(os.path.join(ROOT, "include", "rt_trace.h")) as f:
        text = f.read()
    assert re.search(r"^#define RT_TRACE_VERSION 1$", text, re.M)
    assert re.search(r"^#define RT_TRACE_INVALID \(-2\)", text, re.M)
    assert rtow.trace_lib().rt_trace_version() == rtow.TRACE_VERSION == 1
    assert (rtow.TRACE_MISS, rtow.TRACE_INVALID) == (-1, -2)


def test_trace_leaves_the_render_abi_and_the_other_passes_alone(rtow):
    """The feature adds a header and a library: rt.h and rt_internal.h declare
    what they declared, the ABI version is still 6, librtow.so and
    librtow_aov.so export no rt_trace*, and the new library exports nothing of
    another pass."""
    pub, internal = _declared("rt.h"), _declared("rt_internal.h")
    assert len(pub) == 21 and len(internal) == 10, (pub, internal)
    assert not [n for n in pub + internal if "trace" in n]
    assert rtow.lib().rt_abi_version() == 6 == rtow.ABI_VERSION
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert not re.search(r"\brt_trace", out), path
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.TRACE_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert not re.search(r"\brt_(aov|guides|route|denoise|temporal|resolve|upscale)", out)


def test_trace_structures_match_the_header(rtow):
    assert ctypes.sizeof(rtow.TraceRays) == 24 and rtow.TraceRays.origin.offset == 8
    assert ctypes.sizeof(rtow.TraceHits) == 32
    assert [f[0] for f in rtow.TraceHits._fields_] == ["id", "t", "position", "normal"]


# ---- rejections ---------------------------------------------------------------
def _arrays(n):
    o = np.zeros((n, 3), np.float32)
    d = np.ones((n, 3), np.float32)
    out = {"id": np.full(n, 7, np.int32), "t": np.full(n, 7, np.float32), "position": np.full((n, 3), 7, np.float32),
           "normal": np.full((n, 3), 7, np.float32)}
    return o, d, out


def test_trace_rejections_come_before_any_hip_call(rtow):
    """A NULL context, rays or hits, a NULL origin or direction, n above
    2^31 - 1 and an output overlapping an input or another output:
    RT_ERR_INVALID from both entry points before any HIP call and before the
    context is read (no device here; the stand-in for a context is never
    touched), with the outputs and kernel_ms left as they were."""
    L = rtow.trace_lib()
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    n = 10
    o, d, out = _arrays(n)
    ms = ctypes.c_double(-1.0)

    def rays(n=n, origin=o.ctypes.data, direction=d.ctypes.data):
        return rtow.TraceRays(n=n, origin=origin, direction=direction)

    def hits(**over):
        h = rtow.TraceHits()
        for k, a in out.items():
            setattr(h, k, a.ctypes.data)
        for k, v in over.items():
            setattr(h, k, v)
        return h

    def both(c, r, h):
        rp = ctypes.byref(r) if r is not None else None
        hp = ctypes.byref(h) if h is not None else None
        return (L.rt_trace(c, rp, hp, 0, ctypes.byref(ms)), L.rt_trace(c, rp, hp, 0, None),
                L.rt_trace_async(c, rp, hp, 0, None))

    bad = (rtow.RT_ERR_INVALID,) * 3
    assert both(None, rays(), hits()) == bad
    assert both(ctx, None, hits()) == bad
    assert both(ctx, rays(), None) == bad
    assert both(ctx, rays(origin=None), hits()) == bad
    assert both(ctx, rays(direction=None), hits()) == bad
    assert both(ctx, rays(n=2 ** 31), hits()) == bad  # (2^31 - 1 is the most: the kernel's ray index is 32 bits)
    assert both(ctx, rays(n=2 ** 40), hits()) == bad
    # overlaps: an output on an input, on its last byte, and on another output
    assert both(ctx, rays(), hits(position=o.ctypes.data)) == bad
    assert both(ctx, rays(), hits(normal=d.ctypes.data)) == bad
    assert both(ctx, rays(), hits(id=o.ctypes.data + 12 * n - 1)) == bad
    assert both(ctx, rays(), hits(t=d.ctypes.data + 4)) == bad
    assert both(ctx, rays(), hits(t=out["id"].ctypes.data)) == bad
    assert both(ctx, rays(), hits(normal=out["position"].ctypes.data + 12 * n - 4)) == bad
    assert both(ctx, rays(), hits(id=out["t"].ctypes.data + 4 * n - 1)) == bad
    assert ms.value == -1.0
    assert standin.raw == b"\0" * 64
    for a in out.values():
        assert (a == 7).all()
    assert not o.any() and (d == 1).all()


def test_trace_python_checks_names_and_shapes(rtow):
    class NoContext(rtow.Context):
        def __init__(self):  # no device: the checks come before any call
            self._h = None

    ctx = NoContext()
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        ctx.trace(o, o, which=("id", "albedo"))
    with pytest.raises(ValueError):
        ctx.trace(o, np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError):
        ctx.trace(np.zeros(12, np.float32), np.zeros(12, np.float32))
    with pytest.raises(ValueError):
        ctx.trace_async({"origin": 0, "direction": 0, "depth": 0}, 4)
    with pytest.raises(ValueError):
        ctx.trace_async({"origin": 0, "id": 0}, 4)
    for n in (-1, rtow.TRACE_MAX_RAYS + 1):
        with pytest.raises(ValueError):
            ctx.trace_async({"origin": 0, "direction": 0, "id": 0}, n)
    assert rtow.TRACE_MAX_RAYS == 2 ** 31 - 1


# ---- device code --------------------------------------------------------------
@pytest.mark.parametrize("lib_path, limit", [("TRACE_LIB_PATH", 0), ("SEGMENT_LIB_PATH", 1)], ids=["trace", "segment"])
def test_trace_device_code_has_ten_variants_and_no_flat_or_scratch_instructions(rtow, tmp_path, lib_path, limit):
    """test_aov.py's procedure on librtow_trace.so and librtow_segment.so: the
    ten variants (open x {scan, BVH, grid x 3 placements}) of
    csrc/rt_ray_batch.h's kernel, each library's without (LIMIT 0) or with
    (1) the limit and none of the other's; global_*, ds_* and scalar loads, no
    flat_* and no scratch_* / buffer_* (spill) instruction."""
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and shutil.which("objcopy")):
        pytest.skip("llvm-objdump / objcopy not available")
    fat = tmp_path / "fatbin.bin"
    co = tmp_path / "gfx950.co"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", getattr(rtow, lib_path), str(fat)],
                   check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + str(fat),
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + str(co)], check=True)
    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)],
                         check=True, capture_output=True, text=True).stdout
    kernels = re.findall(r"^[0-9a-f]+ <_ZN3rtk12batch_kernelILb([01])E\w+>:$", dis, re.M)
    assert kernels == [str(limit)] * 10, kernels
    ops = re.findall(r"^\s+((?:flat|global|ds|scratch|buffer)_\w+)", dis, re.M)
    assert sum(o.startswith("global_") for o in ops) > 100 and sum(o.startswith("ds_") for o in ops) >= 8
    other = sorted(set(o for o in ops if not o.startswith(("global_", "ds_"))))
    assert not other, other


# ---- the lists ------------------------------------------------------------------
def test_lists_have_the_shape_the_gpu_tests_rely_on(rtow):
    for name in rf.SCENES:
        L = tc.rays_of(name)
        n, o, valid, tags = L["n"], L["o"], L["valid"], L["tags"]
        assert 257 < n <= 400 and n % tc.WAVE != 0, (name, n)  # (more than one block of 256 lanes)
        oref2 = float(rf.oref2_of(name))
        o2 = (o.astype(np.float64) ** 2).sum(1)
        far = o2 > oref2
        # one far origin at index 17 of an otherwise near first wave; a whole far second wave
        assert far[tc.FAR_AT] and far[:tc.WAVE].sum() == 1 and valid[:tc.WAVE].all(), name
        assert far[tc.WAVE:2 * tc.WAVE].all() and valid[tc.WAVE:2 * tc.WAVE].all(), name
        assert far[2 * tc.WAVE:].any() and not far[2 * tc.WAVE:].all(), name  # (distant ground points among near rays)
        # the invalid forms, each where the list says
        assert sorted(np.nonzero(~valid)[0]) == list(tc.INVALID_AT), name
        d = L["d"]
        with np.errstate(over="ignore", invalid="ignore"):
            l2 = (d.astype(np.float32) ** 2).sum(1, dtype=np.float32)
        for i in tc.INVALID_AT:
            assert not np.isfinite(o[i]).all() or not np.isfinite(d[i]).all() or l2[i] == 0 or not np.isfinite(l2[i]), tags[i]
        assert np.isfinite(o[valid]).all() and np.isfinite(d[valid]).all()
        # direction lengths 1e-3, 1 and 1e3; both signs of zero
        ln = np.sqrt((d[valid].astype(np.float64) ** 2).sum(1))
        for want in tc.LENGTHS:
            assert (np.abs(ln / want - 1.0) < 0.05).sum() >= 20, (name, want)
        zero = d[valid] == 0
        assert (zero & np.signbit(d[valid])).any() and (zero & ~np.signbit(d[valid])).any(), name
        for tag in ("centre", "graze", "sky", "inside-glass", "surface-out", "surface-in", "ground-out", "ground-in"):
            assert tag in tags, (name, tag)
    assert "in-shell" in tc.rays_of("five")["tags"] and "in-hollow" in tc.rays_of("five")["tags"]


def test_lists_meet_their_coverage_conditions_on_the_oracle(rtow):
    """Summed over the four scenes, on the records the GPU test compares with."""
    tot = dict(layer=0, extras=0, miss=0, inside=0, neg=0, zero=0)
    for name in rf.SCENES:
        L, w, sc = tc.rays_of(name), tc.want_of(name), rf.scene_of(name)
        valid, ids = L["valid"], w["id"]
        assert (ids[~valid] == rtow.TRACE_INVALID).all() and np.isinf(w["t"][~valid]).all()
        hit = valid & (ids >= 0)
        assert (ids[valid] >= -1).all() and (ids[valid] < sc.n).all()
        # (a surface origin going in may hit its own sphere at a refined root a rounding below 0: the render's rule)
        assert np.isinf(w["t"][valid & ~hit]).all() and np.isfinite(w["t"][hit]).all() and (w["t"][hit] > -1e-6).all()
        if name in rf.LAYER_SCENES:
            lay = np.zeros(sc.n, bool)
            lay[rf.layer_spheres(sc)] = True
            tot["layer"] += int(lay[ids[hit]].sum())
            tot["extras"] += int((~lay[ids[hit]]).sum())
        tot["miss"] += int((valid & (ids == rtow.TRACE_MISS)).sum())
        tot["neg"] += int(((w["events"] & EV["neg_radius"]) != 0).sum())
        tot["zero"] += int((hit & (L["d"] == 0).any(1)).sum())
        C = np.stack([sc.cx, sc.cy, sc.cz], 1).astype(np.float64)
        dist = np.linalg.norm(L["o"][hit].astype(np.float64) - C[ids[hit]], axis=1)
        tot["inside"] += int((dist < np.abs(sc.radius[ids[hit]].astype(np.float64)) * (1.0 - 1e-4)).sum())
    print(tot)
    assert tot["layer"] >= 50 and tot["extras"] >= 20 and tot["miss"] >= 50, tot
    assert tot["inside"] >= 10 and tot["neg"] >= 1 and tot["zero"] >= 8, tot


def test_the_rays_cross_checked_with_rt_aov_are_of_their_kinds(rtow):
    picks = tc.aov_check_rays("final")
    assert len(set(i for i, _, _ in picks)) == len(tc.AOV_CHECK) >= 8
    assert sum(kind == "hit" for _, _, kind in picks) >= 5 and sum(kind == "miss" for _, _, kind in picks) >= 2


def test_frozen_rays_take_the_spurious_root_skip(rtow):
    """rt_aov.h notes that no case of the feature passes' tests takes a camera
    ray's spurious-root skip.  trace_cases.search_skips finds such rays (24 in
    1 310 720 candidates on the final scene, 13 on the five-sphere scene); six
    are frozen in the lists, and each still takes the skip: the oracle's record
    carries RTO_EV_SKIP_TMIN, with both interval flags."""
    assert tc.N_FROZEN >= 4
    n = 0
    for name in tc.FROZEN:
        L = tc.rays_of(name)
        idx = [i for i, t in enumerate(L["tags"]) if t == "frozen-skip"]
        assert len(idx) == len(tc.FROZEN[name])
        for interval in (0, 1):
            ev = tc.want_of(name, interval)["events"][idx]
            assert ((ev & EV["skip_tmin"]) != 0).all(), (name, interval)
        n += len(idx)
        # some go on to hit another sphere: t = the distance walked + the second walk's root
        assert (tc.want_of(name)["id"][idx] >= 0).any() and (tc.want_of(name)["id"][idx] == -1).any()
    assert n == tc.N_FROZEN


def test_the_search_still_finds_skips(rtow):
    """A short run of the search (one call's 32 768 candidates per sphere
    patch): it returns rays whose single-ray record carries the skip."""
    tried, found = tc.search_skips("final", 12, 7)
    assert tried == 12 * 32 * 16 * 64
    assert found
    for o, d, corner in found[:3]:
        rec = tc.judge(rf.scene_of("final"), rf.fan(o, corner, (0, 0, 0), (0, 0, 0)))
        assert rec["events"] & EV["skip_tmin"]
