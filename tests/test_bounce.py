"""The render's path step for ray batches (include/rt_bounce.h,
librtow_bounce.so), host side: the eleventh library's exported surface, its
ctypes layouts, every argument check that returns before a HIP call, its
gfx950 code's memory instructions, and the coverage conditions of
tests/bounce_cases.py's case lists on the CPU oracle's records.  The pass
itself is checked on the GPU in test_bounce_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bounce_cases as bc
import features_cases as fc
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
EV = oracle_lib.EVENTS
FUNCS = ["rt_bounce", "rt_bounce_async", "rt_bounce_camera_rays", "rt_bounce_camera_rays_async", "rt_bounce_version"]


def _header():
    with open(os.path.join(ROOT, "include", "rt_bounce.h")) as f:
        return f.read()


# ---- surface ----------------------------------------------------------------
def test_bounce_library_exports_every_declared_symbol(rtow):
    text = _header()
    assert sorted(set(re.findall(DECL, text, re.M))) == FUNCS
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.BOUNCE_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for n in FUNCS:
        assert re.search(rf"\bT {n}$", out, re.M), n
    assert not re.search(r"\brt_(aov|guides|route|denoise|temporal|resolve|upscale|trace|segment)", out)
    assert re.search(r"^#define RT_BOUNCE_VERSION 1$", text, re.M)
    for name, value in (("MISS", 0), ("SCATTERED", 1), ("ABSORBED", 2), ("INVALID", 3)):
        assert re.search(rf"^#define RT_BOUNCE_{name} {value}\b", text, re.M), name
        assert getattr(rtow, "BOUNCE_" + name) == value
    assert rtow.bounce_lib().rt_bounce_version() == rtow.BOUNCE_VERSION == 1
    # the header states the skip's form
    assert "NORMALISED AGAIN" in text and "rt_guides" in text and "INVALID" in text


def test_bounce_leaves_the_render_abi_and_the_other_passes_alone(rtow):
    assert rtow.lib().rt_abi_version() == 6 == rtow.ABI_VERSION
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH, rtow.TRACE_LIB_PATH, rtow.SEGMENT_LIB_PATH, rtow.GUIDES_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert not re.search(r"\brt_bounce", out), path


def test_bounce_structures_match_the_header(rtow):
    R, O = rtow.BounceRays, rtow.BounceOut
    assert ctypes.sizeof(R) == 48 and ctypes.sizeof(O) == 56
    assert [(f[0], getattr(R, f[0]).offset) for f in R._fields_] == [("n", 0), ("origin", 8), ("direction", 16),
                                                                     ("from_", 24), ("key", 32), ("seed", 40)]
    assert [f[0] for f in O._fields_] == ["status", "id", "t", "position", "normal", "scatter", "attenuation"]
    assert [f[0] for f in rtow.BOUNCE_FIELDS] == [f[0] for f in O._fields_]
    # the header's field order is the structures'
    body = re.search(r"typedef struct \{([^{}]*)\} rt_bounce_out;", _header(), re.S).group(1)
    names = re.findall(r"\*\s*(\w+)\s*[,;]", body)
    assert names == [f[0] for f in O._fields_], names


# ---- rejections ---------------------------------------------------------------
def test_bounce_rejections_come_before_any_hip_call(rtow):
    """A NULL context, rays or out, a NULL origin, direction or key, n above
    2^31 - 1 and an output overlapping any of the four inputs or another
    output: RT_ERR_INVALID from both entry points before any HIP call and
    before the context is read (no device here; the stand-in for a context is
    never touched), with the outputs and kernel_ms left as they were.  A NULL
    `from` is no error."""
    L = rtow.bounce_lib()
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    n = 10
    o, d = np.zeros((n, 3), np.float32), np.ones((n, 3), np.float32)
    frm, key = np.full(n, -1, np.int32), np.zeros((n, 3), np.uint32)
    out = {f: np.full((n, 3) if ch == 3 else (n,), 7, dt) for f, dt, ch in rtow.BOUNCE_FIELDS}
    ms = ctypes.c_double(-1.0)

    def rays(**over):
        a = dict(n=n, origin=o.ctypes.data, direction=d.ctypes.data, from_=frm.ctypes.data, key=key.ctypes.data, seed=5)
        a.update(over)
        return rtow.BounceRays(**a)

    def outs(**over):
        h = rtow.BounceOut()
        for k, a in out.items():
            setattr(h, k, a.ctypes.data)
        for k, v in over.items():
            setattr(h, k, v)
        return h

    def both(c, r, h):
        rp = ctypes.byref(r) if r is not None else None
        hp = ctypes.byref(h) if h is not None else None
        return (L.rt_bounce(c, rp, hp, 0, ctypes.byref(ms)), L.rt_bounce(c, rp, hp, 0, None),
                L.rt_bounce_async(c, rp, hp, 0, None))

    bad = (rtow.RT_ERR_INVALID,) * 3
    assert both(None, rays(), outs()) == bad
    assert both(ctx, None, outs()) == bad
    assert both(ctx, rays(), None) == bad
    assert both(ctx, rays(origin=None), outs()) == bad
    assert both(ctx, rays(direction=None), outs()) == bad
    assert both(ctx, rays(key=None), outs()) == bad
    assert both(ctx, rays(n=2 ** 31), outs()) == bad
    assert both(ctx, rays(n=2 ** 40), outs()) == bad
    # overlaps: an output on each input (its first and its last byte), and on another output
    assert both(ctx, rays(), outs(position=o.ctypes.data)) == bad
    assert both(ctx, rays(), outs(scatter=d.ctypes.data)) == bad
    assert both(ctx, rays(), outs(id=frm.ctypes.data)) == bad
    assert both(ctx, rays(), outs(status=frm.ctypes.data + 4 * n - 1)) == bad
    assert both(ctx, rays(), outs(attenuation=key.ctypes.data + 12 * n - 4)) == bad
    assert both(ctx, rays(), outs(t=key.ctypes.data)) == bad
    assert both(ctx, rays(), outs(status=o.ctypes.data + 12 * n - 1)) == bad
    assert both(ctx, rays(), outs(t=out["id"].ctypes.data)) == bad
    assert both(ctx, rays(), outs(scatter=out["normal"].ctypes.data + 12 * n - 4)) == bad
    assert both(ctx, rays(), outs(attenuation=out["scatter"].ctypes.data + 4)) == bad
    assert both(ctx, rays(), outs(id=out["status"].ctypes.data + n - 1)) == bad
    assert ms.value == -1.0
    assert standin.raw == b"\0" * 64
    for a in out.values():
        assert (a == 7).all()
    assert not o.any() and (d == 1).all() and (frm == -1).all() and not key.any()


def test_camera_rays_rejections_come_before_any_hip_call(rtow):
    """NULL arguments, params and cameras a render rejects, a negative sample0
    or count, sample0 + samples above 2^24 and more than 2^31 - 1 rays."""
    L = rtow.bounce_lib()
    cam = rtow.camera_cpu(aspect=2.0)
    buf = np.zeros((64, 3), np.float32)
    key = np.zeros((64, 3), np.uint32)
    ms = ctypes.c_double(-1.0)

    def both(c, cm, p, s0, cnt, o=buf.ctypes.data, d=buf.ctypes.data, k=key.ctypes.data):
        cp = ctypes.byref(cm) if cm is not None else None
        pp = ctypes.byref(p) if p is not None else None
        return (L.rt_bounce_camera_rays(c, cp, pp, s0, cnt, o, d, k, ctypes.byref(ms)),
                L.rt_bounce_camera_rays_async(c, cp, pp, s0, cnt, o, d, k, None))

    bad = (rtow.RT_ERR_INVALID,) * 2
    p = rtow.make_params(4, 2, 1)
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    assert both(None, cam, p, 0, 1) == bad
    assert both(ctx, None, p, 0, 1) == bad
    assert both(ctx, cam, None, 0, 1) == bad
    assert both(ctx, cam, p, -1, 1) == bad
    assert both(ctx, cam, p, 0, -1) == bad
    assert both(ctx, cam, p, 2 ** 24, 1) == bad
    assert both(ctx, cam, p, 1, 2 ** 24) == bad
    assert both(ctx, cam, rtow.make_params(0, 2, 1), 0, 1) == bad         # params_ok's width
    assert both(ctx, cam, rtow.make_params(4, 2, 1, max_depth=-1), 0, 1) == bad
    assert both(ctx, cam, rtow.make_params(1, 1, 1), 0, 1) == bad         # the lens model needs two pixels each way
    big = rtow.make_params(32768, 32768, 1)
    assert both(ctx, cam, big, 0, 2) == bad                               # 2^31 rays
    assert ms.value == -1.0 and standin.raw == b"\0" * 64 and not buf.any()


def test_bounce_python_checks_names_and_shapes(rtow):
    class NoContext(rtow.Context):
        def __init__(self):  # no device: the checks come before any call
            self._h = None

    ctx = NoContext()
    o = np.zeros((4, 3), np.float32)
    k = np.zeros((4, 3), np.uint32)
    with pytest.raises(ValueError):
        ctx.bounce(o, o, k, 0, which=("id", "albedo"))
    with pytest.raises(ValueError):
        ctx.bounce(o, np.zeros((5, 3), np.float32), k, 0)
    with pytest.raises(ValueError):
        ctx.bounce(o, o, np.zeros((4, 2), np.uint32), 0)
    with pytest.raises(ValueError):
        ctx.bounce(o, o, k, 0, from_=np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        ctx.bounce_async({"origin": 0, "direction": 0, "key": 0, "depth": 0}, 4, 0)
    with pytest.raises(ValueError):
        ctx.bounce_async({"origin": 0, "direction": 0, "id": 0}, 4, 0)
    for n in (-1, rtow.TRACE_MAX_RAYS + 1):
        with pytest.raises(ValueError):
            ctx.bounce_async({"origin": 0, "direction": 0, "key": 0, "id": 0}, n, 0)


def test_path_trace_is_short_and_refuses_what_it_does_not_restate(rtow):
    import inspect
    src = inspect.getsource(rtow.path_trace)
    assert len(src.splitlines()) < 40

    class Ctx:
        scene = fc.clamp_scene(rtow)
    with pytest.raises(ValueError):
        rtow.path_trace(Ctx, rtow.camera_cpu(aspect=2.0), rtow.make_params(4, 2, 1))  # wide sums
    Ctx.scene = rtow.five_scene()
    with pytest.raises(ValueError):
        rtow.path_trace(Ctx, rtow.camera_cpu(aspect=2.0), rtow.make_params(4, 2, 4096))  # dithered sums


# ---- device code --------------------------------------------------------------
def test_bounce_device_code_has_ten_variants_and_no_flat_or_scratch_instructions(rtow, tmp_path):
    """test_trace.py's procedure on librtow_bounce.so: the ten variants of
    bounce_kernel and camera_rays_kernel; global_*, ds_* and scalar loads, no
    flat_* and no scratch_* / buffer_* (spill) instruction, and a private
    segment of 0 bytes in every kernel."""
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and shutil.which("objcopy")):
        pytest.skip("llvm-objdump / objcopy not available")
    fat = tmp_path / "fatbin.bin"
    co = tmp_path / "gfx950.co"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", rtow.BOUNCE_LIB_PATH, str(fat)], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + str(fat),
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + str(co)], check=True)
    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)],
                         check=True, capture_output=True, text=True).stdout
    assert len(re.findall(r"^[0-9a-f]+ <_ZN3rtk13bounce_kernelI\w+>:$", dis, re.M)) == 10
    assert len(re.findall(r"^[0-9a-f]+ <_ZN3rtk18camera_rays_kernel\w+>:$", dis, re.M)) == 1
    ops = re.findall(r"^\s+((?:flat|global|ds|scratch|buffer)_\w+)", dis, re.M)
    assert sum(o.startswith("global_") for o in ops) > 100 and sum(o.startswith("ds_") for o in ops) >= 8
    other = sorted(set(o for o in ops if not o.startswith(("global_", "ds_"))))
    assert not other, other
    readelf = os.path.join(llvm, "llvm-readelf")
    if os.path.exists(readelf):
        notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)
        assert len(sizes) == 11 and set(sizes) == {"0"}, sizes


# ---- the lists ------------------------------------------------------------------
def test_the_case_lists_are_the_ones_the_gpu_tests_rely_on(rtow):
    assert set(bc.CHAIN_CASES) == set(fc.CASES) and "clamp" in bc.CHAIN_CASES and "glassground" in bc.CHAIN_CASES
    # the render judge leaves out exactly the cases whose pixel sums are wide (an opaque albedo above 1)
    wide = {c for c in fc.CASES if float(fc.scene_of(rtow, c).albedo[fc.scene_of(rtow, c).kind != 2].max()) > 1.0}
    assert wide == set(bc.WIDE_CASES) and set(bc.RENDER_CASES) == set(fc.CASES) - wide and len(bc.RENDER_CASES) == 20
    assert bc.DEPTHS == (50, 3) and bc.CHAIN_BOUNCES == (-1, 1, 2, 8)
    # each interval form and each metal form is present
    flags = {fc.CASES[c]["flags"] for c in bc.RENDER_CASES}
    assert any(f & 1 for f in flags) and any(not f & 1 for f in flags)
    assert any(f & 2 for f in flags) and any(not f & 2 for f in flags)
    # walks: layer scenes (the grid's three placements) and plain ones
    layer = [c for c in bc.RENDER_CASES if bc.is_layer_scene(rtow, c)]
    assert layer and len(layer) < len(bc.RENDER_CASES)
    for c in layer[:1]:
        for _, _, mode in bc.LAYER_WALKS:
            if mode:
                assert rtow.accel_info(fc.scene_of(rtow, c), mode)["grid_placement"] == rtow.GRID_PLACEMENTS[mode]
    # lens, pinhole, banded
    models = {fc.CASES[c]["model"] for c in bc.CAMERA_CASES}
    assert models == {"cpu_lens", "gpu_pinhole"} and any("bands" in fc.CASES[c] for c in bc.CAMERA_CASES)
    # path_trace's limits hold for every render case
    for c in bc.RENDER_CASES:
        sc = fc.scene_of(rtow, c)
        assert fc.CASES[c]["spp"] < 4096 and float(sc.albedo[sc.kind != 2].max()) <= 1.0, c


def test_the_cases_meet_their_coverage_conditions_on_the_oracle(rtow):
    """Over the cases, the oracle's chain records (8 bounces, every fuzz
    followed) show every event the material blocks and the skip rule have, and
    the render restatement enters a sealed sphere at least once (contact)."""
    seen = 0
    count = {k: 0 for k in EV}
    for case in bc.CHAIN_CASES:
        frame = fc.frames_of(case)[0]
        if fc.CASES[case]["spp"] == 0:
            continue
        t = fc.terminals(rtow, case, frame, 8, 1.0)
        ev = t["events"]
        seen |= int(np.bitwise_or.reduce(ev.ravel()))
        for k, bit in EV.items():
            count[k] += int(((ev & bit) != 0).sum())
    print(count)
    for k in ("refract", "schlick", "tir", "absorbed", "fuzzy", "skip_tmin", "skip_exit", "neg_radius"):
        assert seen & EV[k], k
    # the 2^100 clamp changes a value only in a chain of 64 bounces between clamp's mirrors
    frame = fc.frames_of("clamp")[0]
    assert not (fc.terminals(rtow, "clamp", frame, 8, 0.0)["events"] & EV["clamp"]).any()
    assert (fc.terminals(rtow, "clamp", frame, bc.CLAMP_BOUNCES, 0.0)["events"] & EV["clamp"]).any()
    # the opaque-inside rule: paths whose first hit inside a sealed lambertian ball ends them
    L = oracle_lib.lib()
    L.rto_kernel_attrib.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    L.rto_kernel_attrib.restype = None
    a = (ctypes.c_ulonglong * 3)()
    L.rto_kernel_attrib(a, 1)
    case = "contact"
    frame = fc.frames_of(case)[0]
    assert oracle_lib.sealed(fc.scene_of(rtow, case)).any()
    oracle_lib.kernel_render(fc.scene_of(rtow, case), fc.camera_of(rtow, case, frame), bc.params_of(rtow, case, frame))
    L.rto_kernel_attrib(a, 1)
    print("attrib (skips, sealed entries, after a skip):", list(a))
    assert a[1] >= 1
