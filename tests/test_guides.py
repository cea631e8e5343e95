"""Feature buffers that follow mirror and glass paths (include/rt_guides.h,
librtow_guides.so), host side: the seventh library's exported surface and
dependencies, the struct mirrors, every rejection (before any HIP call, with
the context and the buffers untouched), the Python option rules and its gfx950
code's memory instructions.  The pass itself is checked on the GPU in
test_guides_gpu.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
OTHER_PASSES = ("aov", "denoise", "temporal", "resolve", "upscale")


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_guides_library_exports_every_declared_symbol(rtow):
    """Every function include/rt_guides.h declares is a defined text symbol of
    librtow_guides.so, no other pass's is, and the header carries its own
    version."""
    text = _header("rt_guides.h")
    names = sorted(set(re.findall(DECL, text, re.M)))
    assert names == ["rt_guides", "rt_guides_async", "rt_guides_version"], names
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.GUIDES_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}$", out, re.M), n
    assert not re.search(r"\brt_(%s)" % "|".join(OTHER_PASSES), out)
    assert re.search(r"^#define RT_GUIDES_VERSION 1$", text, re.M)
    assert rtow.guides_lib().rt_guides_version() == rtow.GUIDES_VERSION == 1


def test_guides_library_needs_librtow_and_no_pass_library(rtow):
    needed = subprocess.run(["readelf", "-d", rtow.GUIDES_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "librtow.so" in needed
    for other in OTHER_PASSES:
        assert "librtow_" + other not in needed, other


def test_guides_leaves_the_other_libraries_and_headers_alone(rtow):
    """The six other libraries export and need nothing of rt_guides, and their
    headers declare nothing of it (the three "Known limitation" paragraphs name
    it in comment text only); the render ABI is what it was."""
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH, rtow.DENOISE_LIB_PATH, rtow.TEMPORAL_LIB_PATH,
                 rtow.RESOLVE_LIB_PATH, rtow.UPSCALE_LIB_PATH):
        out = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        assert "rt_guides" not in out, path
        needed = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
        assert "librtow_guides" not in needed, path
    for h in ("rt.h", "rt_internal.h", "rt_aov.h", "rt_denoise.h", "rt_temporal.h", "rt_resolve.h", "rt_upscale.h",
              "rt_turn_table.h"):
        code = re.sub(r"/\*.*?\*/", "", _header(h), flags=re.S)  # comments removed
        assert "guides" not in code, h
    assert rtow.lib().rt_abi_version() == 6 == rtow.ABI_VERSION


def test_guides_mirrors_have_the_headers_layout(rtow):
    """rtow.GuidesOptions / GuidesBuffers are rt_guides_options / rt_guides_buffers:
    three 4-byte fields; rt_aov_buffers' six pointers in its order, then two."""
    O, B = rtow.GuidesOptions, rtow.GuidesBuffers
    assert ctypes.sizeof(O) == 12
    assert [(f[0], getattr(O, f[0]).offset) for f in O._fields_] == [("max_bounces", 0), ("max_fuzz", 4),
                                                                      ("reserved", 8)]
    assert ctypes.sizeof(B) == 64
    names = [f[0] for f in B._fields_]
    assert names == ["hits", "id", "depth", "position", "normal", "albedo", "bounces", "escaped"]
    assert [getattr(B, n).offset for n in names] == [8 * i for i in range(8)]
    assert names[:6] == [f[0] for f in rtow.AovBuffers._fields_]
    assert [(n, np.dtype(dt), ch) for n, dt, ch in rtow.GUIDES_FIELDS[6:]] == [("bounces", np.dtype(np.uint32), 1),
                                                                               ("escaped", np.dtype(np.uint32), 1)]
    # the header's field order
    text = _header("rt_guides.h")
    body = re.search(r"typedef struct \{[^}]*\} rt_guides_buffers;", text, re.S).group(0)
    assert re.findall(r"\*(\w+);", body) == names
    body = re.search(r"typedef struct \{[^}]*\} rt_guides_options;", text, re.S).group(0)
    assert re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M) == [("int32_t", "max_bounces"), ("float", "max_fuzz"),
                                                            ("uint32_t", "reserved")]


def test_guides_rejections_come_before_any_hip_call(rtow):
    """NULL context / camera / params / buffers, max_bounces < -1 or > 64, a NaN
    or negative max_fuzz, reserved != 0: RT_ERR_INVALID from both entry points
    before any HIP call and before the context is touched (no device here; the
    stand-in for a context is never read), with every buffer left as it was."""
    L = rtow.guides_lib()
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    cam = rtow.camera_cpu(aspect=2.0)
    prm = rtow.make_params(16, 8, 1)
    keep, bufs = [], rtow.GuidesBuffers()
    for name, dt, ch in rtow.GUIDES_FIELDS:
        a = np.zeros((8, 16) + ((3,) if ch == 3 else ()), dt)
        keep.append(a)
        setattr(bufs, name, a.ctypes.data)
    ms = ctypes.c_double(-1.0)
    c, p, b = ctypes.byref(cam), ctypes.byref(prm), ctypes.byref(bufs)

    def rejected(*args):
        return (L.rt_guides(*args, ctypes.byref(ms)) == rtow.RT_ERR_INVALID and
                L.rt_guides(*args, None) == rtow.RT_ERR_INVALID and
                L.rt_guides_async(*args, None) == rtow.RT_ERR_INVALID)

    ok = ctypes.byref(rtow.GuidesOptions())
    for args in ((None, c, p, ok, b), (ctx, None, p, ok, b), (ctx, c, None, ok, b), (ctx, c, p, ok, None),
                 (ctx, c, p, None, None), (None, None, None, None, None)):
        assert rejected(*args)
    bad = [rtow.GuidesOptions(max_bounces=-2), rtow.GuidesOptions(max_bounces=65),
           rtow.GuidesOptions(max_bounces=-2147483648), rtow.GuidesOptions(max_bounces=2147483647),
           rtow.GuidesOptions(max_fuzz=math.nan), rtow.GuidesOptions(max_fuzz=-1e-30),
           rtow.GuidesOptions(max_fuzz=-math.inf), rtow.GuidesOptions(reserved=1),
           rtow.GuidesOptions(max_bounces=3, max_fuzz=0.5, reserved=0x80000000)]
    for o in bad:
        assert rejected(ctx, c, p, ctypes.byref(o), b), (o.max_bounces, o.max_fuzz, o.reserved)
    assert ms.value == -1.0  # a rejected call writes nothing
    assert all(not a.any() for a in keep)
    assert standin.raw == bytes(64)


def test_guides_python_option_rules(rtow):
    """None is the default (the struct's 0), a value means itself: max_bounces
    = 0 is spelled -1 in the struct; out-of-range, fractional, NaN and negative
    values and unknown buffer names raise before any call."""
    o = rtow.guides_options()
    assert (o.max_bounces, o.max_fuzz, o.reserved) == (0, 0.0, 0)
    assert rtow.GUIDES_DEFAULTS == {"max_bounces": 8, "max_fuzz": 0.0} and rtow.GUIDES_MAX_BOUNCES == 64
    assert rtow.guides_options(max_bounces=0).max_bounces == -1
    assert rtow.guides_options(max_bounces=1).max_bounces == 1
    assert rtow.guides_options(max_bounces=64).max_bounces == 64
    assert rtow.guides_options(max_fuzz=0.25).max_fuzz == 0.25
    assert rtow.guides_options(max_fuzz=0.0).max_fuzz == 0.0
    assert math.isinf(rtow.guides_options(max_fuzz=math.inf).max_fuzz)
    for kw in (dict(max_bounces=-1), dict(max_bounces=65), dict(max_bounces=1.5), dict(max_bounces=True),
               dict(max_bounces=math.inf), dict(max_bounces=-math.inf), dict(max_bounces=math.nan),
               dict(max_fuzz=-0.1), dict(max_fuzz=math.nan)):
        with pytest.raises(ValueError):
            rtow.guides_options(**kw)

    class NoContext(rtow.Context):
        def __init__(self):  # no device: the checks come before any call
            self._h = None

    ctx = NoContext()
    cam, prm = rtow.camera_cpu(), rtow.make_params(16, 8, 1)
    with pytest.raises(ValueError):
        ctx.guides(cam, prm, which=("hits", "beauty"))
    with pytest.raises(ValueError):
        ctx.guides_async(cam, prm, {"colour": 0})
    with pytest.raises(ValueError):
        ctx.guides(cam, prm, max_bounces=65)
    with pytest.raises(ValueError):
        ctx.guides_async(cam, prm, {"hits": 0}, max_fuzz=-1.0)


def test_guides_device_code_has_no_flat_memory_instructions(rtow, tmp_path):
    """The procedure of test_aov.py's check on librtow_guides.so: its gfx950
    code reads the scene, the grid and its buffers through address_space(1) /
    (4) pointers and LDS through address_space(3): global_*, ds_* and scalar
    loads, no flat_* instruction; ten kernels (open x {scan, BVH, grid x 3
    placements})."""
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and shutil.which("objcopy")):
        pytest.skip("llvm-objdump / objcopy not available")
    fat = tmp_path / "fatbin.bin"
    co = tmp_path / "gfx950.co"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", rtow.GUIDES_LIB_PATH, str(fat)],
                   check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + str(fat),
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + str(co)], check=True)
    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)],
                         check=True, capture_output=True, text=True).stdout
    assert len(re.findall(r"^[0-9a-f]+ <_ZN3rtk13guides_kernel\w+>:$", dis, re.M)) == 10
    ops = re.findall(r"^\s+((?:flat|global|ds)_\w+)", dis, re.M)
    assert sum(o.startswith("global_") for o in ops) > 100 and sum(o.startswith("ds_") for o in ops) >= 8
    flat = sorted(set(o for o in ops if o.startswith("flat_")))
    assert not flat, flat
