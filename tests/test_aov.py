"""First-hit feature buffers (include/rt_aov.h, librtow_aov.so), host side: the
second library's exported surface, its argument handling on paths that need
no device, and its gfx950 code's memory instructions.  The pass itself is
checked on the GPU in test_aov_gpu.py."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(DECL, f.read(), re.M)))


def test_aov_library_exports_every_declared_symbol(rtow):
    """Every function include/rt_aov.h declares is a defined text symbol of
    librtow_aov.so, and the header carries its own version."""
    names = _declared("rt_aov.h")
    assert names == ["rt_aov", "rt_aov_async", "rt_aov_version"], names
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.AOV_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}$", out, re.M), n
    with open(os.path.join(ROOT, "include", "rt_aov.h")) as f:
        assert re.search(r"^#define RT_AOV_VERSION 1$", f.read(), re.M)
    assert rtow.aov_lib().rt_aov_version() == rtow.AOV_VERSION == 1


def test_aov_leaves_the_render_abi_alone(rtow):
    """The feature adds a header and a library: rt.h and rt_internal.h declare
    what they declare without it (21 and 10 functions), none of them the new entry
    points, and the ABI version is still 6."""
    pub, internal = _declared("rt.h"), _declared("rt_internal.h")
    assert len(pub) == 21 and len(internal) == 10, (pub, internal)
    assert not [n for n in pub + internal if "aov" in n or "frame" in n]
    assert rtow.lib().rt_abi_version() == 6 == rtow.ABI_VERSION
    # librtow.so exports no rt_aov*: the pass lives in the second library only
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert not re.search(r"\brt_aov", out)


def test_aov_null_arguments_are_invalid(rtow):
    """NULL context / camera / params / buffers: RT_ERR_INVALID from both entry
    points, before any HIP call (this runs without a device) -- also for a
    buffer struct with every pointer NULL when there is no context."""
    L = rtow.aov_lib()
    cam = rtow.camera_cpu(aspect=2.0)
    prm = rtow.make_params(16, 8, 1)
    bufs = rtow.AovBuffers()
    assert all(getattr(bufs, name) is None for name, _, _ in rtow.AOV_FIELDS)
    c, p, b = ctypes.byref(cam), ctypes.byref(prm), ctypes.byref(bufs)
    fake = ctypes.c_void_p(0)
    ms = ctypes.c_double(-1.0)
    for args in ((fake, c, p, b), (fake, None, p, b), (fake, c, None, b), (fake, c, p, None),
                 (fake, None, None, None)):
        assert L.rt_aov(*args, ctypes.byref(ms)) == rtow.RT_ERR_INVALID
        assert L.rt_aov(*args, None) == rtow.RT_ERR_INVALID
        assert L.rt_aov_async(*args, None) == rtow.RT_ERR_INVALID
    assert ms.value == -1.0  # a rejected call writes nothing


def test_aov_python_rejects_unknown_buffer_names(rtow):
    class NoContext(rtow.Context):
        def __init__(self):  # no device: the name check comes before any call
            self._h = None

    ctx = NoContext()
    with pytest.raises(ValueError):
        ctx.aov(rtow.camera_cpu(), rtow.make_params(16, 8, 1), which=("hits", "beauty"))
    with pytest.raises(ValueError):
        ctx.aov_async(rtow.camera_cpu(), rtow.make_params(16, 8, 1), {"colour": 0})


def test_aov_device_code_has_no_flat_memory_instructions(rtow, tmp_path):
    """The procedure of test_host.py's
    test_device_code_has_no_flat_memory_instructions on librtow_aov.so: its
    gfx950 code reads and writes the scene, the grid and the six buffers
    through address_space(1) / (4) pointers and LDS through address_space(3),
    so it holds global_*, ds_* and scalar loads, and no flat_* instruction."""
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and shutil.which("objcopy")):
        pytest.skip("llvm-objdump / objcopy not available")
    fat = tmp_path / "fatbin.bin"
    co = tmp_path / "gfx950.co"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", rtow.AOV_LIB_PATH, str(fat)],
                   check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + str(fat),
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + str(co)], check=True)
    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)],
                         check=True, capture_output=True, text=True).stdout
    # the ten variants: open x {scan, BVH, grid x 3 placements}
    assert len(re.findall(r"^[0-9a-f]+ <_ZN3rtk10aov_kernel\w+>:$", dis, re.M)) == 10
    ops = re.findall(r"^\s+((?:flat|global|ds)_\w+)", dis, re.M)
    # (LDS only in the four kernels of the two LDS placements: a staging store and the walk's reads each)
    assert sum(o.startswith("global_") for o in ops) > 100 and sum(o.startswith("ds_") for o in ops) >= 8
    flat = sorted(set(o for o in ops if o.startswith("flat_")))
    assert not flat, flat
