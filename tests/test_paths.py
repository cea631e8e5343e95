"""The wavefront loop's device step (include/rt_paths.h, librtow_paths.so), host
side: the twelfth library's exported surface, its ctypes layouts, rt_paths_shift
and rt_paths_scratch_bytes, every argument check that returns before a HIP
call, the Python checks, its gfx950 code's memory instructions, and that
tests/paths_ref.py restates rtow.path_trace's own lines.  The step itself is
checked on the GPU in test_paths_gpu.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import paths_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:[\w\*\s]+?)\b(rt_\w+)\s*\("
FUNCS = sorted(["rt_paths_version", "rt_paths_tile", "rt_paths_scan_block", "rt_paths_shift", "rt_paths_scratch_bytes",
                "rt_paths_step_check", "rt_paths_step_async", "rt_paths_step", "rt_paths_frame_async", "rt_paths_frame"])
INVALID = -1


def _header():
    with open(os.path.join(ROOT, "include", "rt_paths.h")) as f:
        return f.read()


# ---- surface ----------------------------------------------------------------
def test_paths_library_exports_every_declared_symbol(rtow):
    text = _header()
    assert sorted(set(re.findall(DECL, text, re.M))) == FUNCS
    out = subprocess.run(["nm", "-D", "--defined-only", rtow.PATHS_LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for n in FUNCS:
        assert re.search(rf"\bT {n}$", out, re.M), n
    assert not re.search(r"\brt_(aov|guides|route|denoise|temporal|resolve|upscale|trace|segment|bounce)", out)
    assert "g_turn_tab" not in out  # no turn table: the pass compiles none of the render's device helpers
    assert re.search(r"^#define RT_PATHS_VERSION 1$", text, re.M)
    L = rtow.paths_lib()
    assert L.rt_paths_version() == rtow.PATHS_VERSION == 1
    assert L.rt_paths_tile() >= 64 and L.rt_paths_tile() % 64 == 0
    assert L.rt_paths_scan_block() >= 64 and L.rt_paths_scan_block() % 64 == 0
    # the header states what is out of scope and the overlap rule
    assert "STABLE" in text and "dither" in text and "wide sums" in text and "ping-pongs" in text
    with open(os.path.join(ROOT, "ray-tracing-in-one-weekend_amd", "csrc", "rt_paths.hip")) as f:
        src = f.read()
    assert '#include "rt_post.h"' in src and "rt_device.h\"" not in src and "rt_trace_pass.h" not in src
    assert "fmaf" not in src


def test_paths_leaves_the_render_abi_and_the_other_passes_alone(rtow):
    assert rtow.lib().rt_abi_version() == 6 == rtow.ABI_VERSION
    for path in (rtow.LIB_PATH, rtow.AOV_LIB_PATH, rtow.TRACE_LIB_PATH, rtow.SEGMENT_LIB_PATH, rtow.BOUNCE_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert not re.search(r"\brt_paths", out), path


def test_paths_structures_match_the_header(rtow):
    A, O = rtow.PathsIn, rtow.PathsOut
    assert ctypes.sizeof(A) == 88 and ctypes.sizeof(O) == 64
    assert [(f[0], getattr(A, f[0]).offset) for f in A._fields_] == [
        ("n", 0), ("status", 8), ("id", 16), ("position", 24), ("scatter", 32), ("attenuation", 40), ("key", 48),
        ("throughput", 56), ("slot", 64), ("n_slots", 72), ("shift", 80), ("reserved", 84)]
    assert [f[0] for f in O._fields_] == ["sums", "origin", "direction", "from_", "key", "throughput", "slot", "count"]
    text = _header()
    for struct, fields in (("rt_paths_in", A._fields_), ("rt_paths_out", O._fields_)):
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % struct, text, re.S).group(1)
        names = re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(\w+);", body, re.M)
        assert names == [f[0].rstrip("_") for f in fields], names
    assert [f[0] for f in rtow.PATHS_INPUTS] == [f[0] for f in A._fields_[1:9]]
    assert [f[0] for f in rtow.PATHS_NEXT] == list(paths_ref.NEXT)


def test_paths_shift_is_the_renders_f(rtow):
    L = rtow.paths_lib()
    for spp in range(1, 4096):
        assert L.rt_paths_shift(spp) == 31 - (spp.bit_length() - 1), spp
    for spp in (0, -1, -2 ** 31, 4096, 4097, 2 ** 31 - 1):
        assert L.rt_paths_shift(spp) == -1, spp
    assert rtow.paths_shift(100) == 25


def test_paths_scratch_bytes_is_monotone_and_never_zero(rtow):
    L = rtow.paths_lib()
    T = L.rt_paths_tile()
    ns = sorted({0, 1, 63, 64, T - 1, T, T + 1, 4 * T, 4 * T + 1, 5 * T, 10 ** 6, 2 ** 31 - 2, 2 ** 31 - 1})
    got = [L.rt_paths_scratch_bytes(n) for n in ns]
    assert all(g > 0 and g % 16 == 0 for g in got), got
    assert got == sorted(got) and got[-1] > got[0]
    # one uint32 per tile fits
    assert all(g >= 4 * -(-n // T) for g, n in zip(got, ns))
    assert L.rt_paths_scratch_bytes(2 ** 31) == 0 and L.rt_paths_scratch_bytes(2 ** 40) == 0


# ---- rejections ---------------------------------------------------------------
class _Args:
    """A valid step's arguments over host arrays, with overrides."""

    def __init__(self, rtow, n=10, n_slots=4):
        self.rtow, self.n, self.n_slots = rtow, n, n_slots
        self.ins = {name: np.full((n, 3) if ch == 3 else (n,), 1, dt) for name, dt, ch in rtow.PATHS_INPUTS}
        self.outs = {name: np.full((n, 3) if ch == 3 else (n,), 7, dt) for name, dt, ch in rtow.PATHS_NEXT}
        self.sums = np.full((n_slots, 3), 7, np.uint32)
        self.count = np.full(1, 7, np.uint32)
        # the arrays the bounce read: not inputs of the step
        self.bounce_in = {"origin": np.full((n, 3), 7, np.float32), "direction": np.full((n, 3), 7, np.float32),
                          "from": np.full(n, 7, np.int32)}

    def a(self, **over):
        v = dict(n=self.n, n_slots=self.n_slots, shift=25, reserved=0)
        v.update({k: x.ctypes.data for k, x in self.ins.items()})
        v.update(over)
        return self.rtow.PathsIn(**v)

    def o(self, **over):
        v = {("from_" if k == "from" else k): x.ctypes.data for k, x in self.outs.items()}
        v.update(sums=self.sums.ctypes.data, count=self.count.ctypes.data)
        v.update(over)
        return self.rtow.PathsOut(**v)

    def untouched(self):
        return (all((x == 1).all() for x in self.ins.values()) and all((x == 7).all() for x in self.outs.values()) and
                (self.sums == 7).all() and (self.count == 7).all() and all((x == 7).all() for x in self.bounce_in.values()))


def test_paths_step_rejections_come_before_any_hip_call(rtow):
    """Every RT_ERR_INVALID of rt_paths_step and rt_paths_step_async, with a
    stand-in for the context that is never read (no device here), and the
    arrays and kernel_ms left as they were.  rt_paths_step_check gives the
    same verdicts without a context, so that what is accepted can be shown
    too: the next batch's origin, direction and from in the arrays the bounce
    read, NULL outputs, n = 0 with NULL inputs."""
    L = rtow.paths_lib()
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    scratch = np.zeros(64, np.uint8)
    sp = scratch.ctypes.data + (-scratch.ctypes.data % 16)
    ms = ctypes.c_double(-1.0)
    g = _Args(rtow)
    n = g.n

    def all_three(c, a, o, s=sp):
        ap = ctypes.byref(a) if a is not None else None
        op = ctypes.byref(o) if o is not None else None
        return (L.rt_paths_step(c, ap, op, ctypes.byref(ms)), L.rt_paths_step(c, ap, op, None),
                L.rt_paths_step_async(c, ap, op, s, None))

    def rejected(a, o):
        ap = ctypes.byref(a) if a is not None else None
        op = ctypes.byref(o) if o is not None else None
        return all_three(ctx, a, o) == (INVALID,) * 3 and L.rt_paths_step_check(ap, op) == INVALID

    assert all_three(None, g.a(), g.o()) == (INVALID,) * 3
    assert rejected(None, g.o()) and rejected(g.a(), None)
    for name, _, _ in rtow.PATHS_INPUTS:
        assert rejected(g.a(**{name: None}), g.o()), name
    assert rejected(g.a(), g.o(count=None))
    assert rejected(g.a(n=2 ** 31), g.o()) and rejected(g.a(n=2 ** 40), g.o())
    assert rejected(g.a(shift=32), g.o()) and rejected(g.a(shift=-1), g.o())
    assert rejected(g.a(n_slots=(2 ** 32 - 1) // 3 + 1), g.o()) and rejected(g.a(n_slots=2 ** 63), g.o())
    assert rejected(g.a(reserved=1), g.o())
    # the scratch of the asynchronous form: NULL, and misaligned
    assert L.rt_paths_step_async(ctx, ctypes.byref(g.a()), ctypes.byref(g.o()), None, None) == INVALID
    assert L.rt_paths_step_async(ctx, ctypes.byref(g.a()), ctypes.byref(g.o()), sp + 4, None) == INVALID
    # the outgoing key, throughput and slot on each input of the step (first byte, last byte)
    size = {name: (12 if ch == 3 else np.dtype(dt).itemsize) * n for name, dt, ch in rtow.PATHS_INPUTS}
    for out in ("key", "throughput", "slot"):
        for name, arr in g.ins.items():
            assert rejected(g.a(), g.o(**{out: arr.ctypes.data})), (out, name)
            assert rejected(g.a(), g.o(**{out: arr.ctypes.data + size[name] - 1})), (out, name)
    # the exact ping-pong mistake: the same arrays in and out
    assert rejected(g.a(), g.o(key=g.ins["key"].ctypes.data, throughput=g.ins["throughput"].ctypes.data,
                               slot=g.ins["slot"].ctypes.data))
    # origin, direction and from on an input of the step
    assert rejected(g.a(), g.o(origin=g.ins["position"].ctypes.data))
    assert rejected(g.a(), g.o(direction=g.ins["scatter"].ctypes.data + 12 * n - 4))
    assert rejected(g.a(), g.o(from_=g.ins["id"].ctypes.data))
    # sums and count on an input
    assert rejected(g.a(), g.o(sums=g.ins["attenuation"].ctypes.data))
    assert rejected(g.a(), g.o(count=g.ins["status"].ctypes.data + n - 1))
    # an output on another output, on sums, on count
    assert rejected(g.a(), g.o(direction=g.outs["origin"].ctypes.data + 12 * n - 4))
    assert rejected(g.a(), g.o(slot=g.outs["from"].ctypes.data))
    assert rejected(g.a(), g.o(throughput=g.outs["key"].ctypes.data + 4))
    assert rejected(g.a(), g.o(origin=g.sums.ctypes.data + 12 * g.n_slots - 4))
    assert rejected(g.a(), g.o(key=g.sums.ctypes.data))
    assert rejected(g.a(), g.o(count=g.sums.ctypes.data + 8))
    assert rejected(g.a(), g.o(count=g.outs["slot"].ctypes.data + 4 * n - 4))
    assert rejected(g.a(), g.o(sums=g.count.ctypes.data))
    assert ms.value == -1.0 and standin.raw == b"\0" * 64 and g.untouched()
    # accepted, as far as the checks go (the context would be read next)
    ok = lambda a, o: L.rt_paths_step_check(ctypes.byref(a), ctypes.byref(o))  # noqa: E731
    assert ok(g.a(), g.o()) == 0
    assert ok(g.a(), g.o(origin=g.bounce_in["origin"].ctypes.data, direction=g.bounce_in["direction"].ctypes.data,
                         from_=g.bounce_in["from"].ctypes.data)) == 0
    assert ok(g.a(), g.o(sums=None)) == 0 and ok(g.a(n_slots=0), g.o(sums=None)) == 0
    assert ok(g.a(), g.o(origin=None, direction=None, from_=None, key=None, throughput=None, slot=None)) == 0
    assert ok(g.a(shift=0), g.o()) == 0 and ok(g.a(shift=31), g.o()) == 0
    # the largest batch: made-up addresses 2^36 apart (a range is at most 12 (2^31 - 1) bytes; nothing is read)
    far = {name: 2 ** 40 + k * 2 ** 36 for k, (name, _, _) in enumerate(rtow.PATHS_INPUTS)}
    assert ok(g.a(n=2 ** 31 - 1, n_slots=(2 ** 32 - 1) // 3, **far),
              g.o(sums=None, origin=None, direction=None, from_=None, key=None, throughput=None, slot=None,
                  count=2 ** 39)) == 0
    assert rejected(g.a(n=2 ** 31 - 1, **far), g.o(sums=None, origin=None, direction=None, from_=None, key=None,
                                                  throughput=None, slot=None, count=far["key"] + 12 * (2 ** 31 - 1) - 4))
    assert ok(rtow.PathsIn(n=0, shift=3), rtow.PathsOut(count=g.count.ctypes.data)) == 0
    # a sums array that ends where count begins shares no byte with it
    both = np.full(3 * g.n_slots + 1, 7, np.uint32)
    assert ok(g.a(), g.o(sums=both.ctypes.data, count=both.ctypes.data + 12 * g.n_slots)) == 0
    assert g.untouched()


def test_paths_frame_rejections_come_before_any_hip_call(rtow):
    L = rtow.paths_lib()
    standin = ctypes.create_string_buffer(64)
    ctx = ctypes.cast(standin, ctypes.c_void_p)
    sums, frame = np.full(12, 7, np.uint32), np.full(12, 7, np.float32)
    ms = ctypes.c_double(-1.0)

    def both(c, s, k, shift, f):
        return (L.rt_paths_frame(c, s, k, shift, f, ctypes.byref(ms)), L.rt_paths_frame(c, s, k, shift, f, None),
                L.rt_paths_frame_async(c, s, k, shift, f, None))

    bad = (INVALID,) * 3
    sp, fp = sums.ctypes.data, frame.ctypes.data
    assert both(None, sp, 4, 25, fp) == bad
    assert both(ctx, None, 4, 25, fp) == bad and both(ctx, sp, 4, 25, None) == bad
    assert both(ctx, sp, 4, 32, fp) == bad and both(ctx, sp, 4, -1, fp) == bad
    assert both(ctx, sp, (2 ** 32 - 1) // 3 + 1, 25, fp) == bad
    assert both(ctx, sp, 4, 25, sp) == bad and both(ctx, sp, 4, 25, sp + 44) == bad  # in place, and one element
    assert ms.value == -1.0 and standin.raw == b"\0" * 64 and (sums == 7).all() and (frame == 7).all()


def test_paths_python_checks_names_shapes_and_ranges(rtow):
    class NoContext(rtow.Context):
        def __init__(self):  # no device: the checks come before any call
            self._h = None

    ctx = NoContext()
    d = paths_ref.synthetic(4, "mix")
    bounced = {k: d[k] for k in ("status", "id", "position", "scatter", "attenuation")}
    sums = np.zeros((5, 3), np.uint32)
    with pytest.raises(ValueError):
        ctx.paths_step(bounced, d["key"], d["throughput"], d["slot"], sums, 25, which=("origin", "normal"))
    with pytest.raises(ValueError):
        ctx.paths_step({k: v for k, v in bounced.items() if k != "id"}, d["key"], d["throughput"], d["slot"], sums, 25)
    with pytest.raises(ValueError):
        ctx.paths_step(bounced, d["key"][:3], d["throughput"], d["slot"], sums, 25)
    with pytest.raises(ValueError):
        ctx.paths_step(bounced, d["key"], d["throughput"], np.zeros((4, 1), np.uint32), sums, 25)
    with pytest.raises(ValueError):
        ctx.paths_step(bounced, d["key"], d["throughput"], d["slot"], np.zeros((5, 3), np.uint64), 25)
    with pytest.raises(ValueError):
        ctx.paths_step(bounced, d["key"], d["throughput"], d["slot"], np.zeros(7, np.uint32), 25)
    with pytest.raises(ValueError):
        ctx.paths_step(bounced, d["key"], d["throughput"], d["slot"], np.zeros((5, 6), np.uint32)[:, ::2], 25)
    ptrs = {f[0]: 0 for f in rtow.PATHS_INPUTS}
    with pytest.raises(ValueError):
        ctx.paths_step_async(ptrs, 4, 5, 25, 0)  # no count
    ptrs["count"] = 0
    with pytest.raises(ValueError):
        ctx.paths_step_async(dict(ptrs, out_normal=0), 4, 5, 25, 0)
    with pytest.raises(ValueError):
        ctx.paths_step_async({k: v for k, v in ptrs.items() if k != "slot"}, 4, 5, 25, 0)
    for n in (-1, rtow.TRACE_MAX_RAYS + 1):
        with pytest.raises(ValueError):
            ctx.paths_step_async(ptrs, n, 5, 25, 0)
    for n_slots, shift in ((-1, 25), (rtow.PATHS_MAX_SLOTS + 1, 25), (5, 32), (5, -1)):
        with pytest.raises(ValueError):
            ctx.paths_step_async(ptrs, 4, n_slots, shift, 0)
    with pytest.raises(ValueError):
        ctx.paths_frame(np.zeros(7, np.uint32), 25)


def test_path_trace_device_refuses_what_path_trace_refuses(rtow):
    import features_cases as fc

    class Ctx:
        scene, device = fc.clamp_scene(rtow), 0
    cam = rtow.camera_cpu(aspect=2.0)
    for fn in (rtow.path_trace, rtow.path_trace_device):
        Ctx.scene = fc.clamp_scene(rtow)
        with pytest.raises(ValueError):
            fn(Ctx, cam, rtow.make_params(4, 2, 1))  # wide sums
        Ctx.scene = rtow.five_scene()
        with pytest.raises(ValueError):
            fn(Ctx, cam, rtow.make_params(4, 2, 4096))  # dithered sums
    with pytest.raises(ValueError):
        rtow.path_trace_device(Ctx, cam, rtow.make_params(4, 2, 4), chunk_spp=0)
    assert "import torch" in inspect.getsource(rtow.path_trace_device)


# ---- device code --------------------------------------------------------------
def test_paths_device_code_has_its_kernels_and_no_flat_or_scratch_instructions(rtow, tmp_path):
    """test_bounce.py's procedure on librtow_paths.so: count_kernel and
    scatter_kernel (each with and without the deposit), scan_kernel and
    frame_kernel; global_* and ds_* memory instructions only -- no flat_* and no
    scratch_* / buffer_* (spill) instruction -- and a private segment of 0
    bytes in every kernel."""
    import shutil
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and shutil.which("objcopy")):
        pytest.skip("llvm-objdump / objcopy not available")
    fat = tmp_path / "fatbin.bin"
    co = tmp_path / "gfx950.co"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", rtow.PATHS_LIB_PATH, str(fat)], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + str(fat),
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + str(co)], check=True)
    dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)],
                         check=True, capture_output=True, text=True).stdout
    kernels = re.findall(r"^[0-9a-f]+ <(_ZN3rtk\w+)>:$", dis, re.M)
    assert sorted(re.sub(r"^_ZN3rtk\d+(\w+?_kernel).*$", r"\1", k) for k in kernels) == [
        "count_kernel", "count_kernel", "frame_kernel", "scan_kernel", "scatter_kernel", "scatter_kernel"], kernels
    ops = re.findall(r"^\s+((?:flat|global|ds|scratch|buffer)_\w+)", dis, re.M)
    assert sum(o.startswith("global_") for o in ops) > 50 and sum(o.startswith("ds_") for o in ops) >= 8
    assert "global_atomic_add" in ops and "ds_add_u32" in ops  # the deposit, and a wave's count into the tile's
    other = sorted(set(o for o in ops if not o.startswith(("global_", "ds_"))))
    assert not other, other
    # the wave-level idioms are there: a lane's rank from mbcnt, a wave's count from a population count
    assert re.search(r"v_mbcnt_hi_u32_b32", dis) and re.search(r"s_bcnt1_i32_b64", dis)
    readelf = os.path.join(llvm, "llvm-readelf")
    if os.path.exists(readelf):
        notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)
        assert len(sizes) == 6 and set(sizes) == {"0"}, sizes


# ---- the restatement is the loop's ------------------------------------------------
def test_paths_ref_is_path_traces_own_lines():
    """rtow.path_trace's lines between two bounces, copied here, next to
    paths_ref.step inside the same loop, on synthetic bounce results (values
    <= 1, as the loop's are): the same sums, the same next batch in the same
    order, step after step; and paths_ref.frame is the loop's last line."""
    f32, spp, npx, shift = np.float32, 5, 41, 29
    assert shift == 31 - (spp.bit_length() - 1)
    scale = f32(2.0 ** shift)
    n = npx * spp
    first = paths_ref.synthetic(n, "mix", seed=3)
    live = np.arange(n)
    key, thr = first["key"].copy(), np.ones((n, 3), f32)
    sums = np.zeros((npx, 3), np.uint64)                                        # path_trace's state
    r_key, r_thr, r_slot = key.copy(), thr.copy(), (live // spp).astype(np.uint32)  # the restatement's
    r_sums = np.zeros((npx, 3), np.uint32)
    steps = 0
    while live.size:
        got = paths_ref.synthetic(live.size, "mix", seed=100 + steps)
        # -- rtow.path_trace's lines
        thr = thr * got["attenuation"]
        miss = got["status"] == 0
        np.add.at(sums, live[miss] // spp, np.trunc(thr[miss] * scale).astype(np.uint64))
        on = got["status"] == 1
        key = key[on] + np.array([0, 0, 1], np.uint32)
        live, o, d, frm, thr = live[on], got["position"][on], got["scatter"][on], got["id"][on], thr[on]
        # -- the restatement
        nxt, count = paths_ref.step(got["status"], got["id"], got["position"], got["scatter"], got["attenuation"], r_key,
                                    r_thr, r_slot, r_sums, shift)
        r_key, r_thr, r_slot = nxt["key"], nxt["throughput"], nxt["slot"]
        assert count == live.size
        assert nxt["origin"].tobytes() == o.tobytes() and nxt["direction"].tobytes() == d.tobytes()
        assert nxt["from"].tobytes() == frm.tobytes() and r_key.tobytes() == key.tobytes()
        assert r_thr.tobytes() == thr.tobytes() and (r_slot == live // spp).all()
        assert (r_sums == sums.astype(np.uint32)).all()
        steps += 1
    assert steps > 5 and r_sums.any()
    image = sums.astype(np.uint32).astype(f32) * (f32(1.0) / scale)
    assert paths_ref.frame(r_sums, shift).tobytes() == image.tobytes()
    src = inspect.getsource(__import__("rtow").path_trace)
    for line in ('thr = thr * got["attenuation"]', "np.trunc(thr[miss] * scale).astype(np.uint64)",
                 "key = key[on] + np.array([0, 0, 1], np.uint32)"):
        assert line in src, line


def test_paths_ref_clamps_what_the_loop_never_meets():
    f32 = np.float32
    v = np.array([np.nan, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0, 1e30, np.inf, -np.inf], f32)
    got = paths_ref.fixed(v, 31)
    assert got.tolist() == [0, 0, 0, 0, 2 ** 30, 2 ** 31, 4294967040, 4294967040, 4294967040, 0]
    assert paths_ref.fixed(np.array([1.0], f32), 0).tolist() == [1]
    # the sum wraps modulo 2^32
    sums = np.array([[2 ** 32 - 5, 1, 0]], np.uint32)
    one = np.ones((3, 3), f32)
    paths_ref.step(np.zeros(3, np.uint8), np.zeros(3, np.int32), one, one, one, np.zeros((3, 3), np.uint32), one,
                   np.zeros(3, np.uint32), sums, 2)
    assert sums.tolist() == [[7, 13, 12]]
