"""rtow -- Python binding (ctypes) of librtow.so, the MI355X render path.

This is the host-side mirror of the reference's process surface for tests,
bench.py and scripting.  Every call goes straight to the C ABI in
include/rt.h; there is no Python or CPU fallback for the render itself: if
librtow.so is missing, or no HIP device is present, the calls raise.

Reference anchors:
  final_scene()   random_scene()        src/cpu/main.cc:32-76
  camera_cpu()    camera::camera        src/cpu/camera.h:8-26
  camera_gpu()    new_camera            src/gpu/camera.h:53-110
  Context.render  render<<<>>>          src/gpu/camera.h:169-195
  tonemap()       write_color           src/cpu/color.h:8-23
  write_ppm()     main.cc:109 / output_image src/gpu/camera.h:197-210
"""
import ctypes
import math
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# RTOW_LIB: load an alternative build (A/B experiments on the GPU box)
LIB_PATH = os.environ.get("RTOW_LIB") or os.path.join(HERE, "librtow.so")
# the first-hit feature pass (include/rt_aov.h): a second library next to librtow.so
AOV_LIB_PATH = os.path.join(HERE, "librtow_aov.so")
# the guided a-trous denoiser (include/rt_denoise.h): a third library on the same terms
DENOISE_LIB_PATH = os.path.join(HERE, "librtow_denoise.so")
# temporal accumulation with camera reprojection (include/rt_temporal.h): a fourth
TEMPORAL_LIB_PATH = os.path.join(HERE, "librtow_temporal.so")
# the clamped temporal resolve with centre reprojection (include/rt_resolve.h): a fifth
RESOLVE_LIB_PATH = os.path.join(HERE, "librtow_resolve.so")
# guided upsampling of a low-resolution frame (include/rt_upscale.h): a sixth
UPSCALE_LIB_PATH = os.path.join(HERE, "librtow_upscale.so")
# feature buffers that follow mirror and glass paths (include/rt_guides.h): a seventh
GUIDES_LIB_PATH = os.path.join(HERE, "librtow_guides.so")
# guide buffers of each pixel's dominant specular route (include/rt_route.h): an eighth
ROUTE_LIB_PATH = os.path.join(HERE, "librtow_route.so")
# closest-hit queries for caller-supplied ray batches (include/rt_trace.h): a ninth
TRACE_LIB_PATH = os.path.join(HERE, "librtow_trace.so")
# the same queries within a per-ray distance limit (include/rt_segment.h): a tenth
SEGMENT_LIB_PATH = os.path.join(HERE, "librtow_segment.so")
# the render's path step for ray batches (librtow_bounce.so, include/rt_bounce.h)
BOUNCE_LIB_PATH = os.path.join(HERE, "librtow_bounce.so")
# the wavefront loop's step between two bounces (include/rt_paths.h); RTOW_PATHS_LIB: another build of it, for A/B runs
PATHS_LIB_PATH = os.environ.get("RTOW_PATHS_LIB") or os.path.join(HERE, "librtow_paths.so")

RT_LAMBERTIAN, RT_METAL, RT_DIELECTRIC = 0, 1, 2
RT_ERR_INVALID = -1
RT_ERR_NO_SCENE = -6
RT_CAMERA_CPU, RT_CAMERA_GPU = 0, 1
RT_FLAG_OPEN_INTERVAL = 1
RT_FLAG_METAL_UNIT_VECTOR = 2
RT_FLAG_GPU_SEMANTICS = 3
RT_FLAG_KEEP_COUNTERS = 1 << 8
RT_FLAG_ACCEL_BVH = 1 << 9
RT_FLAG_COUNT_WORK = 1 << 10
RT_FLAG_PILOT_SCHEDULE = 1 << 11  # launch expensive tiles first (4-spp pilot per frame geometry)
RT_FLAG_LAYER_BVH = 1 << 12  # layer scenes: walk the layer BVH instead of the layer grid
RT_CHUNK_SPP = 64  # include/rt.h: kept for compatibility (pixel sums are exact integers, units split evenly)
RT_TONEMAP_CPU, RT_TONEMAP_GPU = 0, 1  # write_color of src/cpu (fp64) / src/gpu (fp32)
RT_KAT_SPHERE_HIT, RT_KAT_REFLECT, RT_KAT_REFRACT, RT_KAT_REFLECTANCE = 0, 1, 2, 3
ABI_VERSION = 6
AOV_VERSION = 1  # include/rt_aov.h RT_AOV_VERSION
# rt_aov_buffers' fields in order: (name, numpy dtype, channels)
AOV_FIELDS = (("hits", np.uint32, 1), ("id", np.int32, 1), ("depth", np.float32, 1),
              ("position", np.float32, 3), ("normal", np.float32, 3), ("albedo", np.float32, 3))
DENOISE_VERSION = 1  # include/rt_denoise.h RT_DENOISE_VERSION
# rt_denoise_desc's input pointers in order, and its options with their defaults
DENOISE_INPUTS = ("beauty", "hits", "position", "normal", "albedo")
DENOISE_DEFAULTS = {"iterations": 5, "normal_power": 6, "sigma_plane": 0.5, "sigma_color": 0.15}
TEMPORAL_VERSION = 1  # include/rt_temporal.h RT_TEMPORAL_VERSION
# rt_temporal_desc's pointers in order (history_in and out may be NULL), and its options with their defaults
TEMPORAL_BUFFERS = ("cur", "hits", "position", "normal", "history_in", "history_out", "out")
# (in the three *_DEFAULTS below the TYPE of a value is its desc field's: _pass_options converts with it)
TEMPORAL_DEFAULTS = {"max_len": 2, "plane_tol": 0.0003, "normal_cos": 0.9}
RESOLVE_VERSION = 1  # include/rt_resolve.h RT_RESOLVE_VERSION
# rt_resolve_desc's pointers in order (history_in and out may be NULL), its options with their defaults, its flags
RESOLVE_BUFFERS = ("cur", "hits", "depth", "normal", "history_in", "history_out", "out")
RESOLVE_DEFAULTS = {"max_len": 2, "plane_tol": 0.003, "normal_cos": 0.9, "gamma": 1.0}
RESOLVE_KEEP_PARTIAL = 1  # RT_RESOLVE_KEEP_PARTIAL
UPSCALE_VERSION = 1  # include/rt_upscale.h RT_UPSCALE_VERSION
# rt_upscale_desc's pointers in order (stage may be NULL; the albedos with UPSCALE_NO_ALBEDO), its options, its flags
UPSCALE_INPUTS = ("cur", "hits_lo", "position_lo", "normal_lo", "albedo_lo",
                  "hits_hi", "position_hi", "normal_hi", "albedo_hi")
UPSCALE_BUFFERS = UPSCALE_INPUTS + ("out", "stage")
UPSCALE_DEFAULTS = {"plane_tol": 0.1, "normal_cos": -0.5}
UPSCALE_NO_ALBEDO = 1  # RT_UPSCALE_NO_ALBEDO
GUIDES_VERSION = 1  # include/rt_guides.h RT_GUIDES_VERSION
# rt_guides_buffers' fields in order: rt_aov_buffers', then the two counts; the options with their defaults
GUIDES_FIELDS = AOV_FIELDS + (("bounces", np.uint32, 1), ("escaped", np.uint32, 1))
GUIDES_DEFAULTS = {"max_bounces": 8, "max_fuzz": 0.0}
GUIDES_MAX_BOUNCES = 64
ROUTE_VERSION = 1  # include/rt_route.h RT_ROUTE_VERSION
# rt_route_buffers' output fields in order: rt_aov_buffers', then the dominant route and its sample count (a
# ninth pointer, "state", takes rt_route's final state); the options and their rules are rt_guides'
ROUTE_FIELDS = AOV_FIELDS + (("route", np.uint32, 1), ("matched", np.uint32, 1))
ROUTE_STATE_BYTES_PER_PIXEL = 64  # RT_ROUTE_STATE_BYTES_PER_PIXEL: four planes of 16-byte entries
ROUTE_NO_HIT = 0xFFFFFFFF  # "route" of a pixel without a hit sample
TRACE_VERSION = 1  # include/rt_trace.h RT_TRACE_VERSION
# rt_trace_hits' fields in order: (name, numpy dtype, channels); the ids of a ray without a hit
TRACE_FIELDS = (("id", np.int32, 1), ("t", np.float32, 1), ("position", np.float32, 3), ("normal", np.float32, 3))
TRACE_MISS, TRACE_INVALID = -1, -2  # RT_TRACE_MISS, RT_TRACE_INVALID
TRACE_MAX_RAYS = 2 ** 31 - 1
SEGMENT_VERSION = 1  # include/rt_segment.h RT_SEGMENT_VERSION
# rt_segment_hits' fields in order: "blocked" (uint8), then rt_trace_hits'; the ids are rt_trace's
SEGMENT_FIELDS = (("blocked", np.uint8, 1),) + TRACE_FIELDS
BOUNCE_VERSION = 1  # include/rt_bounce.h RT_BOUNCE_VERSION
BOUNCE_MISS, BOUNCE_SCATTERED, BOUNCE_ABSORBED, BOUNCE_INVALID = 0, 1, 2, 3  # rt_bounce_out.status
BOUNCE_FIELDS = ((("status", np.uint8, 1),) + TRACE_FIELDS +
                 (("scatter", np.float32, 3), ("attenuation", np.float32, 3)))
BOUNCE_INPUTS = ("origin", "direction", "from", "key")
PATHS_VERSION = 1  # include/rt_paths.h RT_PATHS_VERSION
# rt_paths_in's arrays and rt_paths_out's next batch: name, dtype, channels
PATHS_INPUTS = (("status", np.uint8, 1), ("id", np.int32, 1), ("position", np.float32, 3), ("scatter", np.float32, 3),
                ("attenuation", np.float32, 3), ("key", np.uint32, 3), ("throughput", np.float32, 3),
                ("slot", np.uint32, 1))
PATHS_NEXT = (("origin", np.float32, 3), ("direction", np.float32, 3), ("from", np.int32, 1), ("key", np.uint32, 3),
              ("throughput", np.float32, 3), ("slot", np.uint32, 1))
PATHS_MAX_SLOTS = (2 ** 32 - 1) // 3
SEGMENT_MISS, SEGMENT_INVALID = -1, -2  # RT_SEGMENT_MISS, RT_SEGMENT_INVALID
# rt_context_set_option (include/rt.h): placement / shape / launch options, never semantics
RT_OPT_GRID_PLACEMENT, RT_OPT_GRID_SCALE, RT_OPT_BVH_LEAF = 1, 2, 3
RT_OPT_BVH_COLLAPSE, RT_OPT_BVH_SIDE, RT_OPT_LAUNCH_SAMPLES, RT_OPT_GRID_FIT = 4, 5, 6, 7
RT_OPT_INTERNAL_GRID_PHASE_X, RT_OPT_INTERNAL_GRID_PHASE_Z = 8, 9  # include/rt_internal.h
RT_GRID_AUTO, RT_GRID_LDS, RT_GRID_CELLS_LDS, RT_GRID_GLOBAL = 0, 1, 2, 3
GRID_PLACEMENTS = {"auto": RT_GRID_AUTO, "lds": RT_GRID_LDS, "cells": RT_GRID_CELLS_LDS, "global": RT_GRID_GLOBAL}

_f = ctypes.POINTER(ctypes.c_float)
_u32 = ctypes.POINTER(ctypes.c_uint32)


class SceneView(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("cx", _f), ("cy", _f), ("cz", _f), ("radius", _f),
                ("mat_kind", _u32), ("albedo_rgb", _f), ("mat_param", _f)]


class SceneBuf(ctypes.Structure):
    _fields_ = [("capacity", ctypes.c_uint32), ("n", ctypes.c_uint32), ("cx", _f), ("cy", _f),
                ("cz", _f), ("radius", _f), ("mat_kind", _u32), ("albedo_rgb", _f),
                ("mat_param", _f)]


class Camera(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int32), ("has_lens", ctypes.c_int32),
                ("eye", ctypes.c_float * 3), ("corner", ctypes.c_float * 3),
                ("horiz", ctypes.c_float * 3), ("vert", ctypes.c_float * 3),
                ("lens_u", ctypes.c_float * 3), ("lens_v", ctypes.c_float * 3)]


class Params(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("spp", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("row_block", ctypes.c_int32),
                ("band_stride", ctypes.c_int32), ("band_offset", ctypes.c_int32),
                ("local_rows", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("units", ctypes.c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("segments", ctypes.c_uint64), ("samples", ctypes.c_uint64),
                ("bf_tests", ctypes.c_uint64), ("sphere_tests", ctypes.c_uint64),
                ("box_tests", ctypes.c_uint64), ("box_hits", ctypes.c_uint64),
                ("wave_steps", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double), ("root_tests", ctypes.c_uint64),
                ("launches", ctypes.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AovBuffers(ctypes.Structure):
    """rt_aov_buffers: device (rt_aov_async) or host (rt_aov) pointers, NULL = not wanted."""
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in AOV_FIELDS]


class GuidesBuffers(ctypes.Structure):
    """rt_guides_buffers: device (rt_guides_async) or host (rt_guides) pointers, NULL = not wanted."""
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in GUIDES_FIELDS]


class GuidesOptions(ctypes.Structure):
    """rt_guides_options: max_bounces (0 = default, -1 = none), max_fuzz, reserved."""
    _fields_ = [("max_bounces", ctypes.c_int32), ("max_fuzz", ctypes.c_float), ("reserved", ctypes.c_uint32)]


class RouteBuffers(ctypes.Structure):
    """rt_route_buffers: device (rt_route_async) or host (rt_route) pointers, NULL = not wanted; state: rt_route only."""
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in ROUTE_FIELDS] + [("state", ctypes.c_void_p)]


class RouteOptions(ctypes.Structure):
    """rt_route_options: max_bounces (0 = default, -1 = none), max_fuzz, reserved."""
    _fields_ = [("max_bounces", ctypes.c_int32), ("max_fuzz", ctypes.c_float), ("reserved", ctypes.c_uint32)]


class TraceRays(ctypes.Structure):
    """rt_trace_rays: n rays, origin and direction as device (rt_trace_async) or host (rt_trace) pointers."""
    _fields_ = [("n", ctypes.c_uint64), ("origin", ctypes.c_void_p), ("direction", ctypes.c_void_p)]


class TraceHits(ctypes.Structure):
    """rt_trace_hits: device (rt_trace_async) or host (rt_trace) pointers, NULL = not wanted."""
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in TRACE_FIELDS]


class SegmentRays(ctypes.Structure):
    """rt_segment_rays: rt_trace_rays and t_max, n floats in units of the direction (NULL = +inf for every ray)."""
    _fields_ = TraceRays._fields_ + [("t_max", ctypes.c_void_p)]


class SegmentHits(ctypes.Structure):
    """rt_segment_hits: device (rt_segment_async) or host (rt_segment) pointers, NULL = not wanted."""
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in SEGMENT_FIELDS]


class BounceRays(ctypes.Structure):
    """rt_bounce_rays: n rays as device (rt_bounce_async) or host (rt_bounce) pointers -- origin, direction
    (unnormalised), from (the sphere a ray starts on, NULL = none), key (pix, sample, depth) -- and the seed."""
    _fields_ = ([("n", ctypes.c_uint64)] + [(name, ctypes.c_void_p) for name in ("origin", "direction", "from_", "key")] +
                [("seed", ctypes.c_uint64)])


class BounceOut(ctypes.Structure):
    """rt_bounce_out: device (rt_bounce_async) or host (rt_bounce) pointers, NULL = not wanted."""
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in BOUNCE_FIELDS]


class PathsIn(ctypes.Structure):
    """rt_paths_in: n rays as device (rt_paths_step_async) or host (rt_paths_step) pointers -- what rt_bounce
    wrote (status, id, position, scatter, attenuation) and what the rays carried into it (key, throughput, slot)
    -- the number of pixel sums and the render's shift F."""
    _fields_ = ([("n", ctypes.c_uint64)] + [(name, ctypes.c_void_p) for name, _, _ in PATHS_INPUTS] +
                [("n_slots", ctypes.c_uint64), ("shift", ctypes.c_int32), ("reserved", ctypes.c_int32)])


class PathsOut(ctypes.Structure):
    """rt_paths_out: the pixel sums (NULL = no deposit), the next batch (NULL = not wanted) and its count."""
    _fields_ = ([("sums", ctypes.c_void_p)] +
                [("from_" if name == "from" else name, ctypes.c_void_p) for name, _, _ in PATHS_NEXT] +
                [("count", ctypes.c_void_p)])


class DenoiseDesc(ctypes.Structure):
    """rt_denoise_desc: the frame, the options (0 = default) and device
    (rt_denoise_async) or host (rt_denoise) pointers."""
    _fields_ = ([(name, ctypes.c_int32) for name in ("width", "height", "spp", "iterations", "normal_power")] +
                [("sigma_plane", ctypes.c_float), ("sigma_color", ctypes.c_float), ("reserved", ctypes.c_int32)] +
                [(name, ctypes.c_void_p) for name in DENOISE_INPUTS + ("out",)])


class TemporalView(ctypes.Structure):
    """rt_temporal_view: world point -> continuous pixel coordinates of a frame."""
    _fields_ = [(name, ctypes.c_float * 3) for name in ("eye", "px", "py", "pw")] + \
               [("x0", ctypes.c_float), ("y0", ctypes.c_float)]


class TemporalDesc(ctypes.Structure):
    """rt_temporal_desc: the frame, the options (0 = default), the previous
    frame's view and device (rt_temporal_async) or host (rt_temporal) pointers."""
    _fields_ = ([(name, ctypes.c_int32) for name in ("width", "height", "spp", "max_len")] +
                [("plane_tol", ctypes.c_float), ("normal_cos", ctypes.c_float), ("reserved", ctypes.c_int32 * 2),
                 ("prev", TemporalView)] +
                [(name, ctypes.c_void_p) for name in TEMPORAL_BUFFERS])


class ResolveRays(ctypes.Structure):
    """rt_resolve_rays: the unnormalised centre ray of pixel (col, row) is
    (d00 + col * du) + row * dv, from eye."""
    _fields_ = [(name, ctypes.c_float * 3) for name in ("eye", "d00", "du", "dv")]


class ResolveDesc(ctypes.Structure):
    """rt_resolve_desc: the frame, the options (0 = default), the flags, the
    previous frame's view, this frame's centre rays and device
    (rt_resolve_async) or host (rt_resolve) pointers."""
    _fields_ = ([(name, ctypes.c_int32) for name in ("width", "height", "spp", "max_len")] +
                [("plane_tol", ctypes.c_float), ("normal_cos", ctypes.c_float), ("gamma", ctypes.c_float),
                 ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32), ("prev", TemporalView),
                 ("now", ResolveRays)] +
                [(name, ctypes.c_void_p) for name in RESOLVE_BUFFERS])


class UpscaleDesc(ctypes.Structure):
    """rt_upscale_desc: the two frames, the options (0 = default), the flags,
    the low-resolution frame's view, the output frame's centre rays and device
    (rt_upscale_async) or host (rt_upscale) pointers."""
    _fields_ = ([(name, ctypes.c_int32) for name in ("lo_width", "lo_height", "lo_spp", "width", "height", "spp")] +
                [("plane_tol", ctypes.c_float), ("normal_cos", ctypes.c_float), ("flags", ctypes.c_uint32),
                 ("reserved", ctypes.c_int32), ("lo_view", TemporalView), ("rays", ResolveRays)] +
                [(name, ctypes.c_void_p) for name in UPSCALE_BUFFERS])


_lib = None
_aov_lib = None
_denoise_lib = None
_temporal_lib = None
_resolve_lib = None
_upscale_lib = None
_guides_lib = None
_route_lib = None
_trace_lib = None
_segment_lib = None
_bounce_lib = None
_paths_lib = None


def _missing(path):
    return RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; "
                        "g.build()'` (or make -C ray-tracing-in-one-weekend_amd)")


def _reject_unknown(names, known, what):
    unknown = [k for k in names if k not in known]
    if unknown:
        raise ValueError(f"unknown {what} {unknown}")


def _pass_options(options, defaults, what):
    """The option fields of a pass's desc from a *_desc function's **options:
    names outside `defaults` are rejected, None means left out, and 0 is
    rejected, since the struct reads 0 as "default"; a field left out is 0."""
    _reject_unknown(options, defaults, f"{what} options")
    opt = {k: v for k, v in options.items() if v is not None}
    zero = [k for k, v in opt.items() if v == 0]
    if zero:
        raise ValueError(f"{what} options {zero} must not be 0 (the struct's 0 means the default)")
    return {k: type(dflt)(opt.get(k, 0)) for k, dflt in defaults.items()}  # (an int default: an int field)


def _load_pass(path, version_fn, version, protos):
    """Load a pass's library (raises if it has not been built): librtow.so
    loads first, since the pass runs on its contexts; protos maps function
    names to (restype or None = int, argtypes); version_fn() must give
    `version`, the constant the header names version_fn.upper()."""
    lib()
    if not os.path.exists(path):
        raise _missing(path)
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in protos.items():
        getattr(L, name).argtypes = argtypes
        if restype is not None:
            getattr(L, name).restype = restype
    got = getattr(L, version_fn)()
    if got != version:
        raise RuntimeError(f"{path}: {version_fn.upper()} {got}, expected {version}")
    return L


def temporal_lib():
    """Load librtow_temporal.so, temporal accumulation with reprojection
    (raises if it has not been built)."""
    global _temporal_lib
    if _temporal_lib is None:
        _temporal_lib = _load_pass(TEMPORAL_LIB_PATH, "rt_temporal_version", TEMPORAL_VERSION, {
            "rt_temporal_history_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
            "rt_temporal_view_from_camera": (None, [ctypes.POINTER(Camera), ctypes.c_int, ctypes.c_int,
                                                    ctypes.POINTER(TemporalView)]),
            "rt_temporal_async": (None, [ctypes.c_void_p, ctypes.POINTER(TemporalDesc), ctypes.c_void_p]),
            "rt_temporal": (None, [ctypes.c_void_p, ctypes.POINTER(TemporalDesc), ctypes.POINTER(ctypes.c_double)])})
    return _temporal_lib


def temporal_view(cam, width, height):
    """The TemporalView of a camera for a width x height frame
    (rt_temporal_view_from_camera): what the NEXT frame's pass gets as prev."""
    v = TemporalView()
    check(temporal_lib().rt_temporal_view_from_camera(ctypes.byref(cam), width, height, ctypes.byref(v)),
          "rt_temporal_view_from_camera")
    return v


def as_temporal_view(view):
    """A TemporalView from anything with eye, px, py, pw (three numbers each), x0 and y0."""
    if isinstance(view, TemporalView):
        return view
    v = TemporalView(x0=float(view.x0), y0=float(view.y0))
    for name in ("eye", "px", "py", "pw"):
        setattr(v, name, (ctypes.c_float * 3)(*[float(x) for x in getattr(view, name)]))
    return v


def temporal_desc(width, height, spp, prev_view=None, **options):
    """A TemporalDesc without pointers.  Options (TEMPORAL_DEFAULTS) left out
    or None take their defaults; a value means itself: plane_tol=inf and
    normal_cos=-1 switch their tests off.  The struct reads 0 as "default", so
    max_len=0, plane_tol=0 and normal_cos=0 cannot be asked for."""
    d = TemporalDesc(width=width, height=height, spp=spp, **_pass_options(options, TEMPORAL_DEFAULTS, "temporal"))
    if prev_view is not None:
        d.prev = as_temporal_view(prev_view)
    return d


def resolve_lib():
    """Load librtow_resolve.so, the clamped temporal resolve with centre
    reprojection (raises if it has not been built)."""
    global _resolve_lib
    if _resolve_lib is None:
        _resolve_lib = _load_pass(RESOLVE_LIB_PATH, "rt_resolve_version", RESOLVE_VERSION, {
            "rt_resolve_rays_from_camera": (None, [ctypes.POINTER(Camera), ctypes.c_int, ctypes.c_int,
                                                   ctypes.POINTER(ResolveRays)]),
            "rt_resolve_async": (None, [ctypes.c_void_p, ctypes.POINTER(ResolveDesc), ctypes.c_void_p]),
            "rt_resolve": (None, [ctypes.c_void_p, ctypes.POINTER(ResolveDesc), ctypes.POINTER(ctypes.c_double)])})
    return _resolve_lib


def resolve_rays(cam, width, height):
    """The ResolveRays of a camera for a width x height frame
    (rt_resolve_rays_from_camera): what THIS frame's pass gets as now_rays."""
    r = ResolveRays()
    check(resolve_lib().rt_resolve_rays_from_camera(ctypes.byref(cam), width, height, ctypes.byref(r)),
          "rt_resolve_rays_from_camera")
    return r


def as_resolve_rays(rays):
    """A ResolveRays from anything with eye, d00, du and dv (three numbers each)."""
    if isinstance(rays, ResolveRays):
        return rays
    r = ResolveRays()
    for name in ("eye", "d00", "du", "dv"):
        setattr(r, name, (ctypes.c_float * 3)(*[float(x) for x in getattr(rays, name)]))
    return r


def resolve_desc(width, height, spp, prev_view=None, now_rays=None, flags=0, **options):
    """A ResolveDesc without pointers.  Options (RESOLVE_DEFAULTS) left out or
    None take their defaults; a value means itself: plane_tol=inf,
    normal_cos=-1 and gamma=inf switch their steps off.  The struct reads 0 as
    "default", so an option of 0 cannot be asked for.  flags:
    RESOLVE_KEEP_PARTIAL or 0."""
    opt = _pass_options(options, RESOLVE_DEFAULTS, "resolve")
    if now_rays is None:
        raise ValueError("now_rays (resolve_rays of this frame's camera) is required")
    d = ResolveDesc(width=width, height=height, spp=spp, flags=int(flags), **opt)
    if prev_view is not None:
        d.prev = as_temporal_view(prev_view)
    d.now = as_resolve_rays(now_rays)
    return d


def upscale_lib():
    """Load librtow_upscale.so, guided upsampling of a low-resolution frame
    (raises if it has not been built)."""
    global _upscale_lib
    if _upscale_lib is None:
        _upscale_lib = _load_pass(UPSCALE_LIB_PATH, "rt_upscale_version", UPSCALE_VERSION, {
            "rt_upscale_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
            "rt_upscale_async": (None, [ctypes.c_void_p, ctypes.POINTER(UpscaleDesc), ctypes.c_void_p,
                                        ctypes.c_void_p]),
            "rt_upscale": (None, [ctypes.c_void_p, ctypes.POINTER(UpscaleDesc), ctypes.POINTER(ctypes.c_double)])})
    return _upscale_lib


def upscale_scratch_bytes(lo_width, lo_height):
    """rt_upscale_scratch_bytes: 48 * w * h, 0 for a size out of range."""
    return upscale_lib().rt_upscale_scratch_bytes(lo_width, lo_height)


def upscale_desc(lo_width, lo_height, lo_spp, width, height, spp, lo_view=None, rays=None, flags=0, **options):
    """An UpscaleDesc without pointers.  Options (UPSCALE_DEFAULTS) left out or
    None take their defaults; a value means itself: plane_tol=inf and
    normal_cos=-1 switch their tests off.  The struct reads 0 as "default", so
    an option of 0 cannot be asked for.  lo_view: temporal_view of the
    low-resolution camera; rays: resolve_rays of the output's camera (the two
    share the eye).  flags: UPSCALE_NO_ALBEDO or 0."""
    opt = _pass_options(options, UPSCALE_DEFAULTS, "upscale")
    if lo_view is None or rays is None:
        raise ValueError("lo_view (temporal_view of the low-resolution camera) and rays (resolve_rays of the "
                         "output's camera) are required")
    d = UpscaleDesc(lo_width=lo_width, lo_height=lo_height, lo_spp=lo_spp, width=width, height=height, spp=spp,
                    flags=int(flags), **opt)
    d.lo_view = as_temporal_view(lo_view)
    d.rays = as_resolve_rays(rays)
    return d


def denoise_lib():
    """Load librtow_denoise.so, the guided a-trous filter (raises if it has
    not been built)."""
    global _denoise_lib
    if _denoise_lib is None:
        _denoise_lib = _load_pass(DENOISE_LIB_PATH, "rt_denoise_version", DENOISE_VERSION, {
            "rt_denoise_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
            "rt_denoise_async": (None, [ctypes.c_void_p, ctypes.POINTER(DenoiseDesc), ctypes.c_void_p,
                                        ctypes.c_void_p]),
            "rt_denoise": (None, [ctypes.c_void_p, ctypes.POINTER(DenoiseDesc), ctypes.POINTER(ctypes.c_double)])})
    return _denoise_lib


def denoise_desc(width, height, spp, **options):
    """A DenoiseDesc without pointers.  Options (DENOISE_DEFAULTS) left out or
    None take their defaults; here a value means itself, so normal_power=0 is
    "no squaring" and sigma_color=0 / sigma_plane=inf switch their terms off
    (the struct's own 0 = default and -1 = off encoding stays inside)."""
    _reject_unknown(options, DENOISE_DEFAULTS, "denoise options")
    opt = {k: v for k, v in options.items() if v is not None}
    if opt.get("iterations", 1) == 0 or opt.get("sigma_plane", 1) == 0:
        raise ValueError("iterations and sigma_plane must be positive")
    d = DenoiseDesc(width=width, height=height, spp=spp)
    d.iterations = int(opt.get("iterations", 0))
    d.normal_power = int(opt["normal_power"]) or -1 if "normal_power" in opt else 0
    d.sigma_plane = float(opt.get("sigma_plane", 0.0))
    d.sigma_color = (float(opt["sigma_color"]) or -1.0) if "sigma_color" in opt else 0.0
    return d


def guides_lib():
    """Load librtow_guides.so, the feature pass that follows mirror and glass
    paths (raises if it has not been built)."""
    global _guides_lib
    if _guides_lib is None:
        head = [ctypes.c_void_p, ctypes.POINTER(Camera), ctypes.POINTER(Params), ctypes.POINTER(GuidesOptions),
                ctypes.POINTER(GuidesBuffers)]
        _guides_lib = _load_pass(GUIDES_LIB_PATH, "rt_guides_version", GUIDES_VERSION, {
            "rt_guides_async": (None, head + [ctypes.c_void_p]),
            "rt_guides": (None, head + [ctypes.POINTER(ctypes.c_double)])})
    return _guides_lib


def guides_options(max_bounces=None, max_fuzz=None):
    """A GuidesOptions.  None takes the default (GUIDES_DEFAULTS); a value means
    itself: max_bounces=0 follows nothing (rt_aov's buffers; the struct spells
    it -1, its own 0 being the default), 1..GUIDES_MAX_BOUNCES bounds the
    chain; max_fuzz >= 0 is the roughest metal that still continues it."""
    o = GuidesOptions()
    if max_bounces is not None:
        if isinstance(max_bounces, bool) or not math.isfinite(max_bounces) or int(max_bounces) != max_bounces:
            raise ValueError("max_bounces must be an integer")
        if not 0 <= max_bounces <= GUIDES_MAX_BOUNCES:
            raise ValueError(f"max_bounces must be in 0..{GUIDES_MAX_BOUNCES}")
        o.max_bounces = int(max_bounces) or -1
    if max_fuzz is not None:
        if not float(max_fuzz) >= 0.0:
            raise ValueError("max_fuzz must be >= 0")
        o.max_fuzz = float(max_fuzz)
    return o


def route_lib():
    """Load librtow_route.so, the feature pass of each pixel's dominant
    specular route (raises if it has not been built)."""
    global _route_lib
    if _route_lib is None:
        head = [ctypes.c_void_p, ctypes.POINTER(Camera), ctypes.POINTER(Params), ctypes.POINTER(RouteOptions),
                ctypes.POINTER(RouteBuffers)]
        _route_lib = _load_pass(ROUTE_LIB_PATH, "rt_route_version", ROUTE_VERSION, {
            "rt_route_state_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
            "rt_route_async": (None, head + [ctypes.c_void_p, ctypes.c_void_p]),
            "rt_route": (None, head + [ctypes.POINTER(ctypes.c_double)])})
    return _route_lib


def route_options(max_bounces=None, max_fuzz=None):
    """A RouteOptions, under guides_options' rules: None takes the default
    (GUIDES_DEFAULTS), a value means itself, max_bounces=0 follows nothing."""
    g = guides_options(max_bounces, max_fuzz)
    return RouteOptions(max_bounces=g.max_bounces, max_fuzz=g.max_fuzz, reserved=0)


def aov_lib():
    """Load librtow_aov.so, the first-hit feature pass (raises if it has not
    been built)."""
    global _aov_lib
    if _aov_lib is None:
        _aov_lib = _load_pass(AOV_LIB_PATH, "rt_aov_version", AOV_VERSION, {
            "rt_aov_async": (None, [ctypes.c_void_p, ctypes.POINTER(Camera), ctypes.POINTER(Params),
                                    ctypes.POINTER(AovBuffers), ctypes.c_void_p]),
            "rt_aov": (None, [ctypes.c_void_p, ctypes.POINTER(Camera), ctypes.POINTER(Params),
                              ctypes.POINTER(AovBuffers), ctypes.POINTER(ctypes.c_double)])})
    return _aov_lib


def trace_lib():
    """Load librtow_trace.so, closest-hit queries for ray batches (raises if it
    has not been built)."""
    global _trace_lib
    if _trace_lib is None:
        _trace_lib = _load_pass(TRACE_LIB_PATH, "rt_trace_version", TRACE_VERSION, {
            "rt_trace_async": (None, [ctypes.c_void_p, ctypes.POINTER(TraceRays), ctypes.POINTER(TraceHits),
                                      ctypes.c_uint32, ctypes.c_void_p]),
            "rt_trace": (None, [ctypes.c_void_p, ctypes.POINTER(TraceRays), ctypes.POINTER(TraceHits),
                                ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)])})
    return _trace_lib


def segment_lib():
    """Load librtow_segment.so, closest hits within a per-ray distance limit
    (raises if it has not been built)."""
    global _segment_lib
    if _segment_lib is None:
        head = [ctypes.c_void_p, ctypes.POINTER(SegmentRays), ctypes.POINTER(SegmentHits), ctypes.c_uint32]
        _segment_lib = _load_pass(SEGMENT_LIB_PATH, "rt_segment_version", SEGMENT_VERSION, {
            "rt_segment_async": (None, head + [ctypes.c_void_p]),
            "rt_segment": (None, head + [ctypes.POINTER(ctypes.c_double)])})
    return _segment_lib


def bounce_lib():
    """Load librtow_bounce.so, the render's path step and camera rays for ray
    batches (raises if it has not been built)."""
    global _bounce_lib
    if _bounce_lib is None:
        head = [ctypes.c_void_p, ctypes.POINTER(BounceRays), ctypes.POINTER(BounceOut), ctypes.c_uint32]
        cam = [ctypes.c_void_p, ctypes.POINTER(Camera), ctypes.POINTER(Params), ctypes.c_int32, ctypes.c_int32,
               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _bounce_lib = _load_pass(BOUNCE_LIB_PATH, "rt_bounce_version", BOUNCE_VERSION, {
            "rt_bounce_async": (None, head + [ctypes.c_void_p]),
            "rt_bounce": (None, head + [ctypes.POINTER(ctypes.c_double)]),
            "rt_bounce_camera_rays_async": (None, cam + [ctypes.c_void_p]),
            "rt_bounce_camera_rays": (None, cam + [ctypes.POINTER(ctypes.c_double)])})
    return _bounce_lib


def paths_lib():
    """Load librtow_paths.so, the wavefront loop's step between two bounces
    (raises if it has not been built)."""
    global _paths_lib
    if _paths_lib is None:
        step = [ctypes.c_void_p, ctypes.POINTER(PathsIn), ctypes.POINTER(PathsOut)]
        frame = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]
        _paths_lib = _load_pass(PATHS_LIB_PATH, "rt_paths_version", PATHS_VERSION, {
            "rt_paths_tile": (None, []), "rt_paths_scan_block": (None, []),
            "rt_paths_shift": (None, [ctypes.c_int32]),
            "rt_paths_scratch_bytes": (ctypes.c_size_t, [ctypes.c_uint64]),
            "rt_paths_step_check": (None, [ctypes.POINTER(PathsIn), ctypes.POINTER(PathsOut)]),
            "rt_paths_step_async": (None, step + [ctypes.c_void_p, ctypes.c_void_p]),
            "rt_paths_step": (None, step + [ctypes.POINTER(ctypes.c_double)]),
            "rt_paths_frame_async": (None, frame + [ctypes.c_void_p]),
            "rt_paths_frame": (None, frame + [ctypes.POINTER(ctypes.c_double)])})
    return _paths_lib


def paths_shift(spp):
    """rt_paths_shift: the render's F for narrow sums, -1 outside 1 .. 4095."""
    return paths_lib().rt_paths_shift(int(spp))


def paths_scratch_bytes(n):
    """rt_paths_scratch_bytes: the device scratch of a step over n rays."""
    return paths_lib().rt_paths_scratch_bytes(int(n))


# the two ray-batch queries, rt_<kind> and rt_<kind>_async: output fields, structures, library
_RAY_BATCH = {"trace": (TRACE_FIELDS, TraceRays, TraceHits, trace_lib),
              "segment": (SEGMENT_FIELDS, SegmentRays, SegmentHits, segment_lib)}


def lib():
    """Load librtow.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise _missing(LIB_PATH)
        # torch's bundled HIP runtime has the same soname as the system one
        # librtow links (libamdhip64.so.7): whichever loads first serves the
        # process, and torch cannot enumerate devices through the system's.
        # So torch, when present, loads first ("Loading").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        d3 = ctypes.POINTER(ctypes.c_double)
        L.rt_abi_version.restype = ctypes.c_int
        L.rt_strerror.restype = ctypes.c_char_p
        L.rt_strerror.argtypes = [ctypes.c_int]
        L.rt_last_hip_error.restype = ctypes.c_int
        L.rt_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.rt_scene_final.argtypes = [ctypes.c_int, ctypes.POINTER(SceneBuf), d3]
        L.rt_scene_five.argtypes = [ctypes.POINTER(SceneBuf)]
        L.rt_camera_cpu.argtypes = [d3, d3, d3, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, ctypes.POINTER(Camera)]
        L.rt_camera_gpu.argtypes = [d3, d3, d3, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_double, ctypes.c_double, ctypes.POINTER(Camera)]
        L.rt_context_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.rt_context_destroy.argtypes = [ctypes.c_void_p]
        L.rt_context_destroy.restype = None
        L.rt_scene_upload.argtypes = [ctypes.c_void_p, ctypes.POINTER(SceneView)]
        L.rt_render_async.argtypes = [ctypes.c_void_p, ctypes.POINTER(Camera), ctypes.POINTER(Params),
                                      ctypes.c_void_p, ctypes.c_void_p]
        L.rt_render.argtypes = [ctypes.c_void_p, ctypes.POINTER(Camera), ctypes.POINTER(Params),
                                ctypes.c_void_p, ctypes.POINTER(Stats)]
        L.rt_collect_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(Stats)]
        L.rt_reset_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        if hasattr(L, "rt_render_progress"):
            L.rt_render_progress.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                             ctypes.POINTER(ctypes.c_uint32)]
        L.rt_tonemap_u8.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        L.rt_tonemap_u8_mode.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p]
        L.rt_tonemap_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.rt_device_kat.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.c_void_p]
        L.rt_write_ppm.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int]
        L.rt_internal_accel_info.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                             ctypes.c_void_p, ctypes.c_size_t]
        if hasattr(L, "rt_internal_launch_plan"):
            L.rt_internal_launch_plan.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                                  ctypes.c_size_t]
        if hasattr(L, "rt_internal_sealed"):
            L.rt_internal_sealed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        if hasattr(L, "rt_context_set_option"):  # (absent in pre-ABI-4 builds loaded for A/B runs)
            L.rt_context_set_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
        _lib = L
    return _lib


class RTError(RuntimeError):
    def __init__(self, status, where):
        L = lib()
        msg = L.rt_strerror(status).decode()
        if status == -2:
            msg += f" (hipError {L.rt_last_hip_error()})"
        super().__init__(f"{where}: {msg} [{status}]")
        self.status = status


def check(status, where):
    if status != 0:
        raise RTError(status, where)


def device_code_sha16(path=None):
    """Fingerprint of the gfx950 code in a built library: sha256 of its
    .hip_fatbin section (the device code objects only; host-side edits leave it
    unchanged, and rebuilding the same source gives the same bytes).  PMC
    summaries record it so that bench.py can flag counters collected on other
    kernel code."""
    import hashlib
    import struct
    with open(path or LIB_PATH, "rb") as f:
        b = f.read()
    shoff = struct.unpack_from("<Q", b, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]
    names = secs[shstrndx][4]
    for s in secs:
        if b[names + s[0]:b.index(b"\0", names + s[0])] == b".hip_fatbin":
            return hashlib.sha256(b[s[4]:s[4] + s[5]]).hexdigest()[:16]
    return None


def _ptr(a, t):
    return a.ctypes.data_as(t)


def _frame_array(name, a, dtype, d, lead=(), tail=(3,)):
    """a as a C-contiguous array of dtype, checked against the shape
    lead + (height, width) + tail of the desc d's frame."""
    a = np.ascontiguousarray(a, dtype)
    if a.shape != lead + (d.height, d.width) + tail:
        raise ValueError(f"{name}: shape {a.shape} does not match the {d.width} x {d.height} frame")
    return a


@dataclass
class Scene:
    """Sphere scene as SoA numpy arrays (fp32)."""
    cx: np.ndarray
    cy: np.ndarray
    cz: np.ndarray
    radius: np.ndarray
    kind: np.ndarray
    albedo: np.ndarray  # (n, 3)
    param: np.ndarray
    rng_next: float = float("nan")

    @property
    def n(self):
        return int(self.cx.shape[0])

    def view(self):
        """A SceneView pointing into this object's arrays (keep self alive)."""
        for name in ("cx", "cy", "cz", "radius", "albedo", "param"):
            a = getattr(self, name)
            if a.dtype != np.float32 or not a.flags.c_contiguous:
                setattr(self, name, np.ascontiguousarray(a, dtype=np.float32))
        if self.kind.dtype != np.uint32 or not self.kind.flags.c_contiguous:
            self.kind = np.ascontiguousarray(self.kind, dtype=np.uint32)
        return SceneView(self.n, _ptr(self.cx, _f), _ptr(self.cy, _f), _ptr(self.cz, _f),
                         _ptr(self.radius, _f), _ptr(self.kind, _u32), _ptr(self.albedo, _f),
                         _ptr(self.param, _f))


def _scene_from(fill, capacity):
    arr = {k: np.zeros(capacity, np.float32) for k in ("cx", "cy", "cz", "radius", "param")}
    kind = np.zeros(capacity, np.uint32)
    albedo = np.zeros((capacity, 3), np.float32)
    buf = SceneBuf(capacity, 0, _ptr(arr["cx"], _f), _ptr(arr["cy"], _f), _ptr(arr["cz"], _f),
                   _ptr(arr["radius"], _f), _ptr(kind, _u32), _ptr(albedo, _f),
                   _ptr(arr["param"], _f))
    nxt = fill(buf)
    n = buf.n
    return Scene(arr["cx"][:n].copy(), arr["cy"][:n].copy(), arr["cz"][:n].copy(),
                 arr["radius"][:n].copy(), kind[:n].copy(), albedo[:n].copy(),
                 arr["param"][:n].copy(), nxt)


def final_scene(half_extent=11):
    """The final random-spheres scene (486 spheres at half_extent=11)."""
    cap = (2 * half_extent) ** 2 + 8

    def fill(buf):
        nxt = ctypes.c_double()
        check(lib().rt_scene_final(half_extent, ctypes.byref(buf), ctypes.byref(nxt)), "rt_scene_final")
        return nxt.value
    return _scene_from(fill, cap)


def five_scene():
    def fill(buf):
        check(lib().rt_scene_five(ctypes.byref(buf)), "rt_scene_five")
        return float("nan")
    return _scene_from(fill, 8)


def _d3(v):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def camera_cpu(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vup=(0, 1, 0), vfov=20.0,
               aspect=16.0 / 9.0, aperture=0.1, focus_dist=10.0):
    cam = Camera()
    check(lib().rt_camera_cpu(_d3(lookfrom), _d3(lookat), _d3(vup), vfov, aspect, aperture,
                              focus_dist, ctypes.byref(cam)), "rt_camera_cpu")
    return cam


def camera_gpu(width, height, lookfrom=(13, 2, 3), lookat=(0, 0, 0), vup=(0, 1, 0), vfov=20.0,
               defocus_angle=0.6, focus_dist=10.0):
    cam = Camera()
    check(lib().rt_camera_gpu(_d3(lookfrom), _d3(lookat), _d3(vup), vfov, width, height,
                              defocus_angle, focus_dist, ctypes.byref(cam)), "rt_camera_gpu")
    return cam


def make_params(width, height, spp, max_depth=50, seed=0, flags=0, rank=0, world=1, row_block=8,
                units=0):
    """Params for rank `rank` of `world` (interleaved row bands of row_block rows).

    units: waves sharing each tile's samples in even shares (0 = automatic);
    scheduling only, the image is the same for every value (fixed-point sums)."""
    if world == 1:
        return Params(width, height, spp, max_depth, seed, max(1, height), 1, 0, height, flags, units)
    band_rows = row_block * world
    n_bands = -(-height // band_rows)  # every rank gets the same number of bands
    return Params(width, height, spp, max_depth, seed, row_block, world, rank, n_bands * row_block,
                  flags, units)


def local_to_global_rows(p):
    r = np.arange(p.local_rows)
    band = r // p.row_block
    return (band * p.band_stride + p.band_offset) * p.row_block + r % p.row_block


def device_count():
    n = ctypes.c_int()
    check(lib().rt_device_count(ctypes.byref(n)), "rt_device_count")
    return n.value


class Context:
    """One HIP device + uploaded scene (rt_context)."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        check(lib().rt_context_create(device, ctypes.byref(h)), "rt_context_create")
        self._h = h
        self.device = device
        self.scene = None

    def close(self):
        if self._h:
            lib().rt_context_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        """rt_context_set_option: placement / shape / launch granularity (0 = default)."""
        check(lib().rt_context_set_option(self._h, option, float(value)), "rt_context_set_option")

    def upload(self, scene, grid_mode=None, grid_scale=None, grid_phase=None):
        """rt_scene_upload; grid_mode ("auto", "lds", "cells", "global") and
        grid_scale / grid_phase ((x, z) cell fractions) set the layer grid's
        options first (the image is the same).
        Options are the context's: they stay set for later uploads until set
        again (0 / "auto" restores the default)."""
        if grid_mode is not None:
            self.set_option(RT_OPT_GRID_PLACEMENT, GRID_PLACEMENTS[grid_mode])
        if grid_scale is not None:
            self.set_option(RT_OPT_GRID_SCALE, grid_scale)
        if grid_phase is not None:
            self.set_option(RT_OPT_INTERNAL_GRID_PHASE_X, grid_phase[0])
            self.set_option(RT_OPT_INTERNAL_GRID_PHASE_Z, grid_phase[1])
        v = scene.view()
        check(lib().rt_scene_upload(self._h, ctypes.byref(v)), "rt_scene_upload")
        self.scene = scene

    def grid_scale(self):
        """The cell scale of the context's current layer grid (RT_OPT_GRID_FIT
        refits it per frame geometry); 0.0 without a grid."""
        lib().rt_internal_grid_scale.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        g = ctypes.c_double()
        check(lib().rt_internal_grid_scale(self._h, ctypes.byref(g)), "rt_internal_grid_scale")
        return g.value

    def render(self, cam, params):
        """Render synchronously; returns (sums float32 [rows, W, 3], Stats)."""
        out = np.zeros((params.local_rows, params.width, 3), np.float32)
        st = Stats()
        check(lib().rt_render(self._h, ctypes.byref(cam), ctypes.byref(params),
                              out.ctypes.data, ctypes.byref(st)), "rt_render")
        return out, st

    def pilot_schedule(self, cam, params):
        """One synchronous render of (cam, params) -- params carries
        RT_FLAG_PILOT_SCHEDULE -- that also shows its schedule
        (rt_internal_pilot_schedule): a dict of "image" (the sums, as render's),
        "pilot_ran" (False: the context's cached order served), "tile_cost"
        (uint32 [blocks * 4], the pilot's segments per tile of the local frame
        in row-major tile order; None unless the pilot ran) and "order" (uint32
        [blocks * units], the block order the launches read; empty when the
        render took launch order)."""
        L = lib()
        L.rt_internal_pilot_schedule.argtypes = [ctypes.c_void_p, ctypes.POINTER(Camera), ctypes.POINTER(Params),
                                                 ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                                 ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                                 ctypes.c_void_p]
        blocks = frame_blocks(params)
        cost = np.zeros(blocks * 4, np.uint32)
        order = np.zeros(blocks * 8, np.uint32)  # (units is at most 8)
        image = np.zeros((params.local_rows, params.width, 3), np.float32)
        ran, n = ctypes.c_int(), ctypes.c_size_t()
        check(L.rt_internal_pilot_schedule(self._h, ctypes.byref(cam), ctypes.byref(params), cost.ctypes.data,
                                           cost.size, ctypes.byref(ran), order.ctypes.data, order.size,
                                           ctypes.byref(n), image.ctypes.data), "rt_internal_pilot_schedule")
        assert n.value <= order.size, n.value
        return {"image": image, "pilot_ran": bool(ran.value), "tile_cost": cost if ran.value else None,
                "order": order[:n.value].copy()}

    def block_order(self):
        """The block order the context holds (rt_internal_context_order), read
        after the device's work is done, so also after render_async on any
        stream: uint32 [blocks * units]; empty when it holds none that is
        valid (no render with RT_FLAG_PILOT_SCHEDULE yet, or an upload since)."""
        L = lib()
        L.rt_internal_context_order.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_size_t)]
        n = ctypes.c_size_t()
        check(L.rt_internal_context_order(self._h, None, 0, ctypes.byref(n)), "rt_internal_context_order")
        order = np.zeros(n.value, np.uint32)
        check(L.rt_internal_context_order(self._h, order.ctypes.data, order.size, ctypes.byref(n)),
              "rt_internal_context_order")
        assert n.value == order.size
        return order

    def render_async(self, cam, params, dev_ptr, stream=0):
        """Enqueue into a device pointer (e.g. torch tensor.data_ptr()) on a hipStream_t."""
        check(lib().rt_render_async(self._h, ctypes.byref(cam), ctypes.byref(params),
                                    ctypes.c_void_p(dev_ptr), ctypes.c_void_p(stream)),
              "rt_render_async")

    def _feature_pass(self, fields, buffers_type, call, name, cam, params, which, opts=(), extra=None):
        """Context.aov / Context.guides / Context.route: the wanted host arrays
        (extra: further ones of the caller's own shape, by field name), the
        call, the dict."""
        _reject_unknown(which, [f[0] for f in fields], "feature buffers")
        out, bufs = dict(extra or {}), buffers_type()
        for field, a in out.items():
            setattr(bufs, field, a.ctypes.data)
        for field, dt, ch in fields:
            if field in which:
                shape = (params.local_rows, params.width) + ((3,) if ch == 3 else ())
                out[field] = np.zeros(shape, dt)
                setattr(bufs, field, out[field].ctypes.data)
        ms = ctypes.c_double()
        check(call(self._h, ctypes.byref(cam), ctypes.byref(params), *opts, ctypes.byref(bufs), ctypes.byref(ms)), name)
        out["kernel_ms"] = ms.value
        return out

    def _feature_pass_async(self, fields, buffers_type, call, name, cam, params, dev_ptrs, stream, opts=()):
        """Context.aov_async / Context.guides_async: the device pointers, the call."""
        _reject_unknown(dev_ptrs, [f[0] for f in fields], "feature buffers")
        bufs = buffers_type()
        for field, ptr in dev_ptrs.items():
            setattr(bufs, field, ptr)
        check(call(self._h, ctypes.byref(cam), ctypes.byref(params), *opts, ctypes.byref(bufs),
                   ctypes.c_void_p(stream)), name)

    def aov(self, cam, params, which=("hits", "id", "depth", "position", "normal", "albedo")):
        """First-hit feature buffers of the render's primary rays (rt_aov,
        include/rt_aov.h), synchronously: a dict of numpy arrays shaped
        (local_rows, W) or (local_rows, W, 3) for the names in `which`, holding
        unnormalised sums over each pixel's hit samples (divide by "hits"), plus
        "kernel_ms"."""
        return self._feature_pass(AOV_FIELDS, AovBuffers, aov_lib().rt_aov, "rt_aov", cam, params, which)

    def aov_async(self, cam, params, dev_ptrs, stream=0):
        """Enqueue the first-hit pass (rt_aov_async) into raw device pointers
        (e.g. torch tensor.data_ptr()): dev_ptrs maps names of AOV_FIELDS to
        device pointers; names left out are not computed."""
        self._feature_pass_async(AOV_FIELDS, AovBuffers, aov_lib().rt_aov_async, "rt_aov_async", cam, params,
                                 dev_ptrs, stream)

    def _ray_batch(self, kind, origins, directions, t_max, which, flags):
        """Context.trace / Context.segment: the arrays, the outputs in `which`, the call."""
        fields, rays_type, hits_type, lib = _RAY_BATCH[kind]
        _reject_unknown(which, [f[0] for f in fields], f"{kind} outputs")
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(directions, np.float32)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError(f"origins and directions must both be (n, 3), got {o.shape} and {d.shape}")
        n = o.shape[0]
        rays = rays_type(n=n, origin=o.ctypes.data, direction=d.ctypes.data)
        if t_max is not None:
            tm = np.asarray(t_max, np.float32)
            if tm.ndim not in (0, 1) or (tm.ndim == 1 and tm.shape[0] != n):
                raise ValueError(f"t_max must be a scalar or ({n},), got {tm.shape}")
            tm = np.ascontiguousarray(np.broadcast_to(tm, (n,)))
            rays.t_max = tm.ctypes.data if n else None
        out, hits = {}, hits_type()
        for field, dt, ch in fields:
            if field in which:
                out[field] = np.zeros((n, 3) if ch == 3 else (n,), dt)
                setattr(hits, field, out[field].ctypes.data)
        ms = ctypes.c_double()
        check(getattr(lib(), f"rt_{kind}")(self._h, ctypes.byref(rays), ctypes.byref(hits), int(flags),
                                            ctypes.byref(ms)), f"rt_{kind}")
        out["kernel_ms"] = ms.value
        return out

    def _ray_batch_async(self, kind, dev_ptrs, n, flags, stream):
        """Context.trace_async / Context.segment_async: the names, the range of n, the device pointers, the call."""
        fields, rays_type, hits_type, lib = _RAY_BATCH[kind]
        inputs, outputs = [f[0] for f in rays_type._fields_[1:]], [f[0] for f in fields]
        _reject_unknown(dev_ptrs, inputs + outputs, f"{kind} buffers")
        missing = [k for k in ("origin", "direction") if k not in dev_ptrs]
        if missing:
            raise ValueError(f"{kind}_async: {missing} missing")
        if not 0 <= int(n) <= TRACE_MAX_RAYS:
            raise ValueError(f"{kind}_async: n = {n} is outside 0 .. {TRACE_MAX_RAYS}")
        rays, hits = rays_type(n=int(n)), hits_type()
        for struct, names in ((rays, inputs), (hits, outputs)):
            for field in names:
                if field in dev_ptrs:
                    setattr(struct, field, dev_ptrs[field])
        check(getattr(lib(), f"rt_{kind}_async")(self._h, ctypes.byref(rays), ctypes.byref(hits), int(flags),
                                                  ctypes.c_void_p(stream)), f"rt_{kind}_async")

    def trace(self, origins, directions, which=("id", "t", "position", "normal"), flags=0):
        """Closest hits of a batch of rays (rt_trace, include/rt_trace.h),
        synchronously: origins and directions are (n, 3) arrays (converted to
        contiguous float32; directions unnormalised), the result a dict of
        numpy arrays for the names in `which` -- "id" int32 (n,) (TRACE_MISS,
        TRACE_INVALID), "t" float32 (n,) (+inf without a hit), "position" and
        "normal" float32 (n, 3) -- plus "kernel_ms".  flags: the interval and
        acceleration flags of a render."""
        return self._ray_batch("trace", origins, directions, None, which, flags)

    def trace_async(self, dev_ptrs, n, flags=0, stream=0):
        """Enqueue the batch query (rt_trace_async) on raw device pointers
        (e.g. torch tensor.data_ptr() of contiguous float32 (n, 3) / int32 (n,)
        tensors): dev_ptrs maps "origin", "direction" and the wanted names of
        TRACE_FIELDS to device pointers; outputs left out are not computed."""
        self._ray_batch_async("trace", dev_ptrs, n, flags, stream)

    def segment(self, origins, directions, t_max=None, which=tuple(f[0] for f in SEGMENT_FIELDS), flags=0):
        """Closest hits of a batch of rays within a distance limit per ray
        (rt_segment, include/rt_segment.h), synchronously.  origins and
        directions as in trace(); t_max an (n,) array in units of the
        unnormalised direction (t_max = 1: the segment from o to o + d), a
        scalar for every ray, or None for no limit.  A candidate counts only
        strictly below the limit.  The result: trace()'s dict plus "blocked",
        uint8 (n,), 1 with a hit on the segment (SEGMENT_MISS: nothing on it;
        SEGMENT_INVALID: trace()'s invalid forms, or a NaN t_max)."""
        return self._ray_batch("segment", origins, directions, t_max, which, flags)

    def segment_async(self, dev_ptrs, n, flags=0, stream=0):
        """Enqueue the limited query (rt_segment_async) on raw device pointers
        (e.g. torch tensor.data_ptr() of contiguous float32 (n, 3) / (n,),
        int32 (n,) and uint8 (n,) tensors): dev_ptrs maps "origin",
        "direction", optionally "t_max" (left out: no limit) and the wanted
        names of SEGMENT_FIELDS to device pointers; outputs left out are not
        computed."""
        self._ray_batch_async("segment", dev_ptrs, n, flags, stream)

    def bounce(self, origins, directions, keys, seed, from_=None, which=tuple(f[0] for f in BOUNCE_FIELDS), flags=0):
        """One path step of the render for a batch of rays (rt_bounce,
        include/rt_bounce.h), synchronously.  origins and directions as in
        trace(); keys a uint32 (n, 3) array of (pix, sample, depth) per ray;
        seed the render's (Params.seed); from_ an int32 (n,) array, the sphere
        each ray starts on (-1 = none), or None for none at all.  The result is
        a dict of numpy arrays for the names in `which` -- "status" uint8 (n,)
        (BOUNCE_MISS, _SCATTERED, _ABSORBED, _INVALID), trace()'s four,
        "scatter" float32 (n, 3) (the next ray's unnormalised direction, from
        "position") and "attenuation" float32 (n, 3) (the albedo, or on a miss
        the sky's factor) -- plus "kernel_ms".  flags: a render's interval,
        metal and acceleration flags."""
        _reject_unknown(which, [f[0] for f in BOUNCE_FIELDS], "bounce outputs")
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(directions, np.float32)
        k = np.ascontiguousarray(keys, np.uint32)
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape or k.shape != o.shape:
            raise ValueError(f"origins, directions and keys must all be (n, 3), got {o.shape}, {d.shape} and {k.shape}")
        n = o.shape[0]
        rays = BounceRays(n=n, origin=o.ctypes.data, direction=d.ctypes.data, key=k.ctypes.data, seed=int(seed))
        if from_ is not None:
            f = np.ascontiguousarray(from_, np.int32)
            if f.shape != (n,):
                raise ValueError(f"from_ must be ({n},), got {f.shape}")
            rays.from_ = f.ctypes.data if n else None
        out, outs = {}, BounceOut()
        for field, dt, ch in BOUNCE_FIELDS:
            if field in which:
                out[field] = np.zeros((n, 3) if ch == 3 else (n,), dt)
                setattr(outs, field, out[field].ctypes.data)
        ms = ctypes.c_double()
        check(bounce_lib().rt_bounce(self._h, ctypes.byref(rays), ctypes.byref(outs), int(flags), ctypes.byref(ms)),
              "rt_bounce")
        out["kernel_ms"] = ms.value
        return out

    def bounce_async(self, dev_ptrs, n, seed, flags=0, stream=0):
        """Enqueue the path step (rt_bounce_async) on raw device pointers (e.g.
        torch tensor.data_ptr() of contiguous tensors): dev_ptrs maps "origin",
        "direction", "key", optionally "from" and the wanted names of
        BOUNCE_FIELDS to device pointers; outputs left out are not computed."""
        outputs = [f[0] for f in BOUNCE_FIELDS]
        _reject_unknown(dev_ptrs, list(BOUNCE_INPUTS) + outputs, "bounce buffers")
        missing = [k for k in ("origin", "direction", "key") if k not in dev_ptrs]
        if missing:
            raise ValueError(f"bounce_async: {missing} missing")
        if not 0 <= int(n) <= TRACE_MAX_RAYS:
            raise ValueError(f"bounce_async: n = {n} is outside 0 .. {TRACE_MAX_RAYS}")
        rays, outs = BounceRays(n=int(n), seed=int(seed)), BounceOut()
        for field, ptr in dev_ptrs.items():
            if field in BOUNCE_INPUTS:
                setattr(rays, "from_" if field == "from" else field, ptr)
            else:
                setattr(outs, field, ptr)
        check(bounce_lib().rt_bounce_async(self._h, ctypes.byref(rays), ctypes.byref(outs), int(flags),
                                           ctypes.c_void_p(stream)), "rt_bounce_async")

    def camera_rays(self, cam, params, sample0=0, samples=None):
        """The render's camera rays of (cam, params) as a batch for bounce()
        (rt_bounce_camera_rays): samples [sample0, sample0 + samples) of every
        pixel of the local frame (samples None: params.spp) -> (origins float32
        (n, 3), directions float32 (n, 3), unnormalised, keys uint32 (n, 3)),
        ray (lrow * W + col) * samples + j.  A padding row's rays are all-zero
        and come back BOUNCE_INVALID."""
        samples = params.spp if samples is None else int(samples)
        n = max(0, params.local_rows * params.width * samples)
        o, d, k = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint32)
        check(bounce_lib().rt_bounce_camera_rays(self._h, ctypes.byref(cam), ctypes.byref(params), int(sample0), samples,
                                                 o.ctypes.data, d.ctypes.data, k.ctypes.data, None),
              "rt_bounce_camera_rays")
        return o, d, k

    def paths_step(self, bounced, keys, throughput, slots, sums, shift,
                   which=tuple(f[0] for f in PATHS_NEXT)):
        """The wavefront loop's step after a bounce (rt_paths_step,
        include/rt_paths.h), synchronously.  bounced: bounce()'s dict with at
        least "status", "id", "position", "scatter" and "attenuation"; keys
        uint32 (n, 3), throughput float32 (n, 3) and slots uint32 (n,) what the
        rays carried into that bounce; sums a C-contiguous uint32 array of 3
        values per pixel sum that the misses are ADDED into in place, or None
        for no deposit; shift the render's F (paths_shift).  The result is a
        dict of the next batch's arrays for the names in `which` ("origin",
        "direction", "from", "key", "throughput", "slot"), trimmed to the
        scattered rays in their order, plus "count" and "kernel_ms"."""
        _reject_unknown(which, [f[0] for f in PATHS_NEXT], "paths outputs")
        ins = dict(bounced, key=keys, throughput=throughput, slot=slots)
        missing = [f[0] for f in PATHS_INPUTS if f[0] not in ins]
        if missing:
            raise ValueError(f"paths_step: {missing} missing")
        n = np.asarray(ins["status"]).shape[0]
        a = PathsIn(n=n, shift=int(shift))
        keep = []
        for name, dt, ch in PATHS_INPUTS:
            v = np.ascontiguousarray(ins[name], dt)
            if v.shape != ((n, 3) if ch == 3 else (n,)):
                raise ValueError(f"paths_step: {name} must be {(n, 3) if ch == 3 else (n,)}, got {v.shape}")
            keep.append(v)
            setattr(a, name, v.ctypes.data)
        o = PathsOut()
        if sums is not None:
            if (not isinstance(sums, np.ndarray) or sums.dtype != np.uint32 or not sums.flags.c_contiguous or
                    not sums.flags.writeable or sums.size % 3):
                raise ValueError("paths_step: sums must be a writeable C-contiguous uint32 array of 3 values per slot")
            a.n_slots, o.sums = sums.size // 3, sums.ctypes.data
        out = {}
        for name, dt, ch in PATHS_NEXT:
            if name in which:
                out[name] = np.zeros((n, 3) if ch == 3 else (n,), dt)
                setattr(o, "from_" if name == "from" else name, out[name].ctypes.data)
        count, ms = np.zeros(1, np.uint32), ctypes.c_double()
        o.count = count.ctypes.data
        check(paths_lib().rt_paths_step(self._h, ctypes.byref(a), ctypes.byref(o), ctypes.byref(ms)), "rt_paths_step")
        out = {k: v[:int(count[0])] for k, v in out.items()}
        out["count"], out["kernel_ms"] = int(count[0]), ms.value
        return out

    def paths_step_async(self, dev_ptrs, n, n_slots, shift, scratch_ptr, stream=0):
        """Enqueue the step (rt_paths_step_async) on raw device pointers (e.g.
        torch tensor.data_ptr() of contiguous tensors): dev_ptrs maps the
        eight names of PATHS_INPUTS and "count" (one uint32) to device
        pointers, and optionally "sums" and the next batch's arrays as
        "out_origin", "out_direction", "out_from", "out_key", "out_throughput"
        and "out_slot"; what is left out is not computed.  scratch_ptr:
        paths_scratch_bytes(n) bytes, 16-byte aligned."""
        inputs = [f[0] for f in PATHS_INPUTS]
        outputs = ["out_" + f[0] for f in PATHS_NEXT]
        _reject_unknown(dev_ptrs, inputs + outputs + ["sums", "count"], "paths buffers")
        missing = [k for k in inputs + ["count"] if k not in dev_ptrs]
        if missing:
            raise ValueError(f"paths_step_async: {missing} missing")
        if not 0 <= int(n) <= TRACE_MAX_RAYS:
            raise ValueError(f"paths_step_async: n = {n} is outside 0 .. {TRACE_MAX_RAYS}")
        if not 0 <= int(n_slots) <= PATHS_MAX_SLOTS or not 0 <= int(shift) <= 31:
            raise ValueError(f"paths_step_async: n_slots = {n_slots} or shift = {shift} is out of range")
        a, o = PathsIn(n=int(n), n_slots=int(n_slots), shift=int(shift)), PathsOut()
        for name, ptr in dev_ptrs.items():
            if name in inputs:
                setattr(a, name, ptr)
            else:
                name = name[4:] if name.startswith("out_") else name
                setattr(o, "from_" if name == "from" else name, ptr)
        check(paths_lib().rt_paths_step_async(self._h, ctypes.byref(a), ctypes.byref(o), ctypes.c_void_p(scratch_ptr),
                                              ctypes.c_void_p(stream)), "rt_paths_step_async")

    def paths_frame(self, sums, shift):
        """The render's final conversion (rt_paths_frame), synchronously: uint32
        sums of any shape -> float32 (float) sums * 2^-shift of that shape."""
        s = np.ascontiguousarray(sums, np.uint32)
        if s.size % 3:
            raise ValueError("paths_frame: sums must hold 3 values per slot")
        out = np.zeros(s.shape, np.float32)
        check(paths_lib().rt_paths_frame(self._h, s.ctypes.data, s.size // 3, int(shift), out.ctypes.data, None),
              "rt_paths_frame")
        return out

    def paths_frame_async(self, dev_sums, n_slots, shift, dev_frame, stream=0):
        """Enqueue the conversion (rt_paths_frame_async) on device pointers: 3 n_slots uint32 -> float32."""
        check(paths_lib().rt_paths_frame_async(self._h, ctypes.c_void_p(dev_sums), int(n_slots), int(shift),
                                               ctypes.c_void_p(dev_frame), ctypes.c_void_p(stream)),
              "rt_paths_frame_async")

    def visible(self, a, b, shrink=1e-3, flags=0):
        """Whether point b[i] is visible from point a[i]: a bool (n,) array,
        True where no sphere lies on the segment.  a and b are (n, 3) (or one
        of them a single point, (3,)); the query is segment() with d = b - a
        and t_max = 1 - shrink, and the answer is not blocked.

        Both ends are open, each by a fraction of the segment's length.  At a,
        t_min = 0.001 in units of d skips everything within 0.001 |b - a| of
        the start, so a segment that starts ON a surface (a shading point, a
        trace() position) does not see that surface -- and would not see
        another one that close either.  At b, shrink cuts the last shrink
        |b - a| off: with the default a segment that ends ON a surface (a point
        on a light, another hit point) stops 0.001 |b - a| short of it and is
        not blocked by it, where shrink = 0 leaves that to the last bit of the
        surface's root.  A point deeper inside a sphere than those margins is
        hidden by the sphere's shell.  The answer is ~blocked and nothing else:
        a[i] == b[i] (a zero direction, an invalid ray) reads as visible, a
        point from itself, and so does a pair with a non-finite component; use
        segment() and its "id" to tell those apart.  shrink = 1 leaves nothing
        of the segment, and every pair reads as visible."""
        a = np.asarray(a, np.float32)
        b = np.asarray(b, np.float32)
        if a.ndim not in (1, 2) or b.ndim not in (1, 2) or a.shape[-1] != 3 or b.shape[-1] != 3:
            raise ValueError(f"a and b must be (n, 3) or (3,), got {a.shape} and {b.shape}")
        if a.ndim == 2 and b.ndim == 2 and a.shape != b.shape:
            raise ValueError(f"a and b must hold the same number of points, got {a.shape} and {b.shape}")
        if not 0.0 <= float(shrink) <= 1.0:  # (a NaN fails too)
            raise ValueError(f"shrink = {shrink} is outside 0 .. 1")
        a, b = np.broadcast_arrays(np.atleast_2d(a), np.atleast_2d(b))
        got = self.segment(a, b - a, np.float32(1.0) - np.float32(shrink), which=("blocked",), flags=flags)
        return got["blocked"] == 0

    def guides(self, cam, params, which=tuple(f[0] for f in GUIDES_FIELDS), max_bounces=None, max_fuzz=None):
        """Feature buffers that follow each sample's path through mirrors and
        glass to the first rough surface (rt_guides, include/rt_guides.h),
        synchronously: Context.aov's dict (the same keys, layout and sum
        contract, so denoise / temporal / resolve / upscale take it as it is)
        plus "bounces" and "escaped".  Options: see guides_options."""
        _reject_unknown(which, [f[0] for f in GUIDES_FIELDS], "feature buffers")
        opts = guides_options(max_bounces, max_fuzz)
        return self._feature_pass(GUIDES_FIELDS, GuidesBuffers, guides_lib().rt_guides, "rt_guides", cam, params,
                                  which, (ctypes.byref(opts),))

    def guides_async(self, cam, params, dev_ptrs, stream=0, max_bounces=None, max_fuzz=None):
        """Enqueue the pass (rt_guides_async) into raw device pointers (e.g.
        torch tensor.data_ptr()): dev_ptrs maps names of GUIDES_FIELDS to device
        pointers; names left out are not computed."""
        _reject_unknown(dev_ptrs, [f[0] for f in GUIDES_FIELDS], "feature buffers")
        opts = guides_options(max_bounces, max_fuzz)
        self._feature_pass_async(GUIDES_FIELDS, GuidesBuffers, guides_lib().rt_guides_async, "rt_guides_async", cam,
                                 params, dev_ptrs, stream, (ctypes.byref(opts),))

    def route(self, cam, params, which=tuple(f[0] for f in ROUTE_FIELDS), max_bounces=None, max_fuzz=None):
        """Guide buffers of each pixel's dominant specular route (rt_route,
        include/rt_route.h), synchronously: Context.aov's dict (the same keys,
        layout and sum contract: the dominant route's mean features times
        "hits") plus "route" ((bounces << 1) | escaped of that route,
        ROUTE_NO_HIT without a hit) and "matched" (the samples the mean is
        over).  "state" in `which` adds the pass's final per-pixel state, uint32
        (4, local_rows, W, 4): the four planes of 16-byte entries the header
        documents.  Options: see route_options."""
        names = [f[0] for f in ROUTE_FIELDS]
        _reject_unknown(which, names + ["state"], "feature buffers")
        opts = route_options(max_bounces, max_fuzz)
        extra = {"state": np.zeros((4, params.local_rows, params.width, 4), np.uint32)} if "state" in which else None
        return self._feature_pass(ROUTE_FIELDS, RouteBuffers, route_lib().rt_route, "rt_route", cam, params,
                                  [n for n in which if n != "state"], (ctypes.byref(opts),), extra)

    def route_async(self, cam, params, dev_ptrs, state, stream=0, max_bounces=None, max_fuzz=None):
        """Enqueue the pass (rt_route_async) into raw device pointers (e.g.
        torch tensor.data_ptr()): dev_ptrs maps names of ROUTE_FIELDS to device
        pointers, names left out are not computed; state is device memory of
        route_lib().rt_route_state_bytes(W, local_rows) bytes, 16-byte aligned,
        that the pass works in and leaves its final state in."""
        _reject_unknown(dev_ptrs, [f[0] for f in ROUTE_FIELDS], "feature buffers")
        opts = route_options(max_bounces, max_fuzz)

        def call(h, c, p, o, b, s):
            return route_lib().rt_route_async(h, c, p, o, b, ctypes.c_void_p(state), s)
        self._feature_pass_async(ROUTE_FIELDS, RouteBuffers, call, "rt_route_async", cam, params, dev_ptrs, stream,
                                 (ctypes.byref(opts),))

    def denoise(self, beauty, aov, spp, **options):
        """The guided a-trous filter (rt_denoise, include/rt_denoise.h),
        synchronously, on host arrays: beauty (H, W, 3) float32 sums of a
        whole frame, aov the dict Context.aov returns for the same parameters
        ("hits", "position", "normal", "albedo" are read).  Options:
        DENOISE_DEFAULTS (see denoise_desc).  Returns the filtered sums
        (H, W, 3) float32; self.denoise_ms holds the launches' event time."""
        d = denoise_desc(int(np.shape(beauty)[1]), int(np.shape(beauty)[0]), spp, **options)
        missing = [k for k in DENOISE_INPUTS[1:] if k not in aov]
        if missing:
            raise ValueError(f"feature buffers {missing} are missing")
        keep = {"beauty": _frame_array("beauty", beauty, np.float32, d),
                "hits": _frame_array("hits", aov["hits"], np.uint32, d, tail=())}
        for k in DENOISE_INPUTS[2:]:
            keep[k] = _frame_array(k, aov[k], np.float32, d)
        for k, a in keep.items():
            setattr(d, k, a.ctypes.data)
        out = np.zeros((d.height, d.width, 3), np.float32)
        d.out = out.ctypes.data
        ms = ctypes.c_double()
        check(denoise_lib().rt_denoise(self._h, ctypes.byref(d), ctypes.byref(ms)), "rt_denoise")
        self.denoise_ms = ms.value
        return out

    def denoise_async(self, dev_ptrs, width, height, spp, scratch_ptr, stream=0, **options):
        """Enqueue the filter (rt_denoise_async) on raw device pointers (e.g.
        torch tensor.data_ptr()): dev_ptrs maps DENOISE_INPUTS and "out" to
        device pointers ("out" may be the beauty buffer), scratch_ptr is
        denoise_lib().rt_denoise_scratch_bytes(width, height) bytes."""
        _reject_unknown(dev_ptrs, DENOISE_INPUTS + ("out",), "denoise buffers")
        d = denoise_desc(width, height, spp, **options)
        for name, ptr in dev_ptrs.items():
            setattr(d, name, ptr)
        check(denoise_lib().rt_denoise_async(self._h, ctypes.byref(d), ctypes.c_void_p(scratch_ptr),
                                             ctypes.c_void_p(stream)), "rt_denoise_async")

    def temporal(self, cur, aov, spp, prev_view=None, history=None, **options):
        """Temporal accumulation with reprojection (rt_temporal,
        include/rt_temporal.h), synchronously, on host arrays: cur (H, W, 3)
        float32 sums of this frame (the render's or the denoiser's), aov the
        dict Context.aov returns for this frame ("hits", "position", "normal"
        are read), history the (3, H, W, 4) float32 array the previous
        frame's call returned and prev_view that frame's temporal_view (both
        None: no history).  Options: TEMPORAL_DEFAULTS (see temporal_desc).
        Returns (out, history_out): the accumulated sums (H, W, 3) and this
        frame's history; self.temporal_ms holds the launch's event time."""
        return self._history_pass("temporal", temporal_lib, TEMPORAL_BUFFERS[1:4], cur, aov, history,
                                  prev_view, lambda w, h: temporal_desc(w, h, spp, prev_view, **options))

    def _history_pass(self, what, get_lib, inputs, cur, aov, history, prev_view, make_desc):
        """What Context.temporal and Context.resolve share: the host arrays
        (cur, the feature buffers `inputs` of aov, the history when there is
        one) staged into make_desc(width, height), out and history_out
        allocated, the call rt_<what> of get_lib() (loaded only after the
        arguments passed) and self.<what>_ms."""
        if (history is None) != (prev_view is None):
            raise ValueError("history and prev_view go together")
        d = make_desc(int(np.shape(cur)[1]), int(np.shape(cur)[0]))
        missing = [k for k in inputs if k not in aov]
        if missing:
            raise ValueError(f"feature buffers {missing} are missing")
        keep = {"cur": _frame_array("cur", cur, np.float32, d)}
        for k in inputs:
            keep[k] = _frame_array(k, aov[k], np.uint32 if k == "hits" else np.float32, d,
                                   tail=() if k in ("hits", "depth") else (3,))
        if history is not None:
            keep["history_in"] = _frame_array("history_in", history, np.float32, d, lead=(3,), tail=(4,))
        for k, a in keep.items():
            setattr(d, k, a.ctypes.data)
        out = np.zeros((d.height, d.width, 3), np.float32)
        history_out = np.zeros((3, d.height, d.width, 4), np.float32)
        d.out, d.history_out = out.ctypes.data, history_out.ctypes.data
        ms = ctypes.c_double()
        check(getattr(get_lib(), "rt_" + what)(self._h, ctypes.byref(d), ctypes.byref(ms)), "rt_" + what)
        setattr(self, what + "_ms", ms.value)
        return out, history_out

    def temporal_async(self, dev_ptrs, width, height, spp, prev_view, stream=0, **options):
        """Enqueue the pass (rt_temporal_async) on raw device pointers (e.g.
        torch tensor.data_ptr()): dev_ptrs maps TEMPORAL_BUFFERS to device
        pointers ("history_in" and "out" may be left out or None, "out" may be
        the cur buffer; the histories are
        temporal_lib().rt_temporal_history_bytes(width, height) bytes each and
        must not overlap); prev_view: the view history_in was made with (None
        without one)."""
        _reject_unknown(dev_ptrs, TEMPORAL_BUFFERS, "temporal buffers")
        d = temporal_desc(width, height, spp, prev_view, **options)
        for name, ptr in dev_ptrs.items():
            setattr(d, name, ptr)
        check(temporal_lib().rt_temporal_async(self._h, ctypes.byref(d), ctypes.c_void_p(stream)),
              "rt_temporal_async")

    def resolve(self, cur, aov, spp, prev_view=None, now_rays=None, history=None, flags=0, **options):
        """The clamped temporal resolve (rt_resolve, include/rt_resolve.h),
        synchronously, on host arrays: cur (H, W, 3) float32 sums of this
        frame, aov the dict Context.aov returns for this frame and the same
        spp ("hits", "depth", "normal" are read), now_rays this frame's
        resolve_rays, history the (3, H, W, 4) float32 array the previous
        frame's call (or Context.temporal) returned and prev_view that frame's
        temporal_view (both None: no history).  Options: RESOLVE_DEFAULTS (see
        resolve_desc).  Returns (out, history_out) as Context.temporal;
        self.resolve_ms holds the launch's event time."""
        return self._history_pass("resolve", resolve_lib, RESOLVE_BUFFERS[1:4], cur, aov, history,
                                  prev_view,
                                  lambda w, h: resolve_desc(w, h, spp, prev_view, now_rays, flags, **options))

    def resolve_async(self, dev_ptrs, width, height, spp, prev_view, now_rays, stream=0, flags=0, **options):
        """Enqueue the pass (rt_resolve_async) on raw device pointers (e.g.
        torch tensor.data_ptr()): dev_ptrs maps RESOLVE_BUFFERS to device
        pointers ("history_in" and "out" may be left out or None; "out" must
        not be the cur buffer; the histories are
        temporal_lib().rt_temporal_history_bytes(width, height) bytes each and
        must not overlap); prev_view: the view history_in was made with (None
        without one); now_rays: this frame's resolve_rays."""
        _reject_unknown(dev_ptrs, RESOLVE_BUFFERS, "resolve buffers")
        d = resolve_desc(width, height, spp, prev_view, now_rays, flags, **options)
        for name, ptr in dev_ptrs.items():
            setattr(d, name, ptr)
        check(resolve_lib().rt_resolve_async(self._h, ctypes.byref(d), ctypes.c_void_p(stream)),
              "rt_resolve_async")

    def upscale(self, cur, aov_lo, lo_spp, aov_hi, spp, lo_view=None, rays=None, flags=0, want_stage=True,
                **options):
        """Guided upsampling (rt_upscale, include/rt_upscale.h), synchronously,
        on host arrays: cur (h, w, 3) float32 sums of the low-resolution frame
        over lo_spp samples, aov_lo the dict Context.aov returns for that frame
        and aov_hi the one for the output frame, traced with spp ("hits",
        "position", "normal" and, without UPSCALE_NO_ALBEDO, "albedo" are
        read; the output's size is aov_hi's), lo_view the low-resolution
        camera's temporal_view and rays the output camera's resolve_rays.
        Options: UPSCALE_DEFAULTS (see upscale_desc).  Returns (out, stage):
        the sums (H, W, 3) float32, mean x lo_spp, and which step produced
        each pixel (H, W) uint8 (None with want_stage=False);
        self.upscale_ms holds the launches' event time."""
        names = ("hits", "position", "normal") + (() if int(flags) & UPSCALE_NO_ALBEDO else ("albedo",))
        for what, aov in (("aov_lo", aov_lo), ("aov_hi", aov_hi)):
            missing = [k for k in names if k not in aov]
            if missing:
                raise ValueError(f"feature buffers {missing} are missing in {what}")
        d = upscale_desc(int(np.shape(cur)[1]), int(np.shape(cur)[0]), lo_spp, int(np.shape(aov_hi["hits"])[1]),
                         int(np.shape(aov_hi["hits"])[0]), spp, lo_view, rays, flags, **options)
        lo = DenoiseDesc(width=d.lo_width, height=d.lo_height)  # (the two frames, for _frame_array)
        hi = DenoiseDesc(width=d.width, height=d.height)
        keep = {"cur": _frame_array("cur", cur, np.float32, lo)}
        for tag, aov, fr in (("lo", aov_lo, lo), ("hi", aov_hi, hi)):
            keep["hits_" + tag] = _frame_array("hits_" + tag, aov["hits"], np.uint32, fr, tail=())
            for k in names[1:]:
                keep[f"{k}_{tag}"] = _frame_array(f"{k}_{tag}", aov[k], np.float32, fr)
        for k, a in keep.items():
            setattr(d, k, a.ctypes.data)
        out = np.zeros((d.height, d.width, 3), np.float32)
        stage = np.zeros((d.height, d.width), np.uint8) if want_stage else None
        d.out = out.ctypes.data
        if want_stage:
            d.stage = stage.ctypes.data
        ms = ctypes.c_double()
        check(upscale_lib().rt_upscale(self._h, ctypes.byref(d), ctypes.byref(ms)), "rt_upscale")
        self.upscale_ms = ms.value
        return out, stage

    def upscale_async(self, dev_ptrs, lo_width, lo_height, lo_spp, width, height, spp, lo_view, rays, scratch_ptr,
                      stream=0, flags=0, **options):
        """Enqueue the pass (rt_upscale_async) on raw device pointers (e.g.
        torch tensor.data_ptr()): dev_ptrs maps UPSCALE_BUFFERS to device
        pointers ("stage" may be left out or None, the albedos with
        UPSCALE_NO_ALBEDO), scratch_ptr is upscale_scratch_bytes(lo_width,
        lo_height) bytes, 16-byte aligned."""
        _reject_unknown(dev_ptrs, UPSCALE_BUFFERS, "upscale buffers")
        d = upscale_desc(lo_width, lo_height, lo_spp, width, height, spp, lo_view, rays, flags, **options)
        for name, ptr in dev_ptrs.items():
            setattr(d, name, ptr)
        check(upscale_lib().rt_upscale_async(self._h, ctypes.byref(d), ctypes.c_void_p(scratch_ptr),
                                             ctypes.c_void_p(stream)), "rt_upscale_async")

    def tonemap_async(self, dev_sums, n_pixels, spp, dev_out, mode=RT_TONEMAP_CPU, stream=0):
        """write_color on the device: fp32 sums -> bytes, both device pointers."""
        check(lib().rt_tonemap_async(self._h, ctypes.c_void_p(dev_sums), n_pixels, spp, mode,
                                     ctypes.c_void_p(dev_out), ctypes.c_void_p(stream)), "rt_tonemap_async")

    def progress(self):
        """rt_render_progress: (launches done, launches total) of the last render."""
        d, t = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().rt_render_progress(self._h, ctypes.byref(d), ctypes.byref(t)), "rt_render_progress")
        return d.value, t.value

    def reset_stats(self, stream=0):
        check(lib().rt_reset_stats(self._h, ctypes.c_void_p(stream)), "rt_reset_stats")

    def collect_stats(self):
        st = Stats()
        check(lib().rt_collect_stats(self._h, ctypes.byref(st)), "rt_collect_stats")
        return st


def path_trace(ctx, cam, params):
    """rt_render as a wavefront loop over ray batches, the worked example of
    Context.camera_rays and Context.bounce: bit for bit the render's sums
    (float32 (local_rows, W, 3)), and the rays traced.  Narrow pixel sums
    without dither only: spp < 4096 and every albedo <= 1."""
    opaque = ctx.scene.albedo[np.asarray(ctx.scene.kind) != 2]  # (the render reads a dielectric's albedo as 1)
    if params.spp >= 4096 or (opaque.size and float(opaque.max()) > 1.0):
        raise ValueError("path_trace: dithered (spp >= 4096) and wide (an albedo above 1) pixel sums are not restated")
    f32, npx, spp = np.float32, params.local_rows * params.width, params.spp
    scale = f32(2.0 ** (31 - max(spp, 1).bit_length() + 1))  # 2^F, F = 31 - floor(log2 spp)
    sums, traced = np.zeros((npx, 3), np.uint64), 0
    o, d, key = ctx.camera_rays(cam, params)
    live = np.nonzero(np.repeat(local_to_global_rows(params) < params.height, params.width * spp))[0]  # no padding rows
    o, d, key, frm, thr = o[live], d[live], key[live], np.full(live.size, -1, np.int32), np.ones((live.size, 3), f32)
    for _ in range(params.max_depth):
        if not live.size:
            break
        traced += live.size
        got = ctx.bounce(o, d, key, params.seed, frm, ("status", "id", "position", "scatter", "attenuation"), params.flags)
        thr = thr * got["attenuation"]  # the sample's radiance at a miss, the throughput after a hit
        miss = got["status"] == BOUNCE_MISS
        np.add.at(sums, live[miss] // spp, np.trunc(thr[miss] * scale).astype(np.uint64))
        on = got["status"] == BOUNCE_SCATTERED  # compaction: absorbed paths and misses leave
        key = key[on] + np.array([0, 0, 1], np.uint32)
        live, o, d, frm, thr = live[on], got["position"][on], got["scatter"][on], got["id"][on], thr[on]
    image = sums.astype(np.uint32).astype(f32) * (f32(1.0) / scale)  # paths still alive stay black
    return image.reshape(params.local_rows, params.width, 3), traced


def _narrow_sums_only(ctx, params, who):
    opaque = ctx.scene.albedo[np.asarray(ctx.scene.kind) != 2]  # (the render reads a dielectric's albedo as 1)
    if params.spp >= 4096 or (opaque.size and float(opaque.max()) > 1.0):
        raise ValueError(f"{who}: dithered (spp >= 4096) and wide (an albedo above 1) pixel sums are not restated")


def path_trace_device(ctx, cam, params, chunk_spp=4, stream=None):
    """path_trace's loop on the device (the worked example of
    Context.paths_step_async): camera rays per chunk of chunk_spp samples, then
    max_depth rounds of rt_bounce and rt_paths_step with key, throughput and
    slot ping-ponged, and rt_paths_frame at the end.  Only each step's count (4
    bytes) crosses to the host.  -> (float32 (local_rows, W, 3), bit for bit
    the render's sums, and the rays traced).  A padding row's rays are the
    camera batch's all-zero ones: rt_bounce reports them INVALID and the step
    drops them.  stream: a torch.cuda.Stream of the caller's (not torch's
    default stream, whose handle 0 means "the context's own" to the passes);
    None: a stream of the loop's own, which waits for torch's current one."""
    import torch
    _narrow_sums_only(ctx, params, "path_trace_device")
    if int(chunk_spp) < 1:
        raise ValueError(f"path_trace_device: chunk_spp = {chunk_spp} must be at least 1")
    npx, spp, shift = params.local_rows * params.width, params.spp, 31 - max(params.spp, 1).bit_length() + 1
    dev = torch.device("cuda", ctx.device)
    if stream is None:
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
    elif stream.cuda_stream == 0:
        raise ValueError("path_trace_device: torch's default stream is not a stream of the caller's own")
    s, traced = stream.cuda_stream, 0
    valid_px = int((local_to_global_rows(params) < params.height).sum()) * params.width
    with torch.cuda.stream(stream):
        sums = torch.zeros((max(npx, 1), 3), dtype=torch.int32, device=dev)
        frame = torch.zeros((max(npx, 1), 3), dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        bufs = {}  # per chunk size (the last chunk may be shorter)
        for s_lo in range(0, spp, int(chunk_spp)):
            cnt = min(int(chunk_spp), spp - s_lo)
            n = npx * cnt
            if n == 0:
                break
            if cnt not in bufs:
                f3 = lambda: torch.empty((n, 3), dtype=torch.float32, device=dev)  # noqa: E731
                i1 = lambda: torch.empty((n,), dtype=torch.int32, device=dev)  # noqa: E731
                b = {"origin": f3(), "direction": f3(), "from": i1(), "status": torch.empty((n,), dtype=torch.uint8, device=dev),
                     "id": i1(), "position": f3(), "scatter": f3(), "attenuation": f3(),
                     "key": [torch.empty((n, 3), dtype=torch.int32, device=dev) for _ in range(2)],
                     "throughput": [f3(), f3()], "slot": [i1(), i1()],
                     "slot0": torch.arange(n, dtype=torch.int32, device=dev) // cnt,
                     "scratch": torch.empty(paths_scratch_bytes(n), dtype=torch.uint8, device=dev)}
                bufs[cnt] = b
            b = bufs[cnt]
            check(bounce_lib().rt_bounce_camera_rays_async(ctx._h, ctypes.byref(cam), ctypes.byref(params), s_lo, cnt,
                                                           b["origin"].data_ptr(), b["direction"].data_ptr(),
                                                           b["key"][0].data_ptr(), s), "rt_bounce_camera_rays_async")
            b["from"].fill_(-1)
            b["throughput"][0].fill_(1.0)
            b["slot"][0].copy_(b["slot0"])
            live, pad = n, n - valid_px * cnt  # (the padding rows' rays leave in the first step, untraced)
            for depth in range(params.max_depth):
                if live == 0:
                    break
                traced += live - (pad if depth == 0 else 0)
                i, o = depth & 1, (depth + 1) & 1
                ctx.bounce_async({"origin": b["origin"].data_ptr(), "direction": b["direction"].data_ptr(),
                                  "from": b["from"].data_ptr(), "key": b["key"][i].data_ptr(),
                                  "status": b["status"].data_ptr(), "id": b["id"].data_ptr(),
                                  "position": b["position"].data_ptr(), "scatter": b["scatter"].data_ptr(),
                                  "attenuation": b["attenuation"].data_ptr()}, live, params.seed, params.flags, s)
                ctx.paths_step_async({"status": b["status"].data_ptr(), "id": b["id"].data_ptr(),
                                      "position": b["position"].data_ptr(), "scatter": b["scatter"].data_ptr(),
                                      "attenuation": b["attenuation"].data_ptr(), "key": b["key"][i].data_ptr(),
                                      "throughput": b["throughput"][i].data_ptr(), "slot": b["slot"][i].data_ptr(),
                                      "sums": sums.data_ptr(), "count": count.data_ptr(),
                                      "out_origin": b["origin"].data_ptr(), "out_direction": b["direction"].data_ptr(),
                                      "out_from": b["from"].data_ptr(), "out_key": b["key"][o].data_ptr(),
                                      "out_throughput": b["throughput"][o].data_ptr(), "out_slot": b["slot"][o].data_ptr()},
                                     live, npx, shift, b["scratch"].data_ptr(), s)
                live = int(count.item())  # the 4 bytes
        if npx:
            ctx.paths_frame_async(sums.data_ptr(), npx, shift, frame.data_ptr(), s)
        image = frame[:npx].cpu().numpy()
    return image.reshape(params.local_rows, params.width, 3), traced


def tonemap(sums, spp, mode=RT_TONEMAP_CPU):
    """write_color on the host: src/cpu's fp64 levels, or src/gpu's fp32 ones."""
    sums = np.ascontiguousarray(sums, dtype=np.float32)
    out = np.zeros(sums.shape, np.uint8)
    n_pix = sums.size // 3
    check(lib().rt_tonemap_u8_mode(sums.ctypes.data, n_pix, spp, mode, out.ctypes.data),
          "rt_tonemap_u8_mode")
    return out


def device_kat(kind, cases, device=0):
    """Evaluate the render kernel's device arithmetic on known-answer cases
    (rt_device_kat): cases [n, <=10] float64 -> [n, 9] float64."""
    cases = np.asarray(cases, np.float64)
    inp = np.zeros((cases.shape[0], 10), np.float64)
    inp[:, :cases.shape[1]] = cases
    out = np.zeros((cases.shape[0], 9), np.float64)
    check(lib().rt_device_kat(device, kind, inp.ctypes.data, inp.shape[0], out.ctypes.data), "rt_device_kat")
    return out


ACCEL_INFO_KEYS = ("nodes_per_order", "bvh_slots", "layer_mode", "extra_pair0", "n_extra_pairs",
                   "grid_nx", "grid_nz", "grid_items", "grid_lds_bytes", "grid_fits_lds",
                   "max_items_per_cell", "grid_starts_ok", "grid_ring_empty", "oref_milli",
                   "layer_slots", "listed_cells", "grid_placement", "grid_scale_milli")
# rt_internal_accel_info's values 36..42: the layer grid's geometry as the kernel gets it (float32 bits)
ACCEL_INFO_GRID_KEYS = ("grid_xi", "grid_zi", "grid_g", "grid_x1", "grid_z1", "grid_x0", "grid_z0")
ACCEL_INFO_N = 43  # RT_ACCEL_INFO_N


def accel_info(scene, grid_mode="auto", grid_scale=0.0):
    """What rt_scene_upload would build for `scene` with those grid options,
    computed on the host (rt_internal_accel_info; no device): a dict of
    ACCEL_INFO_KEYS (ints) and ACCEL_INFO_GRID_KEYS (numpy float32, the very
    bits the kernel gets; 0 without a grid)."""
    v = scene.view()
    out = np.zeros(ACCEL_INFO_N, np.uint64)
    check(lib().rt_internal_accel_info(ctypes.byref(v), GRID_PLACEMENTS[grid_mode], float(grid_scale),
                                       out.ctypes.data, out.size), "rt_internal_accel_info")
    info = {k: int(x) for k, x in zip(ACCEL_INFO_KEYS, out)}
    geom = out[36:36 + len(ACCEL_INFO_GRID_KEYS)].astype(np.uint32).view(np.float32)
    info.update(zip(ACCEL_INFO_GRID_KEYS, geom))
    return info


def grid_fit(scene, cam, width, height, phase=(0.0, 0.0)):
    """What RT_OPT_GRID_FIT picks for `scene` seen by `cam` in a width x height
    frame, computed on the host (rt_internal_grid_fit_phase; no device), with
    the grid origin shifted by `phase` cells (RT_OPT_INTERNAL_GRID_PHASE_X / _Z): (cell
    scale or 0.0 without an LDS grid, [(candidate scale, modelled cost)])."""
    L = lib()
    L.rt_internal_grid_fit_phase.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_double, ctypes.c_double,
                                             ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_size_t)]
    v = scene.view()
    sc, n = ctypes.c_double(), ctypes.c_size_t()
    costs = np.zeros(2 * 64, np.float64)
    check(L.rt_internal_grid_fit_phase(ctypes.byref(v), ctypes.byref(cam), width, height, float(phase[0]),
                                       float(phase[1]), ctypes.byref(sc), costs.ctypes.data, 64,
                                       ctypes.byref(n)), "rt_internal_grid_fit_phase")
    return sc.value, [(float(costs[2 * i]), float(costs[2 * i + 1])) for i in range(min(64, n.value))]


def sealed(scene):
    """Per sphere, whether the kernel's opaque-inside rule applies to it (a
    sealed lambertian sphere), computed on the host
    (rt_internal_sealed; no device): a bool array."""
    v = scene.view()
    out = np.zeros(max(scene.n, 1), np.uint8)
    check(lib().rt_internal_sealed(ctypes.byref(v), out.ctypes.data, scene.n), "rt_internal_sealed")
    return out[:scene.n].astype(bool)


RT_EXTRAS_AXIAL, RT_EXTRAS_COAXIAL = 1, 2


def extras_info(scene):
    """The extras of a layer scene (the spheres off the layer) as
    rt_scene_upload would lay them out, computed on the host
    (rt_internal_accel_info's values 18..35; no device): (class bits
    RT_EXTRAS_* of the first group of four, the centre y its coaxial spheres
    share as a float32, the original index of each extras slot in scan order,
    -1 = padding; at most the first 16 slots)."""
    v = scene.view()
    out = np.zeros(36, np.uint64)
    check(lib().rt_internal_accel_info(ctypes.byref(v), 0, 0.0, out.ctypes.data, out.size), "rt_internal_accel_info")
    n = min(2 * int(out[4]), 16) if out[2] else 0
    cy = np.array([int(out[19])], np.uint32).view(np.float32)[0]
    return int(out[18]), cy, out[20:20 + n].astype(np.int64).astype(np.int32) - 1


LAUNCH_PLAN_KEYS = ("ranges", "chunks", "units", "entries", "launches")


def launch_plan(params, launch_samples=0.0):
    """How rt_render would cut a render with `params` into launches under a
    launch-sample budget (0 = default), computed on the host
    (rt_internal_launch_plan; no device): a dict of LAUNCH_PLAN_KEYS."""
    out = np.zeros(len(LAUNCH_PLAN_KEYS), np.uint64)
    check(lib().rt_internal_launch_plan(ctypes.byref(params), float(launch_samples), out.ctypes.data, out.size),
          "rt_internal_launch_plan")
    return {k: int(x) for k, x in zip(LAUNCH_PLAN_KEYS, out)}


def frame_blocks(params):
    """The render's blocks for `params`: four 8x8 tiles (one wave each) per
    block over the local frame's tiles in row-major order (csrc/rt_frame.h)."""
    tiles = -(-params.width // 8) * -(-params.local_rows // 8)
    return -(-tiles // 4)


def block_order_host(tile_cost, blocks, units, device=0):
    """The pilot schedule's device sort alone (rt_internal_block_order_host),
    on `device`: tile_cost uint32 [blocks * 4] -> the launch order, uint32
    [blocks * units]: blocks by decreasing cost (the sum of their four tiles),
    equal costs in block order, a block's units adjacent."""
    L = lib()
    L.rt_internal_block_order_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_void_p]
    cost = np.ascontiguousarray(tile_cost, np.uint32)
    if cost.shape != (blocks * 4,):
        raise ValueError(f"tile_cost: shape {cost.shape}, expected ({blocks * 4},)")
    order = np.zeros(blocks * units, np.uint32)
    check(L.rt_internal_block_order_host(device, cost.ctypes.data, blocks, units, order.ctypes.data),
          "rt_internal_block_order_host")
    return order


def write_ppm(path, rgb, binary=False):
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[0], rgb.shape[1]
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        check(lib().rt_write_ppm(fd, rgb.ctypes.data, w, h, 1 if binary else 0), "rt_write_ppm")
    finally:
        os.close(fd)
