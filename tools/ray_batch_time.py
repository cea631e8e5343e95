"""Time the ray-batch passes (include/rt_trace.h, include/rt_segment.h, include/rt_bounce.h):
final scene, layer grid, everything in device buffers, HIP events around
repeated enqueues after a warm-up.  There is no target in either mode.

  python tools/ray_batch_time.py --mode trace   [--width 3840 --height 2160 --reps 20 --log profiles/trace_pass.log]
  python tools/ray_batch_time.py --mode segment [--width 3840 --height 2160 --reps 20 --log profiles/segment_pass.log]

trace: rt_trace next to the first-hit pass (include/rt_aov.h) on the same rays,
the pinhole camera's pixel-centre rays of the frame.  Batch (a) holds the rays
in 8x8-tile order, a wave's 64 rays one tile of the frame as in rt_aov; batch
(b) the same rays in a random permutation.  (a) is read against rt_aov at
1 spp on the same frame in the same run (rt_aov jitters its rays inside the
pixel and writes 52 bytes per pixel where rt_trace reads 24 and writes 32),
and (b) shows what incoherent waves cost.

segment: rt_segment next to rt_trace on secondary rays.  rt_trace on batch
(a); from every hit one cosine-weighted hemisphere ray, origin = position,
direction = normal + a uniform unit vector (numpy, seeded), kept in the
primary rays' order.  These are the rays of an ambient-occlusion or a diffuse
bounce pass: neighbours start close together and fan out.  rt_trace is timed
on them twice, first and last; the spread of the two is the run's noise.
rt_segment is timed without a limit (t_max = +inf: the same walks, one more
input) and at world lengths 4, 1 and 0.25: the lines say what a limit saves on
this scene.

bounce: rt_bounce next to rt_trace on the same rays, the final scene's
secondary rays after one step -- the render's camera rays of the frame
(rt_bounce_camera_rays, lens camera, 1 spp) pushed through one rt_bounce, the
scattered ones kept in order.  rt_trace is timed first and last (the noise),
rt_bounce in between with all seven outputs.  Then the wavefront loop
(camera rays, max_depth steps with compaction on the device, torch) over
--loop-width x --loop-height at --loop-spp in chunks of --chunk-spp samples:
the sum of its rt_bounce and camera-ray kernel times next to rt_render's
kernel_ms for the same frame.

  python tools/ray_batch_time.py --mode bounce [--width 3840 --height 2160 --reps 20 --log profiles/bounce_pass.log]

paths: the wavefront loop's glue between two bounces (include/rt_paths.h) over
--loop-width x --loop-height at --loop-spp in chunks of --chunk-spp samples,
three ways in one run, each twice (the spread is the run's noise): (a) the
loop as --mode bounce runs it, torch boolean indexing and no pixel sums; (b)
that loop with the sums formed by torch (index_add_ on int64), so that it does
the same work -- the comparison point; (c) rt_paths_step, rtow.path_trace_device's
sequence.  HIP events around the whole loop (host waits included) and around
every launch sequence; rt_render's kernel_ms for the same segments next to them.

  python tools/ray_batch_time.py --mode paths [--log profiles/paths_pass.log]

Prints the times and writes the same lines to --log."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-in-one-weekend_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before rtow: INTEGRATION.md, "Loading")

import rtow  # noqa: E402

LENGTHS = (4.0, 1.0, 0.25)
FLAGS = rtow.RT_FLAG_ACCEL_BVH


def timed(fn, reps, stream):
    fn()
    fn()
    stream.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def pixel_centre_rays(cam, w, h):
    """The CPU-model pinhole camera's rays through the pixel centres, float32
    (w * h, 3) origins and unnormalised directions (camera_dir with u = 0.5)."""
    f32 = np.float32
    col, row = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    fs = (col + f32(0.5)) * f32(1.0 / (w - 1))
    ft = (f32(h - 1) - row + f32(0.5)) * f32(1.0 / (h - 1))
    eye, corner, hz, vt = (np.array(v[:], f32) for v in (cam.eye, cam.corner, cam.horiz, cam.vert))
    d = corner + fs[..., None] * hz + ft[..., None] * vt - eye
    return np.broadcast_to(eye, d.shape).reshape(-1, 3).copy(), d.astype(f32).reshape(-1, 3)


def tile_order(w, h, tile=8):
    """Pixel indices in 8x8-tile order (tiles row-major, pixels row-major in a tile)."""
    idx = np.arange(w * h).reshape(h, w)
    assert w % tile == 0 and h % tile == 0
    return idx.reshape(h // tile, tile, w // tile, tile).transpose(0, 2, 1, 3).reshape(-1)


def hemisphere_rays(position, normal, seed):
    """One cosine-weighted direction per hit: normal + a uniform unit vector
    (float32; a sum shorter than 1e-3 is replaced by the normal)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=position.shape).astype(np.float32)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = normal + u
    short = np.linalg.norm(d, axis=1) < 1e-3
    d[short] = normal[short]
    return position, d.astype(np.float32)


def device_batch(o, d, dev, fields):
    """The rays on the device and zeroed outputs for `fields`: (tensors kept alive, name -> device pointer)."""
    n = len(o)
    t = {"origin": torch.from_numpy(np.ascontiguousarray(o)).to(dev),
         "direction": torch.from_numpy(np.ascontiguousarray(d)).to(dev)}
    for name, dt, ch in fields:
        t[name] = torch.zeros((n, 3) if ch == 3 else (n,), dtype=getattr(torch, np.dtype(dt).name), device=dev)
    torch.cuda.synchronize()
    return t, {k: v.data_ptr() for k, v in t.items()}


def trace_mode(ctx, cam, w, h, reps, dev, stream, say):
    n, s = w * h, stream.cuda_stream
    o, d = pixel_centre_rays(cam, w, h)
    order = {"(a) 8x8-tile order": tile_order(w, h), "(b) random permutation": np.random.default_rng(1).permutation(n)}
    aov = {}
    for name, _, ch in rtow.AOV_FIELDS:
        dt = torch.float32 if name in ("depth", "position", "normal", "albedo") else torch.int32
        aov[name] = torch.zeros((h, w, 3) if ch == 3 else (h, w), dtype=dt, device=dev)
    torch.cuda.synchronize()
    say(f"frame {w}x{h} ({n} rays), final scene, RT_FLAG_ACCEL_BVH (layer grid), {reps} repetitions after 2 "
        f"warm-up calls, HIP events; rt_trace all four outputs, rt_aov all six at 1 spp")
    p = rtow.make_params(w, h, 1, seed=7, flags=FLAGS)
    ap6 = {k: t.data_ptr() for k, t in aov.items()}
    t_aov = timed(lambda: ctx.aov_async(cam, p, ap6, s), reps, stream)
    say(f"rt_aov 1 spp: {t_aov:8.3f} ms")
    ids = {}
    for label, sel in order.items():
        t, ptrs = device_batch(o[sel], d[sel], dev, rtow.TRACE_FIELDS)
        t_tr = timed(lambda: ctx.trace_async(ptrs, n, FLAGS, s), reps, stream)
        stream.synchronize()
        got = t["id"].cpu().numpy()
        ids[label] = np.empty(n, np.int32)
        ids[label][sel] = got
        say(f"rt_trace {label}: {t_tr:8.3f} ms (ratio to rt_aov {t_tr / t_aov:.2f}), "
            f"{t_tr * 1e6 / n:.3f} ns per ray, hits {int((got >= 0).sum())}, invalid {int((got == -2).sum())}")
    a_ids, b_ids = ids.values()
    say(f"ids of the two orders agree: {bool(np.array_equal(a_ids, b_ids))}")


def segment_mode(ctx, cam, w, h, reps, dev, stream, say):
    s = stream.cuda_stream
    o, d = pixel_centre_rays(cam, w, h)
    sel = tile_order(w, h)
    first = ctx.trace(o[sel], d[sel], which=("id", "position", "normal"), flags=FLAGS)
    hit = first["id"] >= 0
    so, sd = hemisphere_rays(first["position"][hit], first["normal"][hit], seed=17)
    n = len(so)
    ln = np.linalg.norm(sd.astype(np.float64), axis=1)
    say(f"frame {w}x{h}: {w * h} primary rays, {n} hits, one cosine-hemisphere ray per hit (seed 17); final scene, "
        f"RT_FLAG_ACCEL_BVH (layer grid), {reps} repetitions after 2 warm-up calls, HIP events, all outputs")
    out, ptrs = device_batch(so, sd, dev, rtow.SEGMENT_FIELDS)
    tptrs = {k: v for k, v in ptrs.items() if k != "blocked"}

    def time_trace(label):
        t = timed(lambda: ctx.trace_async(tptrs, n, FLAGS, s), reps, stream)
        stream.synchronize()
        ids = out["id"].cpu().numpy()
        say(f"rt_trace {label}: {t:8.3f} ms, {t * 1e6 / n:.3f} ns per ray, hits {int((ids >= 0).sum())}")
        return t, ids

    t_first, ids_trace = time_trace("(first)")
    rows = []
    for label, length in [("t_max = +inf", np.inf)] + [(f"length {L:g}", L) for L in LENGTHS]:
        tm = torch.from_numpy((length / ln).astype(np.float32)).to(dev)
        ptrs["t_max"] = tm.data_ptr()
        torch.cuda.synchronize()
        t = timed(lambda: ctx.segment_async(ptrs, n, FLAGS, s), reps, stream)
        stream.synchronize()
        ids, blocked = out["id"].cpu().numpy(), out["blocked"].cpu().numpy()
        assert ((ids >= 0) == (blocked == 1)).all()
        rows.append((label, t, int(blocked.sum())))
        if not np.isfinite(length):
            say(f"rt_segment {label}: ids equal rt_trace's: {bool(np.array_equal(ids, ids_trace))}")
    t_last, _ = time_trace("(last)")
    t_ref = 0.5 * (t_first + t_last)
    say(f"rt_trace twice: {t_first:.3f} and {t_last:.3f} ms, spread {abs(t_first - t_last):.3f} ms "
        f"({100 * abs(t_first - t_last) / t_ref:.1f} %): the noise; mean {t_ref:.3f} ms")
    for label, t, nb in rows:
        say(f"rt_segment {label}: {t:8.3f} ms, {t / t_ref:.2f} of rt_trace ({t - t_ref:+.3f} ms), "
            f"blocked {nb} ({100 * nb / n:.1f} %)")


def _tensors(n, fields, dev):
    return {name: torch.zeros((n, 3) if ch == 3 else (n,), dtype=getattr(torch, np.dtype(dt).name), device=dev)
            for name, dt, ch in fields}


def wavefront_ms(ctx, cam, p, s_lo, s_cnt, dev, stream, sums=None):
    """Samples [s_lo, s_lo + s_cnt) of every pixel as a wavefront loop on the
    device -> (the kernel time of its camera-ray and rt_bounce launches in ms,
    rays traced).  The pixel sums are not formed: this times the passes.  With
    sums (int64 (pixels, 3)) torch forms them too: throughput, clamp, index_add_."""
    s = stream.cuda_stream
    n = p.local_rows * p.width * s_cnt
    if sums is not None:
        scale = float(2 ** rtow.paths_shift(p.spp))
        with torch.cuda.stream(stream):
            thr = torch.ones((n, 3), device=dev)
            slot = torch.arange(n, device=dev) // s_cnt
    o, d = torch.zeros((n, 3), device=dev), torch.zeros((n, 3), device=dev)
    key = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    frm = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * (p.max_depth + 1))]
    L = rtow.bounce_lib()
    with torch.cuda.stream(stream):
        ev[0].record(stream)
        rtow.check(L.rt_bounce_camera_rays_async(ctx._h, ctypes.byref(cam), ctypes.byref(p), s_lo, s_cnt, o.data_ptr(), d.data_ptr(),
                                                 key.data_ptr(), s), "rt_bounce_camera_rays_async")
        ev[1].record(stream)
        used, traced = 2, 0
        for _ in range(p.max_depth):
            n = o.shape[0]
            if n == 0:
                break
            traced += n
            out = _tensors(n, [f for f in rtow.BOUNCE_FIELDS if f[0] in ("status", "id", "position", "scatter", "attenuation")], dev)
            ptrs = {k: t.data_ptr() for k, t in out.items()}
            ptrs.update({"origin": o.data_ptr(), "direction": d.data_ptr(), "key": key.data_ptr(), "from": frm.data_ptr()})
            ev[used].record(stream)
            ctx.bounce_async(ptrs, n, p.seed, p.flags, s)
            ev[used + 1].record(stream)
            used += 2
            on = out["status"] == rtow.BOUNCE_SCATTERED
            if sums is not None:
                thr = thr * out["attenuation"]
                miss = out["status"] == rtow.BOUNCE_MISS
                sums.index_add_(0, slot[miss], torch.clamp(thr[miss] * scale, 0.0, 4294967040.0).to(torch.int64))
                thr, slot = thr[on].contiguous(), slot[on].contiguous()
            o, d, frm = out["position"][on].contiguous(), out["scatter"][on].contiguous(), out["id"][on].contiguous()
            key = key[on].contiguous()
            key[:, 2] += 1
    stream.synchronize()
    return sum(ev[i].elapsed_time(ev[i + 1]) for i in range(0, used, 2)), traced


def bounce_mode(ctx, a, dev, stream, say):
    w, h, reps, s = a.width, a.height, a.reps, stream.cuda_stream
    cam = rtow.camera_cpu(aspect=w / h, aperture=0.1)
    p = rtow.make_params(w, h, 1, seed=7, flags=FLAGS)
    o, d, key = ctx.camera_rays(cam, p)
    first = ctx.bounce(o, d, key, p.seed, which=("status", "id", "position", "scatter"), flags=FLAGS)
    on = first["status"] == rtow.BOUNCE_SCATTERED
    so, sd, sf = first["position"][on], first["scatter"][on], first["id"][on]
    sk = key[on] + np.array([0, 0, 1], np.uint32)
    n = len(so)
    say(f"frame {w}x{h}: {w * h} camera rays (lens camera, 1 spp, seed 7), {n} scattered after one rt_bounce; final "
        f"scene, RT_FLAG_ACCEL_BVH (layer grid), {reps} repetitions after 2 warm-up calls, HIP events, all outputs")
    t, ptrs = device_batch(so, sd, dev, rtow.BOUNCE_FIELDS)
    t["from"], t["key"] = torch.from_numpy(sf.copy()).to(dev), torch.from_numpy(sk.view(np.int32).copy()).to(dev)
    ptrs.update({"from": t["from"].data_ptr(), "key": t["key"].data_ptr()})
    tptrs = {k: ptrs[k] for k in ("origin", "direction", "id", "t", "position", "normal")}
    torch.cuda.synchronize()
    t_first = timed(lambda: ctx.trace_async(tptrs, n, FLAGS, s), reps, stream)
    t_b = timed(lambda: ctx.bounce_async(ptrs, n, p.seed, FLAGS, s), reps, stream)
    stream.synchronize()
    st = t["status"].cpu().numpy()
    t_last = timed(lambda: ctx.trace_async(tptrs, n, FLAGS, s), reps, stream)
    t_ref = 0.5 * (t_first + t_last)
    say(f"rt_trace twice: {t_first:.3f} and {t_last:.3f} ms, spread {abs(t_first - t_last):.3f} ms "
        f"({100 * abs(t_first - t_last) / t_ref:.1f} %): the noise; mean {t_ref:.3f} ms, {n / t_ref / 1e3:.1f} Mray/s")
    say(f"rt_bounce: {t_b:8.3f} ms, {n / t_b / 1e3:.1f} Mray/s, {t_b / t_ref:.2f} of rt_trace ({t_b - t_ref:+.3f} ms); status "
        f"miss {int((st == 0).sum())}, scattered {int((st == 1).sum())}, absorbed {int((st == 2).sum())}, "
        f"invalid {int((st == 3).sum())}")
    del t
    # the wavefront loop next to rt_render
    lw, lh, spp, chunk = a.loop_width, a.loop_height, a.loop_spp, a.chunk_spp
    cam = rtow.camera_cpu(aspect=lw / lh, aperture=0.1)
    p = rtow.make_params(lw, lh, spp, seed=7, flags=FLAGS)
    ctx.render(cam, p)
    _, stats = ctx.render(cam, p)
    total, traced = 0.0, 0
    wavefront_ms(ctx, cam, p, 0, min(chunk, spp), dev, stream)  # warm-up
    for s_lo in range(0, spp, chunk):
        ms, tr = wavefront_ms(ctx, cam, p, s_lo, min(chunk, spp - s_lo), dev, stream)
        total, traced = total + ms, traced + tr
    say(f"wavefront loop {lw}x{lh} at {spp} spp, max_depth {p.max_depth}, chunks of {chunk} spp: {total:.3f} ms in "
        f"rt_bounce and camera-ray kernels for {traced} rays ({traced / total / 1e3:.1f} Mray/s); rt_render "
        f"{stats.kernel_ms:.3f} ms for {stats.segments} segments ({stats.segments / stats.kernel_ms / 1e3:.1f} Mray/s); "
        f"ratio {total / stats.kernel_ms:.2f}; rays == segments: {traced == stats.segments}")


def paths_loop_ms(ctx, cam, p, chunk, dev, stream):
    """rtow.path_trace_device's sequence with events around every launch
    sequence -> (ms in camera-ray and rt_bounce kernels, ms in the step's three
    kernels, rays traced, the frame)."""
    s, npx, spp, shift = stream.cuda_stream, p.local_rows * p.width, p.spp, rtow.paths_shift(p.spp)
    pairs = {"bounce": [], "step": []}

    def timed_call(kind, fn):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record(stream)
        fn()
        e[1].record(stream)
        pairs[kind].append(e)

    L, traced = rtow.bounce_lib(), 0
    with torch.cuda.stream(stream):
        n = npx * chunk
        f3 = lambda: torch.empty((n, 3), device=dev)  # noqa: E731
        i1 = lambda: torch.empty((n,), dtype=torch.int32, device=dev)  # noqa: E731
        t = {k: f3() for k in ("origin", "direction", "position", "scatter", "attenuation")}
        t.update({"from": i1(), "id": i1(), "status": torch.empty((n,), dtype=torch.uint8, device=dev)})
        key, thr, slot = [torch.empty((n, 3), dtype=torch.int32, device=dev) for _ in range(2)], [f3(), f3()], [i1(), i1()]
        scratch = torch.empty(rtow.paths_scratch_bytes(n), dtype=torch.uint8, device=dev)
        sums = torch.zeros((npx, 3), dtype=torch.int32, device=dev)
        frame, count = torch.zeros((npx, 3), device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        for s_lo in range(0, spp, chunk):
            cnt = min(chunk, spp - s_lo)
            live = npx * cnt
            timed_call("bounce", lambda: rtow.check(L.rt_bounce_camera_rays_async(
                ctx._h, ctypes.byref(cam), ctypes.byref(p), s_lo, cnt, t["origin"].data_ptr(), t["direction"].data_ptr(),
                key[0].data_ptr(), s), "rt_bounce_camera_rays_async"))
            t["from"].fill_(-1)
            thr[0].fill_(1.0)
            slot[0][:live] = torch.arange(live, dtype=torch.int32, device=dev) // cnt
            for depth in range(p.max_depth):
                if live == 0:
                    break
                traced += live
                i, o = depth & 1, (depth + 1) & 1
                ptrs = {k: t[k].data_ptr() for k in ("origin", "direction", "from", "status", "id", "position", "scatter",
                                                     "attenuation")}
                timed_call("bounce", lambda: ctx.bounce_async(dict(ptrs, key=key[i].data_ptr()), live, p.seed, p.flags, s))
                step = {k: t[k].data_ptr() for k in ("status", "id", "position", "scatter", "attenuation")}
                step.update(key=key[i].data_ptr(), throughput=thr[i].data_ptr(), slot=slot[i].data_ptr(),
                            sums=sums.data_ptr(), count=count.data_ptr(), out_origin=t["origin"].data_ptr(),
                            out_direction=t["direction"].data_ptr(), out_from=t["from"].data_ptr(),
                            out_key=key[o].data_ptr(), out_throughput=thr[o].data_ptr(), out_slot=slot[o].data_ptr())
                timed_call("step", lambda: ctx.paths_step_async(step, live, npx, shift, scratch.data_ptr(), s))
                live = int(count.item())
        ctx.paths_frame_async(sums.data_ptr(), npx, shift, frame.data_ptr(), s)
        image = frame.cpu().numpy()
    ms = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in pairs.items()}
    return ms["bounce"], ms["step"], traced, image.reshape(p.local_rows, p.width, 3)


def paths_mode(ctx, a, dev, stream, say):
    lw, lh, spp, chunk = a.loop_width, a.loop_height, a.loop_spp, a.chunk_spp
    cam = rtow.camera_cpu(aspect=lw / lh, aperture=0.1)
    p = rtow.make_params(lw, lh, spp, seed=7, flags=FLAGS)
    ctx.render(cam, p)
    img, stats = ctx.render(cam, p)
    shift = rtow.paths_shift(spp)
    say(f"frame {lw}x{lh} at {spp} spp, max_depth {p.max_depth}, chunks of {chunk} spp, final scene, lens camera, seed 7, "
        f"RT_FLAG_ACCEL_BVH (layer grid); librtow_paths {rtow.device_code_sha16(rtow.PATHS_LIB_PATH)} "
        f"({os.path.relpath(rtow.PATHS_LIB_PATH, ROOT)}), tile {rtow.paths_lib().rt_paths_tile()}, scan block "
        f"{rtow.paths_lib().rt_paths_scan_block()}")
    say(f"rt_render: {stats.kernel_ms:.3f} ms for {stats.segments} segments ({stats.segments / stats.kernel_ms / 1e3:.1f} Mray/s)")

    def whole(fn):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        got = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), got

    def torch_loop(with_sums):
        sums = torch.zeros((lw * lh, 3), dtype=torch.int64, device=dev) if with_sums else None
        total, traced = 0.0, 0
        for s_lo in range(0, spp, chunk):
            ms, tr = wavefront_ms(ctx, cam, p, s_lo, min(chunk, spp - s_lo), dev, stream, sums)
            total, traced = total + ms, traced + tr
        image = None
        if with_sums:
            with torch.cuda.stream(stream):
                image = ((sums & 0xFFFFFFFF).to(torch.float32) * (1.0 / 2 ** shift)).cpu().numpy().reshape(lh, lw, 3)
        return total, None, traced, image

    runs = {"(a) torch indexing, no sums": lambda: torch_loop(False), "(b) torch indexing + index_add_ sums": lambda: torch_loop(True),
            "(c) rt_paths_step": lambda: paths_loop_ms(ctx, cam, p, chunk, dev, stream)}
    small = rtow.make_params(lw, lh, min(chunk, spp), seed=7, flags=FLAGS)
    wavefront_ms(ctx, cam, small, 0, small.spp, dev, stream, torch.zeros((lw * lh, 3), dtype=torch.int64, device=dev))  # warm-up
    paths_loop_ms(ctx, cam, small, small.spp, dev, stream)
    for rnd in ("first", "second"):
        for label, fn in runs.items():
            ms, (bounce, step, traced, image) = whole(fn)
            same = "" if image is None else f"; frame == rt_render's: {image.tobytes() == img.tobytes()}"
            steps = "" if step is None else f", {step:.3f} ms in the step's three kernels"
            say(f"{label} ({rnd}): whole loop {ms:.3f} ms (events, host waits included), {bounce:.3f} ms in rt_bounce and "
                f"camera-ray kernels{steps}; {traced} rays (== segments: {traced == stats.segments}); whole loop / rt_render "
                f"{ms / stats.kernel_ms:.2f}{same}")
    ms, (image, traced) = whole(lambda: rtow.path_trace_device(ctx, cam, p, chunk, stream))
    say(f"rtow.path_trace_device (no per-launch events): whole loop {ms:.3f} ms; frame == rt_render's: "
        f"{image.tobytes() == img.tobytes()}; rays == segments: {traced == stats.segments}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("trace", "segment", "bounce", "paths"), required=True)
    ap.add_argument("--loop-width", type=int, default=1920)
    ap.add_argument("--loop-height", type=int, default=1080)
    ap.add_argument("--loop-spp", type=int, default=100)
    ap.add_argument("--chunk-spp", type=int, default=4)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default=None, help="default: profiles/<mode>_pass.log; '' writes none")
    a = ap.parse_args()
    log = os.path.join(ROOT, "profiles", f"{a.mode}_pass.log") if a.log is None else a.log
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    cam = rtow.camera_cpu(aspect=a.width / a.height, aperture=0.0)
    with rtow.Context(0) as ctx:
        ctx.upload(rtow.final_scene())
        if a.mode == "bounce":
            bounce_mode(ctx, a, dev, stream, say)
        elif a.mode == "paths":
            paths_mode(ctx, a, dev, stream, say)
        else:
            {"trace": trace_mode, "segment": segment_mode}[a.mode](ctx, cam, a.width, a.height, a.reps, dev, stream, say)
    if log:
        with open(log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
