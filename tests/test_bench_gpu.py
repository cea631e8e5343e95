"""bench.py run as the driver runs it (one process, one GPU): a plain run
prints the headline line without the --full objects, and --dump-outputs
writes the last timed step's frame -- the fp32 sums and the write_color bytes
a caller of rt_render_async / rt_tonemap_async receives -- which must equal a
direct render of the same geometry and seed through the C ABI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, STEPS = 256, 144, 16, 2


def test_plain_run_dumps_the_last_timed_frame(rtow, gpu_ctx, tmp_path):
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--width", str(W), "--height", str(H), "--spp", str(SPP), "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mray/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["full"] is False
    for key in ("roofline", "cpu_baseline", "work_per_launch_rank0"):
        assert key not in line

    assert sorted(os.listdir(dump)) == ["frame_bytes.npy", "pixel_sums.npy"]
    sums, u8 = np.load(dump / "pixel_sums.npy"), np.load(dump / "frame_bytes.npy")
    assert sums.dtype == np.float32 and u8.dtype == np.float32
    # the last timed step renders seed STEPS - 1
    gpu_ctx.upload(rtow.final_scene())
    params = rtow.make_params(W, H, SPP, seed=STEPS - 1, max_depth=50, flags=rtow.RT_FLAG_ACCEL_BVH)
    want, _ = gpu_ctx.render(rtow.camera_cpu(aspect=W / H), params)
    assert np.array_equal(sums, want.reshape(-1, 3))
    assert np.array_equal(u8, rtow.tonemap(want, SPP).reshape(-1, 3).astype(np.float32))
