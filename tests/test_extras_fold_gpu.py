"""GPU: the grid build's folded forms of the first extras group give the
general form's bits.  Every class (both parts folded, either one, neither) at
64x64 and, for a partial tile, 64x40, 8 spp, depth 50, both camera models: the
grid build's pixel sums equal the scan build's and the oracle's bit for bit,
with equal segment counts; and the first-hit pass finds the scan's hits."""
import numpy as np
import pytest

import extras_scenes
import oracle_lib

pytestmark = pytest.mark.gpu

FRAMES = [(64, 64), (64, 40)]


def _scenes(rtow):
    out = {"final": rtow.final_scene()}
    out.update({k: s for k, (s, _) in extras_scenes.hand_made(rtow).items()})
    out.update(extras_scenes.random_with_extras(rtow))
    return out


SCENES = ["final", "big_cz_quarter", "big_cy_one_ulp", "lead_cx_minus_zero", "lead_cx_tiny",
          "final_prefix_65", "final_plus_free_3"]


@pytest.mark.parametrize("name", SCENES)
def test_grid_equals_scan_equals_oracle(rtow, gpu_ctx, name):
    scene = _scenes(rtow)[name]
    gpu_ctx.upload(scene)
    assert rtow.accel_info(scene)["grid_items"] > 0  # RT_FLAG_ACCEL_BVH walks the layer grid
    for w, h in FRAMES:
        for cam in (rtow.camera_cpu(aspect=w / h), rtow.camera_gpu(w, h)):
            p = rtow.make_params(w, h, 8, max_depth=50, seed=23)
            want, segs = oracle_lib.kernel_render(scene, cam, p)
            scan, st_scan = gpu_ctx.render(cam, p)
            p.flags |= rtow.RT_FLAG_ACCEL_BVH
            grid, st_grid = gpu_ctx.render(cam, p)
            for got, st in ((scan, st_scan), (grid, st_grid)):
                n_diff = int((got != want).sum())
                assert n_diff == 0, (name, (w, h), n_diff)
                assert st.segments == segs
            assert grid.tobytes() == scan.tobytes()


def test_first_hit_ids_match_the_scan(rtow, gpu_ctx):
    scene = rtow.final_scene()
    gpu_ctx.upload(scene)
    w, h = FRAMES[0]
    cam = rtow.camera_cpu(aspect=w / h)
    scan = gpu_ctx.aov(cam, rtow.make_params(w, h, 8, seed=23, flags=0), which=("hits", "id"))
    grid = gpu_ctx.aov(cam, rtow.make_params(w, h, 8, seed=23, flags=rtow.RT_FLAG_ACCEL_BVH), which=("hits", "id"))
    assert (scan["id"] >= 0).any() and len(np.unique(scan["id"])) > 4
    assert grid["id"].tobytes() == scan["id"].tobytes()
    assert grid["hits"].tobytes() == scan["hits"].tobytes()
