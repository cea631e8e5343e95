"""The pilot schedule's reference (tests/sched_ref.py, the oracle's per-pixel
segment counts) checked on the CPU, and the non-vacuity of the GPU cases of
test_sched_gpu.py shown from the oracle alone: no device is used here."""
import numpy as np
import pytest

import oracle_lib
import sched_cases
import sched_ref

GRID = sched_cases.GRID


def _sum_cases(rtow):
    final, five = sched_cases.scene(rtow, "final"), sched_cases.scene(rtow, "five")
    return {
        "final_grid_67x37x5": (final, rtow.camera_cpu(aspect=67 / 37), rtow.make_params(67, 37, 5, seed=3, flags=GRID)),
        "five_64x36x4": (five, rtow.camera_cpu(aspect=64 / 36), rtow.make_params(64, 36, 4, seed=4)),
        "five_gpu_semantics": (five, rtow.camera_gpu(64, 36), rtow.make_params(64, 36, 4, seed=5, flags=3)),
        "final_banded": (final, rtow.camera_cpu(aspect=67 / 37),
                         rtow.make_params(67, 37, 5, seed=6, flags=GRID, world=3, rank=1, row_block=8)),
    }


@pytest.mark.parametrize("name", ["final_grid_67x37x5", "five_64x36x4", "five_gpu_semantics", "final_banded"])
def test_pixel_segments_sum_to_the_renders_total(rtow, name):
    """The per-pixel counts add up to kernel_render's segments, the total that
    the GPU's stats.segments is already checked against; padding rows count 0."""
    scene, cam, p = _sum_cases(rtow)[name]
    seg = oracle_lib.kernel_pixel_segments(scene, cam, p)
    _, total = oracle_lib.kernel_render(scene, cam, p)
    assert seg.shape == (p.local_rows, p.width) and seg.dtype == np.uint32
    assert int(seg.astype(np.int64).sum()) == total > 0
    inside = rtow.local_to_global_rows(p) < p.height
    assert not seg[~inside].any() and seg[inside].min() >= p.spp  # every traced sample has a first segment


def test_pixel_segments_do_not_depend_on_spp_or_the_band_split(rtow):
    """Samples are counter-based: the first 4 samples' counts at spp = 9 are
    those at spp = 4, and a rank's rows count what the whole frame's rows do."""
    scene, cam, p = _sum_cases(rtow)["final_banded"]
    whole = rtow.make_params(67, 37, 4, seed=6, flags=GRID)
    full = oracle_lib.kernel_pixel_segments(scene, cam, whole)
    p9 = rtow.make_params(67, 37, 9, seed=6, flags=GRID)
    assert np.array_equal(oracle_lib.kernel_pixel_segments(scene, cam, p9, samples=4), full)
    assert not np.array_equal(oracle_lib.kernel_pixel_segments(scene, cam, p9), full)
    band = oracle_lib.kernel_pixel_segments(scene, cam, p, samples=4)
    grow = rtow.local_to_global_rows(p)
    inside = grow < 37
    assert 0 < inside.sum() < p.local_rows  # the share has padding rows
    assert np.array_equal(band[inside], full[grow[inside]])


def test_tile_costs_on_a_hand_made_frame(rtow):
    """19 x 11 pixels in 3 x 2 tiles: every pixel counts 1, so a tile's cost
    is its area inside the frame; two blocks, the second with two padding
    tiles.  Banded (rank 1 of 2, 4-row bands over 11 rows: local rows 0-3 and
    4-7 are the frame's 4-7 and 12-15, the latter outside): one row of tiles,
    half of each inside."""
    p = rtow.make_params(19, 11, 4)
    cost = sched_ref.tile_costs(np.ones((11, 19), np.uint32), p)
    assert cost.tolist() == [64, 64, 24, 24, 24, 9, 0, 0]
    pb = rtow.make_params(19, 11, 4, world=2, rank=1, row_block=4)
    assert (pb.local_rows, pb.band_stride, pb.band_offset) == (8, 2, 1)
    assert sched_ref.tile_costs(np.ones((8, 19), np.uint32), pb).tolist() == [32, 32, 12, 0]


def test_block_order_on_hand_made_costs():
    """A permutation, non-increasing in block cost, ties in ascending block
    index, each block's units adjacent and ascending."""
    tile = np.array([[1, 1, 1, 1], [0, 0, 0, 9], [4, 0, 0, 0], [2, 2, 0, 0], [0, 0, 0, 0], [9, 0, 0, 0],
                     [2 ** 30 - 1] * 4, [1, 0, 2, 1]], np.uint32).reshape(-1)
    assert sched_ref.block_costs(tile).tolist() == [4, 9, 4, 4, 0, 9, 2 ** 32 - 4, 4]
    assert sched_ref.block_order(tile, 1).tolist() == [6, 1, 5, 0, 2, 3, 7, 4]
    rng = np.random.default_rng(7)
    for blocks, units, hi in ((1, 1, 5), (2, 3, 2), (257, 2, 4), (1000, 8, 2 ** 30)):
        tile = rng.integers(0, hi, blocks * 4, dtype=np.uint32)
        cost = sched_ref.block_costs(tile)
        order = sched_ref.block_order(tile, units).astype(np.int64)
        assert sorted(order.tolist()) == list(range(blocks * units))
        grouped = order.reshape(blocks, units)
        assert np.array_equal(grouped % units, np.tile(np.arange(units), (blocks, 1)))
        by_cost = grouped[:, 0] // units
        assert np.array_equal(grouped // units, np.repeat(by_cost[:, None], units, axis=1))
        c = cost[by_cost]
        assert (np.diff(c) <= 0).all()
        assert (np.diff(by_cost)[np.diff(c) == 0] > 0).all()


@pytest.mark.parametrize("name", sorted(sched_cases.CASES))
def test_gpu_cases_can_tell_a_wrong_schedule(rtow, name):
    """Non-vacuity of test_sched_gpu.py's cases, from the oracle alone: the
    reference order is not launch order (a pilot that stores zeros, whose
    stable sort gives launch order, cannot pass), it is not the ascending
    order either, and the blocks take at least 8 distinct costs."""
    cost = sched_cases.ref_costs(rtow, name)
    _, _, p = sched_cases.case(rtow, name)
    blocks = sched_ref.frame_blocks(p)
    assert cost.shape == (blocks * 4,) and blocks == rtow.frame_blocks(p) > 1
    bc = sched_ref.block_costs(cost)
    assert len(set(bc.tolist())) >= 8, sorted(set(bc.tolist()))
    order = sched_ref.block_order(cost, 1)
    assert not np.array_equal(order, np.arange(blocks))
    assert not np.array_equal(order, np.argsort(bc, kind="stable"))
    # a partial frame's padding tiles cost nothing; every tile inside costs something
    tiles = -(-p.width // 8) * -(-p.local_rows // 8)
    assert not cost[tiles:].any()


def test_the_cache_cases_have_different_orders(rtow):
    """test_sched_gpu.py's cache test reuses one context across cameras and
    scenes at one frame size (equal block counts): a stale order shows only
    if the references differ -- camera A / camera B, final / five-sphere
    scene -- and an order that ignored the seed or spp only if those of A
    with another seed and spp differ from A's first, which must stay."""
    a = sched_ref.block_order(sched_cases.ref_costs(rtow, "final_67x37"), 1)
    b = sched_ref.block_order(sched_cases.ref_costs(rtow, "final_67x37_cam_b"), 1)
    five = sched_ref.block_order(sched_cases.ref_costs(rtow, "five_67x37"), 1)
    assert a.shape == b.shape == five.shape
    assert not np.array_equal(a, b) and not np.array_equal(a, five) and not np.array_equal(b, five)
    a2 = sched_ref.block_order(sched_cases.ref_costs(rtow, "final_67x37", seed=99, spp=3), 1)
    assert not np.array_equal(a, a2)


def test_the_pilot_samples_of_the_cases(rtow):
    """The spp = 2 cases' costs are those of 2 samples, not 4."""
    for name in ("final_67x37", "final_320x120"):
        _, _, p2 = sched_cases.case(rtow, name + "_spp2")
        assert p2.spp == 2
        c4 = sched_cases.ref_costs(rtow, name + "_spp2", spp=5)
        c2 = sched_cases.ref_costs(rtow, name + "_spp2")
        inside = c4 > 0
        assert (c2[inside] < c4[inside]).all() and not c2[~inside].any()  # (the tile costs are compared exactly)
