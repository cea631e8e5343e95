"""What the pilot schedule (RT_FLAG_PILOT_SCHEDULE) is specified
to be, restated in numpy on integers (test infrastructure): the pilot's tile
costs from the oracle's per-pixel segment counts, and the launch order from
tile costs.  tests/test_sched_gpu.py compares the device's with these, entry
for entry; tests/test_sched.py checks them, and the cases, on the CPU.

The frame's layout, as the render kernel reads it (csrc/rt_kernel.hip at the
block_order lookup, csrc/rt_layout.h): the local frame (local_rows x width) is
cut into 8 x 8 tiles, tile t = ty * tiles_x + tx with tiles_x = ceil(width /
8), covering local rows 8 ty .. 8 ty + 7 and columns 8 tx .. 8 tx + 7; one wave
traces a tile, block b's four waves the tiles 4 b .. 4 b + 3.  Local row l
lies in band l // row_block and is the frame's row (band * band_stride +
band_offset) * row_block + l % row_block; a lane whose row is past local_rows
or past the frame's height, or whose column is past its width, traces nothing.
"""
import numpy as np

TILE = 8    # rtk::kTile
WAVES = 4   # rtk::kWavesPerBlock: tiles per block
PILOT_SPP = 4  # the pilot traces samples [0, min(spp, 4)) of every pixel, in one unit


def frame_blocks(params):
    tiles = -(-params.width // TILE) * -(-params.local_rows // TILE)
    return -(-tiles // WAVES)


def tile_costs(seg, params):
    """The pilot's tile_cost array, uint32 [blocks * 4]: seg is the oracle's
    (local_rows, W) segment counts of each pixel's first min(spp, 4) samples
    (oracle_lib.kernel_pixel_segments); tile t's sum stands at t = block * 4 +
    wave in launch order; lanes past the frame or the local rows add 0, and so
    do the padding tiles up to blocks * 4."""
    seg = np.asarray(seg)
    W, rows = int(params.width), int(params.local_rows)
    assert seg.shape == (rows, W) and np.issubdtype(seg.dtype, np.integer), (seg.shape, seg.dtype)
    tx, ty = -(-W // TILE), -(-rows // TILE)
    lrow = np.arange(ty * TILE)
    band = lrow // params.row_block
    grow = (band * params.band_stride + params.band_offset) * params.row_block + (lrow - band * params.row_block)
    row_in = (lrow < rows) & (grow < params.height)
    px = np.zeros((ty * TILE, tx * TILE), np.int64)
    px[:rows, :W] = seg
    px[~row_in, :] = 0
    tiles = px.reshape(ty, TILE, tx, TILE).sum(axis=(1, 3)).reshape(-1)
    assert tiles.max(initial=0) < 2 ** 32
    out = np.zeros(frame_blocks(params) * WAVES, np.uint32)
    out[:tiles.size] = tiles
    return out


def block_costs(tile_cost):
    """A block's cost: the sum of its four tiles' (int64; the device's wraps at
    2^32, which the tests keep away from)."""
    cost = np.asarray(tile_cost).astype(np.int64).reshape(-1, WAVES).sum(axis=1)
    assert cost.max(initial=0) < 2 ** 32, "a wrapped block sum is not specified"
    return cost


def block_order(tile_cost, units):
    """The launch order, uint32 [blocks * units]: blocks by decreasing cost,
    equal costs in increasing block index (a stable sort), and
    order[i * units + u] = sorted[i] * units + u."""
    cost = block_costs(tile_cost)
    by_cost = np.argsort(-cost.astype(np.int64), kind="stable")
    order = by_cost[:, None] * int(units) + np.arange(int(units))[None, :]
    assert order.max(initial=0) < 2 ** 32
    return order.reshape(-1).astype(np.uint32)
