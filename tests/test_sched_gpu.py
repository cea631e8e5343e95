"""The pilot schedule (RT_FLAG_PILOT_SCHEDULE) on the device,
entry for entry against tests/sched_ref.py: the sort kernel on synthetic costs,
the pilot's tile costs against the oracle's per-pixel segment counts, the
order a render's launches read, the per-geometry cache and its clear on a scene
upload, and renders split into sample ranges and strided entry ranges.  Every
comparison is integer array equality.  tests/test_sched.py shows on the CPU
that the cases used here tell a right schedule from a wrong one."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib
import sched_cases
import sched_ref

pytestmark = pytest.mark.gpu

TILE_MAX = 2 ** 30 - 1  # tile costs stay below 2^30: a block's sum cannot wrap


@pytest.fixture(scope="module")
def ctx(rtow):
    """A context of this module's own (no option another module set)."""
    if rtow.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests need an MI355X")
    with rtow.Context(0) as c:
        yield c


# ------------------------------------------------------ a. the sort alone ----

def _split(sums, rng, how):
    """Tile costs (uint32 [blocks * 4], each <= TILE_MAX) whose blocks sum to
    `sums`: even quarters, then (how = "random") a random amount moved from
    each block's tile 0 to its tile 1 and from 2 to 3, or (how = "rotate")
    block b in the b % 4-th of four fixed shapes."""
    sums = np.asarray(sums, np.int64)
    assert sums.min(initial=0) >= 0 and sums.max(initial=0) <= 4 * TILE_MAX
    t = np.repeat(sums[:, None] // 4, 4, axis=1)
    t += np.arange(4)[None, :] < (sums % 4)[:, None]
    if how == "rotate":
        shape = np.arange(len(sums)) % 4
        small = sums <= TILE_MAX
        for k, tile in ((1, 0), (2, 3)):  # everything in tile 0 / in tile 3 (3: the even split stays)
            m = small & (shape == k)
            t[m] = 0
            t[m, tile] = sums[m]
        m = small & (shape == 0) & (sums > 0)  # 1 in tile 1, the rest in tile 2
        t[m] = 0
        t[m, 1] = 1
        t[m, 2] = sums[m] - 1
    else:
        for a, b in ((0, 1), (2, 3)):
            d = (rng.random(len(sums)) * (np.minimum(t[:, a], TILE_MAX - t[:, b]) + 1)).astype(np.int64)
            d = np.minimum(d, np.minimum(t[:, a], TILE_MAX - t[:, b]))
            t[:, a] -= d
            t[:, b] += d
    assert (t >= 0).all() and (t <= TILE_MAX).all() and np.array_equal(t.sum(axis=1), sums)
    return t.reshape(-1).astype(np.uint32)


def _pattern(name, blocks):
    rng = np.random.default_rng([blocks, sorted(PATTERNS).index(name)])
    if name == "equal":  # stability: the result is launch order
        return np.full(blocks * 4, 7, np.uint32)
    if name == "distinct":  # all distinct, over the whole 32-bit range
        return _split(rng.permutation(blocks).astype(np.int64) * ((4 * TILE_MAX) // blocks), rng, "random")
    if name == "four_values":  # long tie runs
        return _split(rng.choice(np.array([3, 17, 68, 100000], np.int64), blocks), rng, "random")
    if name == "zeros":  # blocks that cost nothing among cheap ones
        return _split(rng.integers(1, 50, blocks) * rng.integers(0, 2, blocks), rng, "random")
    if name == "bit31":  # sums on both sides of 2^31, a few equal: an unsigned sort over all 32 bits
        hi = rng.integers(0, 2, blocks).astype(bool)
        s = np.where(hi, 2 ** 31 + rng.integers(0, 9, blocks) * (2 ** 27), rng.integers(0, 9, blocks) * (2 ** 27) + 5)
        return _split(s, rng, "random")
    if name == "equal_sums_other_splits":  # ties between blocks whose tiles differ
        return _split(rng.choice(np.array([100, 200, 201], np.int64), blocks), rng, "rotate")
    raise KeyError(name)


PATTERNS = ("equal", "distinct", "four_values", "zeros", "bit31", "equal_sums_other_splits")
BLOCKS = (1, 2, 255, 256, 257, 4097, 131073)  # the 256-thread tails, one and several sort tiles, a C4 rank share


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("blocks", BLOCKS)
def test_sort_kernel_equals_the_reference(rtow, blocks, pattern):
    tile = _pattern(pattern, blocks)
    cost = sched_ref.block_costs(tile)
    if pattern == "bit31" and blocks > 8:
        assert (cost >= 2 ** 31).any() and (cost < 2 ** 31).any()
    if pattern not in ("equal", "distinct") and blocks > 255:
        assert len(set(cost.tolist())) < blocks  # ties
    if pattern == "distinct":
        assert len(set(cost.tolist())) == blocks
    for units in (1, 2, 3, 8):
        want = sched_ref.block_order(tile, units)
        if pattern == "equal":
            assert np.array_equal(want, np.arange(blocks * units))
        got = rtow.block_order_host(tile, blocks, units)
        assert got.dtype == np.uint32 and np.array_equal(got, want), \
            (units, int((got != want).sum()), np.flatnonzero(got != want)[:4])


def test_sort_of_nothing_writes_nothing(rtow):
    L = rtow.lib()
    L.rt_internal_block_order_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_void_p]
    tile = np.full(32, 5, np.uint32)
    for blocks, units in ((0, 3), (8, 0), (0, 0)):
        order = np.full(64, 0xDEADBEEF, np.uint32)
        assert L.rt_internal_block_order_host(0, tile.ctypes.data, blocks, units, order.ctypes.data) == 0
        assert (order == 0xDEADBEEF).all() and (tile == 5).all()


# ------------------------------------- b. the pilot's tile costs, c. orders ----

@functools.lru_cache(maxsize=None)
def _oracle_image(rtow, name, **override):
    scene, cam, p = sched_cases.case(rtow, name, **override)
    img, segs = oracle_lib.kernel_render(scene, cam, p)
    img.setflags(write=False)
    return img, segs


def _planned_units(rtow, p, budget=0.0):
    return rtow.launch_plan(p, budget)["units"]


@pytest.mark.parametrize("units", [1, 3])
@pytest.mark.parametrize("name", ["final_67x37", "final_320x120", "final_67x37_spp2", "final_320x120_spp2",
                                  "five_64x36", "band_131x85"])
def test_pilot_tile_costs_equal_the_oracles(rtow, ctx, name, units):
    """Every tile's pilot cost is the oracle's segment count of its pixels'
    first min(spp, 4) samples, whatever units the render itself uses; the
    order the render then read is the reference's for those costs."""
    scene, cam, p = sched_cases.case(rtow, name, units=units)
    want = sched_cases.ref_costs(rtow, name, units=units)
    ctx.upload(scene)  # (drops any cached order)
    r = ctx.pilot_schedule(cam, p)
    assert r["pilot_ran"]
    got = r["tile_cost"]
    assert got.shape == want.shape
    assert np.array_equal(got, want), (int((got != want).sum()), np.flatnonzero(got != want)[:8])
    planned = _planned_units(rtow, p)
    assert planned == min(units, p.spp)
    assert np.array_equal(r["order"], sched_ref.block_order(want, planned))


@pytest.mark.parametrize("units", [1, 3, 0])
def test_order_a_render_used(rtow, ctx, units):
    """After an ordinary render with the flag, the context's order is the
    reference's for the planned units (0: automatic, 8 waves per tile on so
    small a frame), and the image is still the oracle's."""
    scene, cam, p = sched_cases.case(rtow, "final_67x37", spp=9, units=units)
    planned = _planned_units(rtow, p)
    assert planned == {1: 1, 3: 3, 0: 8}[units]
    ctx.upload(scene)
    assert ctx.block_order().size == 0  # an upload leaves no valid order
    got, st = ctx.render(cam, p)
    want, segs = _oracle_image(rtow, "final_67x37", spp=9)
    assert np.array_equal(got, want) and st.segments == segs
    order = ctx.block_order()
    assert np.array_equal(order, sched_ref.block_order(sched_cases.ref_costs(rtow, "final_67x37", spp=9), planned))


# ---------------------------------------------------------- d. the cache ----

def test_order_cache_per_geometry_and_scene(rtow):
    """One context: the cached order is reused exactly for the geometry it was
    made for (the key leaves seed and spp out on purpose), another camera gets
    its own, a scene upload drops it, and renders enqueued on two streams each
    read their own."""
    import torch
    A, B, FIVE = "final_67x37", "final_67x37_cam_b", "five_67x37"

    def ref(name, **kw):
        return sched_ref.block_order(sched_cases.ref_costs(rtow, name, units=1, **kw), 1)

    def shown(c, name, ran, want_order, **kw):
        _, cam, p = sched_cases.case(rtow, name, units=1, **kw)
        r = c.pilot_schedule(cam, p)
        assert r["pilot_ran"] == ran, name
        assert np.array_equal(r["order"], want_order), name
        assert np.array_equal(r["image"], _oracle_image(rtow, name, **kw)[0]), name
        return r["order"]

    with rtow.Context(0) as c:
        c.upload(sched_cases.scene(rtow, "final"))
        first = shown(c, A, True, ref(A))
        # the same geometry with another seed and spp: the cached order, byte for byte
        again = shown(c, A, False, first, seed=99, spp=3)
        assert again.tobytes() == first.tobytes()
        shown(c, B, True, ref(B))
        shown(c, A, True, ref(A))
        # another scene, same camera and frame (equal block count), and back
        c.upload(sched_cases.scene(rtow, "five"))
        shown(c, FIVE, True, ref(FIVE))
        c.upload(sched_cases.scene(rtow, "final"))
        shown(c, A, True, ref(A))

        # render_async on two streams, A and B alternating
        dev = torch.device("cuda", 0)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        _, cam_a, pa = sched_cases.case(rtow, A, units=1)
        _, cam_b, pb = sched_cases.case(rtow, B, units=1)
        ta = torch.zeros((pa.local_rows, pa.width, 3), dtype=torch.float32, device=dev)
        tb = torch.zeros_like(ta)
        torch.cuda.synchronize(dev)
        for _ in range(2):
            c.render_async(cam_a, pa, ta.data_ptr(), s1.cuda_stream)
            c.render_async(cam_b, pb, tb.data_ptr(), s2.cuda_stream)
        torch.cuda.synchronize(dev)
        assert np.array_equal(c.block_order(), ref(B))
        assert np.array_equal(ta.cpu().numpy(), _oracle_image(rtow, A)[0])
        assert np.array_equal(tb.cpu().numpy(), _oracle_image(rtow, B)[0])
        c.render_async(cam_a, pa, ta.data_ptr(), s1.cuda_stream)
        torch.cuda.synchronize(dev)
        assert np.array_equal(c.block_order(), ref(A))
        assert np.array_equal(ta.cpu().numpy(), _oracle_image(rtow, A)[0])


# ------------------------------- e. sample ranges, strided entry ranges ----

@pytest.mark.parametrize("spp,budget,ranges,chunks", [
    (50, sched_cases.SPLIT_BUDGET, 5, 1),   # 5 strided entry ranges of all 50 samples
    (400, 320 * 180 * 100, 1, 4),           # 4 sample ranges of 100 spp over every entry
])
def test_split_renders_keep_the_order(rtow, spp, budget, ranges, chunks):
    name = "final_320x180"
    scene, cam, p = sched_cases.case(rtow, name, spp=spp)
    plan = rtow.launch_plan(p, budget)
    assert (plan["ranges"], plan["chunks"], plan["units"]) == (ranges, chunks, 1)
    want = sched_ref.block_order(sched_cases.ref_costs(rtow, name, spp=spp), 1)
    with rtow.Context(0) as c:
        c.upload(scene)
        whole, st0 = c.render(cam, p)
        assert st0.launches == 1 and np.array_equal(c.block_order(), want)
        c.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, budget)
        c.upload(scene)  # (a fresh pilot for the split render)
        split, st = c.render(cam, p)
        assert st.launches == ranges * chunks
        assert np.array_equal(c.block_order(), want)
        assert np.array_equal(split, whole) and st.segments == st0.segments
