"""rt_aov, rt_guides and rt_route against the chain oracle, byte for byte, on
the GPU.  The three passes carry their own restatement of the render's hit
block and of its metal and dielectric blocks (csrc/rt_trace_pass.h,
rt_chain.h); the oracle's records come from the step function the render
restatement runs on (oracle/rt_oracle.cc kernel_step, rto_kernel_terminals),
and tests/features_ref.py restates the sums and the vote in float32.  The
headers fix every output to the bit, so every comparison here is tobytes()
equality: no tolerance, no masked pixel.

The cases are tests/features_cases.py's; test_features_oracle.py shows on the
CPU that they meet refractions, Schlick reflections, total internal
reflection, both arms of the spurious-root rule, absorbed and fuzzy metals,
negative radii, the bounce cap, the 2^100 clamp, chains of four and more
bounces, escaped chains and pixels whose route candidate changed."""
import numpy as np
import pytest

import features_cases as fc
import features_ref
import route_ref

pytestmark = pytest.mark.gpu

ALL = features_ref.ROUTE + ("state",)


@pytest.fixture
def ctx(rtow, gpu_ctx):
    """The session's context with its options at their defaults afterwards."""
    yield gpu_ctx
    gpu_ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_PLACEMENT, 0)
    gpu_ctx.set_option(rtow.RT_OPT_GRID_SCALE, 0)


@pytest.fixture(scope="module", params=list(fc.CASES))
def case(request):
    """Module-scoped, so that pytest runs the three passes' tests of one case
    next to each other: they share that case's oracle records
    (features_cases.terminals keeps one case's at a time)."""
    return request.param


def _setup(rtow, ctx, case):
    """Upload the case's scene and set its launch split; yields (frame, camera, params)."""
    ctx.upload(fc.scene_of(rtow, case))
    out = []
    for frame in fc.frames_of(case):
        p = fc.params_of(rtow, case, frame)
        if "launch" in fc.CASES[case]:  # RT_OPT_LAUNCH_SAMPLES counts samples of the whole frame
            ctx.set_option(rtow.RT_OPT_LAUNCH_SAMPLES, p.width * p.local_rows * fc.CASES[case]["launch"])
            assert p.spp > fc.CASES[case]["launch"]  # several launches
        out.append((frame, fc.camera_of(rtow, case, frame), p))
    return out


def _check(got, want, names, term, what, restate=features_ref.sums):
    """want = restate(term), by name; byte equality, the message by first_difference."""
    for n in names:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (what, n)
        if got[n].tobytes() != want[n].tobytes():
            pytest.fail("%s: %s" % (what, features_ref.first_difference(term, n, got[n], want[n], restate)))


def test_aov_is_the_oracles(rtow, ctx, case):
    """rt_aov's six buffers are the sums of the oracle's first-hit records in
    rt_aov's own form of a primary skip (keep_dir), padding rows included."""
    for frame, cam, p in _setup(rtow, ctx, case):
        term = fc.terminals(rtow, case, frame, -1, 0.0, keep_dir=True)
        _check(ctx.aov(cam, p), features_ref.sums(term), features_ref.AOV, term, "%s %s rt_aov" % (case, frame))


def test_guides_are_the_oracles(rtow, ctx, case):
    """rt_guides' eight buffers, with nothing followed, 1, 2, the default 8
    and 64 bounces, and with max_fuzz 0, 0.3 and 1."""
    for frame, cam, p in _setup(rtow, ctx, case):
        for mb in fc.GUIDES_BOUNCES:
            for mf in fc.GUIDES_FUZZ:
                term = fc.terminals(rtow, case, frame, mb, mf)
                # Context.guides: 0 follows nothing (the struct's -1), None is the default
                got = ctx.guides(cam, p, max_bounces={-1: 0, fc.DEFAULT_BOUNCES: None}.get(mb, mb), max_fuzz=mf)
                _check(got, features_ref.sums(term), features_ref.GUIDES, term,
                       "%s %s rt_guides max_bounces %d max_fuzz %g" % (case, frame, mb, mf))


def test_route_is_the_oracles(rtow, ctx, case):
    """rt_route's final state is the restated vote and sums over the oracle's
    records, and its eight outputs are the restated finalize of that state, at
    the default 8 bounces and at 2.  The vote of route_ref.select on the
    oracle's keys gives the state's key, votes, n and hits."""
    for frame, cam, p in _setup(rtow, ctx, case):
        for mb in fc.ROUTE_BOUNCES:
            term = fc.terminals(rtow, case, frame, mb, 0.0)
            state = features_ref.route_state(term)
            what = "%s %s rt_route max_bounces %d" % (case, frame, mb)
            got = ctx.route(cam, p, which=ALL, max_bounces=None if mb == fc.DEFAULT_BOUNCES else mb)
            st = route_ref.split_state(state)
            if p.spp:
                sel = route_ref.select(np.moveaxis(features_ref.route_keys(term), -1, 0),
                                       np.moveaxis(term["sphere"] >= 0, -1, 0))
                for n in ("key", "votes", "n", "hits"):
                    assert np.array_equal(st[n], sel[n]), (what, n)
            gs = route_ref.split_state(got["state"])
            _check(gs, st, ("key", "votes", "n", "hits", "id", "pad", "depth", "position", "normal", "albedo"), term,
                   what + " state", features_ref.route_fields)
            assert got["state"].tobytes() == state.tobytes(), what
            _check(got, route_ref.finalize(state), features_ref.ROUTE, term, what, features_ref.route_outputs)
