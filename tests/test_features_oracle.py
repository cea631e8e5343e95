"""The chain oracle judged on the CPU (oracle/rt_oracle.cc rto_kernel_terminals,
tests/features_ref.py): before it judges rt_aov, rt_guides and rt_route on the
GPU (test_features_oracle_gpu.py), its routing is checked against the render
restatement it shares its step with, its one-bounce geometry against fp64, its
throughput against the albedos on the path, its two forms of a primary skip
against each other, and its invariants; and the GPU file's case list is shown
to meet every situation the byte comparison is there for."""
import numpy as np
import pytest

import features_cases as fc
import features_ref
import oracle_lib
import route_ref
from mirror_room import left_out64, mirror_room, mirror_room_camera, roots64, second_hop64

W, H = fc.FRAMES[0]
EV = oracle_lib.EVENTS


def _ev(term, name):
    return (term["events"] & EV[name]) != 0


def _continues(rtow, scene, max_fuzz):
    return (scene.kind == rtow.RT_DIELECTRIC) | ((scene.kind == rtow.RT_METAL) &
                                                  (np.minimum(scene.param, np.float32(1.0)) <= np.float32(max_fuzz)))


# ---- 1. routing against the render restatement ------------------------------
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("max_fuzz", [0.0, 0.3])
@pytest.mark.parametrize("scene_name", ["final", "five"])
def test_routing_is_the_render_restatements(rtow, scene_name, max_fuzz, flags):
    """test_guides_routing_is_the_renders' black-terminal twin: every sphere that
    cannot continue a chain gets albedo 0.  At spp 1 and max_depth = B + 1 the
    render restatement of the twin is > 0 exactly where the chain's primary ray
    missed or the chain escaped within B bounces."""
    scene = rtow.final_scene() if scene_name == "final" else rtow.five_scene()
    go_on = _continues(rtow, scene, max_fuzz)
    assert go_on.any() and (~go_on).any()
    twin = rtow.Scene(scene.cx.copy(), scene.cy.copy(), scene.cz.copy(), scene.radius.copy(), scene.kind.copy(),
                      np.where(go_on[:, None], scene.albedo, np.float32(0.0)).astype(np.float32), scene.param.copy())
    bounces = (0, 1, 2, 5)
    # the darkest escaping sample: the smallest tint on the chain, B times, under the darkest sky (0.5)
    tint = float(np.where((scene.kind == rtow.RT_DIELECTRIC)[:, None], 1.0, scene.albedo)[go_on].min())
    assert tint ** max(bounces) * 0.5 > 1024 * 2.0 ** -31
    view = fc.FIVE_VIEW if scene_name == "five" else dict(focus_dist=10.0)
    cam = rtow.camera_cpu(aspect=W / H, aperture=0.1, **view)
    for B in bounces:
        p = rtow.make_params(W, H, 1, max_depth=B + 1, seed=1 + B, flags=flags)
        img, _ = oracle_lib.kernel_render(twin, cam, p)
        lit = (img > 0).all(-1)
        assert np.array_equal(lit, (img > 0).any(-1))
        t = oracle_lib.kernel_terminals(scene, cam, p, B if B else -1, max_fuzz)[..., 0]
        want = (t["sphere"] < 0) | (t["escaped"] == 1)
        assert np.array_equal(lit, want), (B, int((lit != want).sum()))
        assert np.all(t["bounces"] <= B)
        if B >= 2:
            assert (t["escaped"] == 1).any() and (t["bounces"] >= 2).any()


# ---- 2. one-bounce geometry against fp64 -------------------------------------
def test_one_bounce_geometry_against_fp64(rtow):
    """test_guides_one_bounce_geometry_against_fp64 on the oracle's records:
    mirror room, spp 1, pinhole.  The first-hit records give M and N_M; in
    fp64 the reflected ray's nearest root past t_min is the expected id, P, N
    and depth.  The tolerance is that test's: the kernel arithmetic's largest
    deviation from fp64 times 8, times 1 + 2 t / |r_mirror|, floored at 4 ulp32
    of the largest coordinate; rays with two offers or a limb within it are
    left out, at most 1 %.  There is no device here to run rt_device_kat on, so
    the deviation is taken where the same arithmetic can be had: the oracle's
    first-hit t, P and N against fp64 on the first hop's rays, and it is
    asserted to stay within the deviation recorded for the device (4.17e-6), so
    that a bad first hit cannot widen the tolerance it is judged by."""
    scene = mirror_room(rtow)
    cam = mirror_room_camera(rtow, W, H)
    p = rtow.make_params(W, H, 1, seed=3)
    f8 = np.float64
    a = oracle_lib.kernel_terminals(scene, cam, p, -1)[..., 0]
    g = oracle_lib.kernel_terminals(scene, cam, p, 8)[..., 0]
    one = (g["bounces"] == 1) & (g["escaped"] == 0) & (a["sphere"] == 0)
    assert one.sum() >= 40
    eye = np.array(cam.eye[:], f8)
    C = np.stack([scene.cx, scene.cy, scene.cz], -1).astype(f8)
    R = scene.radius.astype(f8)
    M, NM = a["P"][one].astype(f8), a["N"][one].astype(f8)
    offer, r, limb = second_hop64(eye, M, NM, C, R)
    want_id = np.argmin(offer, -1)
    t64 = offer.min(-1)
    tq = np.where(np.isfinite(t64), t64, 0.0)
    P64 = M + tq[:, None] * r
    c, rad = C[want_id], R[want_id]
    N64 = (P64 - c) / rad[:, None]
    N64 *= np.where((N64 * r).sum(-1) > 0, -1.0, 1.0)[:, None]
    first = np.linalg.norm(M - eye, axis=-1)
    d1 = (M - eye) / first[:, None]
    t0, _ = roots64(np.broadcast_to(eye, d1.shape), d1, np.broadcast_to(C[0], d1.shape), np.full(len(d1), R[0]))
    p1 = eye + t0[:, None] * d1
    dev = max(np.abs(a["depth"][one] - t0).max(), np.abs(M - p1).max(), np.abs(NM - (p1 - C[0]) / R[0]).max())
    # dev comes from the code under test, so it may not relax the tolerance: it has to stay within the figure
    # the GPU test records for the device's own sphere arithmetic on these cases (4.17e-6)
    assert dev <= 4.17e-6, dev
    biggest = max(np.abs(C).max(), np.abs(R).max(), np.abs(eye).max(), np.abs(g["P"][one]).max())
    ulp = float(np.spacing(np.float32(biggest)))
    tol = np.maximum(8.0 * dev * (1.0 + 2.0 * tq / abs(R[0])), 4.0 * ulp)
    out = left_out64(offer, limb, tol)
    assert out.mean() <= 0.01
    k = ~out
    P, N, dep = g["P"][one].astype(f8), g["N"][one].astype(f8), g["depth"][one].astype(f8)
    ep, en, ed = np.abs(P - P64).max(-1), np.abs(N - N64).max(-1), np.abs(dep - (first + tq))
    print("oracle mirror room: %d one-bounce pixels, %d left out; deviation %.3e, tol %.3e .. %.3e; measured P %.3e, "
          "N %.3e, depth %.3e" % (len(tq), int(out.sum()), dev, tol.min(), tol.max(), ep[k].max(), en[k].max(),
                                  ed[k].max()))
    assert np.array_equal(g["sphere"][one][k], want_id[k])
    assert np.all(ep[k] <= tol[k]) and np.all(ed[k] <= tol[k]) and np.all(en[k] <= tol[k])
    gn = (P - c) / rad[:, None]
    assert np.all(np.abs(N - gn).max(-1)[k] <= tol[k]) and np.all((N * r).sum(-1)[k] < 0)


# ---- 3. throughput ------------------------------------------------------------
@pytest.mark.parametrize("case", ["final-lens", "five-pinhole", "hot-gpusem", "free12-gpusem"])
def test_throughput_is_the_product_of_the_albedos(rtow, case):
    """thr of a chain of at most 3 counted hits is the float32 product, in path
    order from 1, of the albedos on its trail (a dielectric's is 1)."""
    scene = fc.scene_of(rtow, case)
    term, trail = oracle_lib.kernel_terminals(scene, fc.camera_of(rtow, case, (W, H)), fc.params_of(rtow, case, (W, H)),
                                              8, 0.3, trail=True)
    alb = np.where((scene.kind == rtow.RT_DIELECTRIC)[:, None], np.float32(1.0), scene.albedo).astype(np.float32)
    short = (term["sphere"] >= 0) & (trail[..., 3] < 0)
    n_hits = (trail >= 0).sum(-1)
    assert short.sum() >= 1000 and (n_hits[short] == 3).sum() >= 20 and (n_hits[short] == 2).any()
    thr = np.ones(term.shape + (3,), np.float32)
    for j in range(3):
        thr = np.where((trail[..., j] >= 0)[..., None], thr * alb[np.maximum(trail[..., j], 0)], thr)
    assert thr.dtype == np.float32 and thr[short].tobytes() == term["thr"][short].tobytes()
    # the terminal is the trail's last sphere
    last = np.take_along_axis(trail, np.maximum(n_hits - 1, 0)[..., None], -1)[..., 0]
    assert np.array_equal(last[short], term["sphere"][short])


# ---- 4. the two forms of a primary skip ---------------------------------------
def test_first_hit_records_do_not_depend_on_the_skip_form(rtow):
    """max_bounces = -1: rt_aov's form (keep_dir) and rt_guides' give identical
    records wherever the sample had no first-arm skip."""
    n_skip = n = 0
    for case in fc.CASES:
        for frame in fc.frames_of(case):
            a = fc.terminals(rtow, case, frame, -1, 0.0, keep_dir=True)
            b = fc.terminals(rtow, case, frame, -1, 0.0)
            skip = _ev(a, "skip_tmin") | _ev(b, "skip_tmin")
            assert a[~skip].tobytes() == b[~skip].tobytes(), (case, frame)
            assert not a["bounces"].any() and not a["escaped"].any()
            n_skip += int(skip.sum())
            n += a.size
    print("first-hit records: %d samples, %d with a first-arm skip of the primary ray" % (n, n_skip))


# ---- 5. invariants ------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in fc.CASES if fc.CASES[c]["spp"]])
def test_invariants(rtow, case):
    """bounces <= max_bounces; escaped only on a hit sample, and only after a
    bounce; depth with bounces followed >= the first hit's; and the normal's
    length.

    "Within a few ulp of 1" cannot hold for correct arithmetic (the largest
    ||N| - 1| over the cases is 6.1e-3, on the contact scene), and why gives the
    bound.  The candidate test is the expanded quadratic e = h^2 - g - ks >= 0
    in world coordinates, with h = C.D - O.D and g = |O|^2 - 2 C.O.  With Q =
    (|C| + |O|)^2, in units of 2^-23 Q its roundings add up to at most 6 (h^2,
    from 3 ulp of h), 1.5 (|O|^2), 1.5 (g's three fma), 0.5 (the fma of h^2 -
    g), 0.5 (- ks) and 0.5 (ks itself): 10.5.  So a ray that passes the
    sphere at a distance f with f^2 - r^2 up to 11 * 2^-23 Q is still a
    candidate; its refined discriminant is negative and is held at 2^-96, so P
    is the ray's closest point to C: |P - C| = f, and |N| - 1 = f / |r| - 1 <=
    5.5 * 2^-23 Q / r^2.  That is the 6.1e-3: a camera ray 11.75 long grazing
    a ball of r = 0.05 (Q = 250: the term allows 6.6e-2).  Beside that term, P =
    fma(t, d, o) is off the sphere by a few ulp32 of t (the refined root's
    error) and of its own coordinates, and N = (P - C) * RN(1 / r) adds three
    roundings:
        ||N| - 1| <= 6 * 2^-23 Q / r^2 + 8 * 2^-23 max(|P|, |C|, |r|, t) / |r| + 4 * 2^-24.
    The record has no O and no t; |O| <= min(|P| + depth, the scene's extent
    as seen from the origin, the eye included) and t <= depth stand in for
    them, which only widens the bound.  The worst ratio to it is printed.
    Beside it, |N| is |P - C| / |r| of the record's own P within 4 * 2^-24
    relative (the three roundings alone)."""
    scene = fc.scene_of(rtow, case)
    f8 = np.float64
    C_all = np.stack([scene.cx, scene.cy, scene.cz], -1).astype(f8)
    R_all = np.abs(scene.radius.astype(f8))
    worst = 0.0
    for frame in fc.frames_of(case):
        eye = np.array(fc.camera_of(rtow, case, frame).eye[:], f8)
        extent = max((np.linalg.norm(C_all, axis=-1) + R_all).max(), np.linalg.norm(eye) + 0.1)  # 0.1: the lens
        first = fc.terminals(rtow, case, frame, -1, 0.0)
        for B in (-1, 1, 2, 8, 64):
            t = fc.terminals(rtow, case, frame, B, 0.3)
            hit = t["sphere"] >= 0
            assert np.array_equal(hit, first["sphere"] >= 0)
            assert np.all(t["bounces"] <= max(B, 0)) and np.all(t["escaped"] <= hit)
            assert np.all(t["bounces"][t["escaped"] == 1] >= 1)
            assert np.all(t["depth"][hit] >= first["depth"][hit])
            assert not t["depth"][~hit].any() and not t["P"][~hit].any() and not t["thr"][~hit].any()
            i = np.maximum(t["sphere"], 0)
            c, r = C_all[i], R_all[i]
            P, depth = t["P"].astype(f8), t["depth"].astype(f8)
            n_len = np.linalg.norm(t["N"].astype(f8), axis=-1)
            want = np.where(hit, np.linalg.norm(P - c, axis=-1) / r, 1.0)
            assert np.all(np.abs(n_len / want - 1.0)[hit] <= 4 * 2.0 ** -24), (B, frame)
            lc, lp = np.linalg.norm(c, axis=-1), np.linalg.norm(P, axis=-1)
            Q = (lc + np.minimum(lp + depth, extent)) ** 2
            bound = (6 * 2.0 ** -23 * Q / r ** 2 + 8 * 2.0 ** -23 * np.maximum.reduce([lp, lc, r, depth]) / r +
                     4 * 2.0 ** -24)
            ratio = (np.abs(n_len - 1.0) / bound)[hit]
            if ratio.size:
                worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1.0), (B, frame, float(ratio.max()))
    print("normal length, %s: largest ||N| - 1| / bound %.3f" % (case, worst))


@pytest.mark.parametrize("row_block", [8, 3])
def test_band_partitions_reassemble(rtow, row_block):
    scene = rtow.five_scene()
    cam = rtow.camera_cpu(aspect=W / H, aperture=0.1, **fc.FIVE_VIEW)
    whole = oracle_lib.kernel_terminals(scene, cam, rtow.make_params(W, H, 3, seed=5), 8)
    seen = np.zeros(H, int)
    for rank in range(2):
        pb = rtow.make_params(W, H, 3, seed=5, rank=rank, world=2, row_block=row_block)
        got = oracle_lib.kernel_terminals(scene, cam, pb, 8)
        rows = rtow.local_to_global_rows(pb)
        inside = rows < H
        assert got[inside].tobytes() == whole[rows[inside]].tobytes()
        pad = got[~inside]
        assert np.all(pad["sphere"] == -1) and not pad["depth"].any() and not pad["events"].any()
        seen[rows[inside]] += 1
    assert np.all(seen == 1)


def test_samples_do_not_depend_on_spp_and_the_vote_is_selects(rtow):
    """Sample s is the same whatever spp is, so the sums of the first k records
    are the sums at spp = k; and route_ref.select on the oracle's keys gives
    the key, votes, n and hits of features_ref.route_state."""
    case, frame = "five-pinhole", (W, H)
    term = fc.terminals(rtow, case, frame, 8, 0.0)
    p = fc.params_of(rtow, case, frame)
    p.spp = 5
    t5 = oracle_lib.kernel_terminals(fc.scene_of(rtow, case), fc.camera_of(rtow, case, frame), p, 8, 0.0)
    assert t5.tobytes() == np.ascontiguousarray(term[..., :5]).tobytes()
    st = route_ref.split_state(features_ref.route_state(term))
    sel = route_ref.select(np.moveaxis(features_ref.route_keys(term), -1, 0), np.moveaxis(term["sphere"] >= 0, -1, 0))
    for n in ("key", "votes", "n", "hits"):
        assert np.array_equal(st[n], sel[n]), n
    s = features_ref.sums(term)
    assert np.array_equal(s["hits"], st["hits"]) and np.array_equal(s["id"], st["id"])
    whole = (sel["n"] == sel["hits"]) & (sel["changes"] == 0)
    assert whole.any() and (~whole).any()
    for n in ("depth", "position", "normal", "albedo"):  # one route, never replaced: rt_guides' sums
        assert st[n][whole].tobytes() == s[n][whole].tobytes(), n


# ---- 6. the case list meets what the byte comparison is for -------------------
def test_the_case_list_covers_every_situation(rtow):
    """Over the GPU file's cases and options: every events bit occurs, and so do
    chains of four and more bounces, escaped chains, and pixels of rt_route
    whose candidate changed and whose route does not hold every hit sample
    (matched < hits).  A byte comparison that never met a refraction would
    prove nothing about refraction.  The 2^100 clamp comes from the synthetic
    clamp scene alone (albedo 3.0: within 64 bounces no albedo <= 2.9 reaches
    it, features_cases.clamp_scene); the hot scene's followed metal (albedo
    1.3) stays below it."""
    count = {k: 0 for k in EV}
    walked = b4 = esc = changed = samples = 0
    for case in fc.CASES:
        for frame in fc.frames_of(case):
            for mb in fc.GUIDES_BOUNCES:
                for mf in fc.GUIDES_FUZZ:
                    t = fc.terminals(rtow, case, frame, mb, mf)
                    samples += t.size
                    for k in EV:
                        count[k] += int(_ev(t, k).sum())
                    walked += int((_ev(t, "skip_tmin") & (t["escaped"] == 0) & (t["sphere"] >= 0)).sum())
                    b4 += int((t["bounces"] >= 4).sum())
                    esc += int((t["escaped"] == 1).sum())
                    if case.startswith("hot"):
                        assert not _ev(t, "clamp").any()
            for mb in fc.ROUTE_BOUNCES:
                t = fc.terminals(rtow, case, frame, mb, 0.0)
                if t.shape[2]:
                    sel = route_ref.select(np.moveaxis(features_ref.route_keys(t), -1, 0),
                                           np.moveaxis(t["sphere"] >= 0, -1, 0))
                    changed += int(((sel["n"] < sel["hits"]) & (sel["changes"] > 0)).sum())
    print("coverage over %d cases, %d sample records: %s; a first-arm skip before a counted hit %d; bounces >= 4 %d; "
          "escaped %d; route pixels with matched < hits and a changed candidate %d" %
          (len(fc.CASES), samples, ", ".join("%s %d" % kv for kv in count.items()), walked, b4, esc, changed))
    assert all(count.values()), count
    assert walked and b4 and esc and changed
    hot = fc.scene_of(rtow, "hot")
    assert ((hot.kind == rtow.RT_METAL) & (hot.albedo.max(-1) > 1) & (hot.param <= np.float32(0.3))).any()
    assert 2.9 ** 65 < 2.0 ** 100 < fc.CLAMP_ALBEDO ** 64


# ---- 7. the failure message ----------------------------------------------------
def test_first_difference_names_the_sample(rtow):
    """features_ref.first_difference, given outputs that lost everything from
    sample 3 on at one pixel, names the buffer, the pixel and sample 3, with the
    restatement that fits the pass: the sums, rt_route's state, its outputs."""
    case, frame = "five-pinhole", (W, H)
    term = fc.terminals(rtow, case, frame, 8, 0.0)
    hits = (term["sphere"] >= 0).sum(-1)
    r, c = (int(v) for v in np.argwhere((term["sphere"][..., 3] >= 0) & (hits == term.shape[2]))[0])
    for restate in (features_ref.sums, features_ref.route_fields, features_ref.route_outputs):
        want = restate(term)
        cut = restate(term[r:r + 1, c:c + 1, :3])
        for name in ("hits", "depth", "normal"):
            got = np.array(want[name])
            got[r, c] = cut[name][0, 0]
            msg = features_ref.first_difference(term, name, got, want[name], restate)
            assert msg.startswith("%s differs at 1 pixels, first (row %d, col %d)" % (name, r, c)), msg
            assert "sample 3 is the first that differs" in msg, msg
            assert features_ref.first_difference(term, name, want[name], want[name], restate) == "no difference"
