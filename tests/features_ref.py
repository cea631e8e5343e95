"""numpy restatement of what rt_aov, rt_guides and rt_route do with a pixel's
samples once each sample's chain has ended (include/rt_aov.h, rt_guides.h,
rt_route.h): the fp32 sums in ascending sample order from +0, and rt_route's
one-sweep vote with its sums.  The samples' terminals come from the chain
oracle (oracle_lib.kernel_terminals, a structured array shaped (rows, W, spp));
everything here is float32 arithmetic on them, so the results are meant to be
compared with the passes' outputs byte for byte."""
import numpy as np

import route_ref

AOV = ("hits", "id", "depth", "position", "normal", "albedo")
GUIDES = AOV + ("bounces", "escaped")
ROUTE = AOV + ("route", "matched")
# the features of a hit sample, as the terminal record names them
FIELDS = (("depth", "depth"), ("position", "P"), ("normal", "N"), ("albedo", "thr"))


def _hit(term):
    return term["sphere"] >= 0


def _first_id(term):
    """Sample 0's terminal sphere, -1 if it missed (or there is no sample)."""
    if term.shape[-1] == 0:
        return np.full(term.shape[:-1], -1, np.int32)
    return term["sphere"][..., 0].astype(np.int32)  # a miss's sphere is -1


def sums(term):
    """The eight buffers of rt_guides (the first six are rt_aov's): hits, id of
    sample 0, and the float32 sums of depth, P, N and thr over the hit samples,
    added in ascending sample order starting from +0 -- a miss adds nothing (the
    add is masked, not an add of zero, which would turn a -0 sum into +0) --
    and the integer sums of bounces and escaped."""
    hit = _hit(term)
    out = {"hits": hit.sum(-1).astype(np.uint32), "id": _first_id(term),
           "bounces": np.where(hit, term["bounces"], 0).sum(-1).astype(np.uint32),
           "escaped": np.where(hit, term["escaped"], 0).sum(-1).astype(np.uint32)}
    for name, field in FIELDS:
        x = term[field]  # (rows, W, spp) or (rows, W, spp, 3)
        acc = np.zeros(x.shape[:2] + x.shape[3:], np.float32)
        for s in range(x.shape[2]):
            h = hit[..., s] if acc.ndim == 2 else hit[..., s, None]
            acc = np.where(h, acc + x[:, :, s], acc)
            assert acc.dtype == np.float32
        out[name] = acc
    return out


def route_keys(term):
    """Every sample's route key k = ((b << 1) | e) + 1 (0 where it missed)."""
    return np.where(_hit(term), route_ref.route_key(term["bounces"], term["escaped"]), np.uint32(0)).astype(np.uint32)


def route_state(term):
    """rt_route's per-pixel state after the last sample, as the raw uint32
    (4, rows, W, 4) array of the header's layout: the samples in ascending
    order; a miss changes nothing; a hit sample adds one to hits (sample 0
    gives id); with votes == 0 it is adopted (key = k, votes = n = 1, each sum
    (+0) + x), with the held key it adds one to votes and n and x to each sum,
    with another key it takes one vote away.  float32 throughout."""
    hit, keys = _hit(term), route_keys(term)
    shape = term.shape[:2]
    key, votes, n, hits = (np.zeros(shape, np.uint32) for _ in range(4))
    acc = {name: np.zeros(shape + term[field].shape[3:], np.float32) for name, field in FIELDS}
    one, zero = np.uint32(1), np.float32(0.0)
    for s in range(term.shape[2]):
        h, k = hit[..., s], keys[..., s]
        hits = hits + h.astype(np.uint32)
        adopt = h & (votes == 0)
        same = h & ~adopt & (k == key)
        other = h & ~adopt & ~same
        for name, field in FIELDS:
            x = term[field][:, :, s]
            a, m = (adopt, same) if x.ndim == 2 else (adopt[..., None], same[..., None])
            acc[name] = np.where(a, zero + x, np.where(m, acc[name] + x, acc[name]))
            assert acc[name].dtype == np.float32
        key = np.where(adopt, k, key)
        votes = np.where(adopt, one, votes + same.astype(np.uint32) - other.astype(np.uint32))
        n = np.where(adopt, one, n + same.astype(np.uint32))
    return route_ref.make_state(key, votes, n, hits, acc["depth"], acc["position"], acc["normal"], acc["albedo"],
                                _first_id(term))


def route_outputs(term):
    """rt_route's eight outputs: the finalize of route_state."""
    return route_ref.finalize(route_state(term))


def route_fields(term):
    """rt_route's state by field (route_ref.split_state of route_state)."""
    return route_ref.split_state(route_state(term))


def first_difference(term, name, got, expect, restate=sums):
    """For a failure message: the first pixel (row, col) at which buffer `name`
    differs, and the sample the difference starts at -- the smallest k for which
    the restatement of that pixel's first k samples alone still has the GPU's
    bytes (the GPU then lost or changed sample k) -- with the oracle's records
    of that pixel's samples.  restate(term) -> dict is the restatement `expect`
    came from: sums for rt_aov and rt_guides, route_fields for rt_route's state,
    route_outputs for its outputs.  CPU work only."""
    g = np.ascontiguousarray(got).reshape(expect.shape[:2] + (-1,)).view(np.uint32)
    e = np.ascontiguousarray(expect).reshape(expect.shape[:2] + (-1,)).view(np.uint32)
    bad = np.argwhere((g != e).any(-1))
    if not len(bad):
        return "no difference"
    r, c = (int(v) for v in bad[0])
    px = term[r:r + 1, c:c + 1]
    at = None
    for k in range(term.shape[2] + 1):
        part = np.ascontiguousarray(restate(px[..., :k])[name]).reshape(1, 1, -1).view(np.uint32)
        if np.array_equal(part[0, 0], g[r, c]):
            at = k
            break
    where = ("the restatement of the oracle's first %d samples gives the GPU's value: sample %d is the first that "
             "differs" % (at, at) if at is not None and at < term.shape[2] else
             "no prefix of the oracle's samples gives the GPU's value")
    return "%s differs at %d pixels, first (row %d, col %d): GPU %r, oracle %r; %s; oracle records of the pixel:\n%s" % (
        name, len(bad), r, c, np.asarray(got)[r, c].tolist(), np.asarray(expect)[r, c].tolist(), where,
        "\n".join("  s=%d %r" % (s, px[0, 0, s].tolist()) for s in range(min(term.shape[2], 16))))
