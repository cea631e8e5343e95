"""numpy restatement of the two parts of rt_route (include/rt_route.h) that have
no tracing in them: the per-pixel one-sweep majority vote over the samples'
route keys, and the finalize step from the state to the output buffers."""
import numpy as np

NO_HIT = np.uint32(0xFFFFFFFF)
FEATURES = ("depth", "position", "normal", "albedo")


def route_key(bounces, escaped):
    """k = ((b << 1) | e) + 1, a uint32 that is never 0."""
    return ((np.asarray(bounces).astype(np.uint32) << np.uint32(1)) | np.asarray(escaped).astype(np.uint32)) + \
        np.uint32(1)


def select(keys, hit):
    """The vote of rt_route.h over keys[S, ...] (uint32) of the samples with
    hit[S, ...] (bool), in ascending sample order: a miss changes nothing; a hit
    sample with votes == 0 is adopted (key = k, votes = n = 1), one with the
    held key adds one to votes and n, any other takes one vote away.

    Returns a dict of arrays shaped like keys[0]: key, votes, n, hits (uint32),
    adopted (the sample index of the last adoption, -1 = none), changes (how
    often an adoption replaced a different key) and the bool array member[S,
    ...]: the samples the final sums cover (the held key's since its last
    adoption)."""
    keys = np.asarray(keys, np.uint32)
    hit = np.asarray(hit, bool)
    shape = keys.shape[1:]
    key, votes, n, hits = (np.zeros(shape, np.uint32) for _ in range(4))
    adopted = np.full(shape, -1, np.int64)
    changes = np.zeros(shape, np.int64)
    member = np.zeros(keys.shape, bool)
    for s in range(keys.shape[0]):
        h, k = hit[s], keys[s]
        hits = hits + h.astype(np.uint32)
        adopt = h & (votes == 0)
        same = h & ~adopt & (k == key)
        other = h & ~adopt & ~same
        assert not (other & (votes == 0)).any()  # votes never goes below 0
        changes += adopt & (key != 0) & (key != k)
        member[:, adopt] = False
        member[s] = adopt | same
        key = np.where(adopt, k, key)
        votes = np.where(adopt, np.uint32(1), votes + same.astype(np.uint32) - other.astype(np.uint32))
        n = np.where(adopt, np.uint32(1), n + same.astype(np.uint32))
        adopted = np.where(adopt, s, adopted)
    return dict(key=key, votes=votes, n=n, hits=hits, adopted=adopted, changes=changes, member=member)


def split_state(state):
    """The header's state layout, from the raw uint32 (4, rows, W, 4): plane 0
    (key, votes, n, hits), plane 1 (P.xyz, depth), plane 2 (N.xyz, id bits),
    plane 3 (albedo.rgb, 0)."""
    state = np.ascontiguousarray(state, np.uint32)
    f = state.view(np.float32)
    return dict(key=state[0, ..., 0], votes=state[0, ..., 1], n=state[0, ..., 2], hits=state[0, ..., 3],
                position=f[1, ..., :3], depth=f[1, ..., 3], normal=f[2, ..., :3], id=state[2, ..., 3].view(np.int32),
                albedo=f[3, ..., :3], pad=state[3, ..., 3])


def make_state(key, votes, n, hits, depth, position, normal, albedo, ident):
    """The raw uint32 (4, ..., 4) state of the given fields."""
    shape = np.shape(key)
    st = np.zeros((4,) + shape + (4,), np.uint32)
    f = st.view(np.float32)
    for i, a in enumerate((key, votes, n, hits)):
        st[0, ..., i] = a
    f[1, ..., :3], f[1, ..., 3] = position, depth
    f[2, ..., :3] = normal
    st[2, ..., 3] = np.asarray(ident, np.int32).view(np.uint32)
    f[3, ..., :3] = albedo
    return st


def finalize(state):
    """rt_route.h's finalize, in float32: hits and id copied; depth, position,
    normal and albedo the state's sums where n == hits, else per component
    (sum / float32(n)) * float32(hits), each operation rounded to float32;
    route = key - 1 in uint32 arithmetic (0xFFFFFFFF when hits == 0); matched =
    n."""
    s = split_state(state)
    n, hits = s["n"], s["hits"]
    whole = n == hits
    fn, fh = n.astype(np.float32), hits.astype(np.float32)
    out = dict(hits=hits.copy(), id=s["id"].copy(), route=s["key"] - np.uint32(1), matched=n.copy())
    for name in FEATURES:
        x = s[name]
        w, a, b = (whole, fn, fh) if x.ndim == whole.ndim else (whole[..., None], fn[..., None], fh[..., None])
        with np.errstate(divide="ignore", invalid="ignore"):
            scaled = ((x / a).astype(np.float32) * b).astype(np.float32)
        out[name] = np.where(w, x, scaled)
    return out
