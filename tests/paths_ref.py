"""numpy float32 restatement of the wavefront loop's step and of the sums'
conversion (include/rt_paths.h; test infrastructure): rtow.path_trace's lines
between two bounces, with the header's clamp in front of the integer
conversion.  Shared by test_paths.py, which shows it is the loop's, and
test_paths_gpu.py, which compares the device step with it byte for byte."""
import numpy as np

MISS, SCATTERED = 0, 1
NEXT = ("origin", "direction", "from", "key", "throughput", "slot")


def fixed(v, shift):
    """(uint32) fminf(fmaxf(v * 2^shift, 0), 4294967040.f) of float32 values; fmaxf sends a NaN to 0."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        x = np.asarray(v, f32) * f32(2.0 ** shift)
        x = np.where(np.isnan(x), f32(0.0), np.maximum(x, f32(0.0)))  # fmaxf(x, 0)
        x = np.minimum(x, f32(4294967040.0))
    return x.astype(np.uint64).astype(np.uint32)


def step(status, id_, position, scatter, attenuation, key, throughput, slot, sums, shift):
    """One step: sums (uint32 (n_slots, 3), or None) is added into in place,
    modulo 2^32; -> the next batch as a dict of NEXT's arrays, and its count."""
    with np.errstate(all="ignore"):
        thr = np.asarray(throughput, np.float32) * np.asarray(attenuation, np.float32)
    status = np.asarray(status, np.uint8)
    if sums is not None:
        miss = (status == MISS) & (slot < len(sums))
        wide = np.zeros(sums.shape, np.uint64)
        np.add.at(wide, slot[miss], fixed(thr[miss], shift).astype(np.uint64))
        sums += wide.astype(np.uint32)  # (uint32 addition wraps)
    on = status == SCATTERED
    nxt = {"origin": position[on], "direction": scatter[on], "from": id_[on],
           "key": key[on] + np.array([0, 0, 1], np.uint32), "throughput": thr[on], "slot": slot[on]}
    return nxt, int(on.sum())


def frame(sums, shift):
    """(float) sums * 2^-shift."""
    return np.asarray(sums, np.uint32).astype(np.float32) * np.float32(2.0 ** -shift)


def synthetic(n, pattern, seed=0, n_slots=37):
    """A step's eight input arrays with every value distinct enough to show a
    misplaced record.  pattern: "all", "none", "alternate", "last", "first"
    (scattered rays among absorbed ones) or "mix" (a seeded mix of the four
    status values and an out-of-range byte, misses included)."""
    rng = np.random.default_rng([seed, n])
    f32 = np.float32
    if pattern == "mix":
        status = rng.choice(np.array([0, 1, 2, 3, 200], np.uint8), n, p=[0.25, 0.45, 0.15, 0.1, 0.05])
    else:
        status = np.full(n, 2, np.uint8)
        sel = {"all": slice(None), "none": slice(0, 0), "alternate": slice(0, None, 2), "last": slice(n - 1, n),
               "first": slice(0, 1)}[pattern]
        status[sel] = SCATTERED
    return {"status": status, "id": rng.integers(-2, 500, n).astype(np.int32),
            "position": rng.normal(size=(n, 3)).astype(f32), "scatter": rng.normal(size=(n, 3)).astype(f32),
            "attenuation": rng.random((n, 3)).astype(f32),
            "key": rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint64).astype(np.uint32),
            "throughput": rng.random((n, 3)).astype(f32), "slot": rng.integers(0, n_slots, n).astype(np.uint32)}
