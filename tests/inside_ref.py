"""numpy restatement of the inside-ray list (mli_inside_list, include/mli_hip.h) and of the
compact-to-original tile map the FIELD pass of mli_sdf applies with it."""
import numpy as np


def inside_list(outside, n_pad=0):
    """outside [R] (any nonzero = the ray misses the bounds) -> (inside_list [R] int32: the rays
    inside the bounds ascending, then the others ascending; n_inside: the rays inside the bounds
    plus the first n_pad of the others, as far as there are any)."""
    out = np.asarray(outside) != 0
    r = np.arange(len(out), dtype=np.int32)
    return np.concatenate([r[~out], r[out]]).astype(np.int32), min(int((~out).sum()) + n_pad, len(out))


def tile_map(outside, N, n_pad=0):
    """The original 32-sample tile of every compact tile the FIELD pass evaluates
    ([n_inside * N / 32] int64); compact tiles past them are skipped."""
    if N % 32:
        raise ValueError("n_per_ray = %d is not a whole number of 32-sample tiles" % N)
    lst, n = inside_list(outside, n_pad)
    T = N // 32
    ci = np.arange(n * T, dtype=np.int64)
    return lst[ci // T].astype(np.int64) * T + ci % T


def patterns(R, seed=0):
    """name -> [R] bool outside flags: the crafted patterns and a seeded 60 % draw."""
    r = np.arange(R)
    return {"none": np.zeros(R, bool), "all": np.ones(R, bool), "first_inside": r != 0,
            "last_inside": r != R - 1, "alternating": r % 2 == 1,
            "draw60": np.random.default_rng(1000 * seed + R).random(R) < 0.6}
