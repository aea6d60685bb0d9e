"""Properties of the live-ray compaction (tests/live_ref.py, the restatement mli_live_rays is
tested against bit for bit in test_gpu_live_rays.py) (CPU)."""
import numpy as np
import pytest

from live_ref import live_flags, live_rays


def patterns(R):
    """name -> [R] bool live flags: the crafted patterns and a few random ones."""
    r = np.arange(R)
    out = {"all_live": np.ones(R, bool), "all_dead": np.zeros(R, bool), "first": r == 0, "last": r == R - 1,
           "alternating": r % 2 == 0, "alternating_odd": r % 2 == 1, "three": r < 3, "five_spread": (r * 5) % R < 5,
           "runs": (r // 3) % 2 == 1, "all_but_one": r != R // 2}
    rng = np.random.default_rng(R)
    for i, p in enumerate((0.1, 0.4, 0.9)):
        out["random%d" % i] = rng.random(R) < p
    return out


def weights_of(live, N, seed=0):
    """[N][R] float32 weights with the given live rays: a live ray has one to N non-zero weights
    (denormals, negative zero on the dead side and a lone last sample among them)."""
    R = len(live)
    rng = np.random.default_rng(seed)
    w = np.zeros((N, R), np.float32)
    for r in np.flatnonzero(live):
        n = int(rng.integers(1, N + 1))
        ks = rng.choice(N, n, replace=False)
        w[ks, r] = rng.choice(np.array([1e-45, 1e-20, 0.25, 1.0], np.float32), n)
    dead = np.flatnonzero(~np.asarray(live))
    w[::3, dead[::2]] = -0.0    # -0.0 == 0.0: still dead
    if live.any():
        w[:, np.flatnonzero(live)[0]] = 0
        w[N - 1, np.flatnonzero(live)[0]] = 1e-45   # only the last sample, the smallest denormal
    return w


SHAPES = [(R, N) for R in (8, 16, 40) for N in (32, 64, 128, 256)]


@pytest.mark.parametrize("R,N", SHAPES)
def test_properties(R, N):
    T, G = N // 32, 256 // N
    for name, live in patterns(R).items():
        w = weights_of(live, N, seed=R + N)
        assert np.array_equal(live_flags(w), live), name
        tl, tr, n = live_rays(w)
        L = int(live.sum())
        assert tl.dtype == np.int32 and tr.dtype == np.int32
        assert tl.shape == (R * T,) and tr.shape == (R * T + 1,)
        # the list is a permutation; the processed prefix holds distinct tiles of whole rays
        assert np.array_equal(np.sort(tl), np.arange(R * T)), name
        assert n % 8 == 0 and L * T <= n < L * T + 8 and n <= R * T, name
        rays = tl.reshape(R, T)
        assert np.array_equal(rays, rays[:, :1] + np.arange(T)) and (rays[:, 0] % T == 0).all(), name
        order = rays[:, 0] // T
        # live rays first, ascending; pad rays are dead and lie beyond every rank range
        assert live[order[:L]].all() and (np.diff(order[:L]) > 0).all(), name
        assert not live[order[L:]].any() and (np.diff(order[L:]) > 0).all(), name
        assert tr[-1] == L * T and tr[0] == 0 and tr.max() == L * T, name
        # rank is monotone, steps by one inside live rays, and inverts the list on live tiles
        d = np.diff(tr)
        assert ((d == 0) | (d == 1)).all(), name
        assert np.array_equal(d == 1, np.repeat(live, T)), name
        live_tiles = np.flatnonzero(np.repeat(live, T))
        assert np.array_equal(tl[tr[live_tiles]], live_tiles), name
        # any aligned original range maps to the compact tiles of exactly its live tiles
        for k0 in range(0, R * T, 2):
            for k1 in (k0 + 2, R * T):
                assert np.array_equal(tl[tr[k0]:tr[k1]], live_tiles[(live_tiles >= k0) & (live_tiles < k1)]), name


def test_rejects_other_shapes():
    for N, R in ((192, 4), (96, 8), (128, 3), (32, 4)):
        with pytest.raises(ValueError):
            live_rays(np.zeros((N, R), np.float32))

