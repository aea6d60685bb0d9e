"""The padded nonzero-tile list (tests/heads_tiles_ref.py, the restatement mli_live_tiles'
n_wtiles_pad output is tested against in test_gpu_heads_tiles.py) against a scalar loop over random
flag words (CPU)."""
import numpy as np
import pytest

from heads_tiles_ref import padded_tiles
from live_tiles_ref import live_tiles
from test_live_tiles_ref import weights_from_tiles


def _scalar_scan(flags, T):
    """The scan of csrc/rays.hip written as one loop per ray over its flag word: (wtile_list with
    pads, wtile_rank, padded count)."""
    R = len(flags)
    live = [r for r in range(R) if flags[r]]
    dead = [r for r in range(R) if not flags[r]]
    W = sum(bin(f).count("1") for f in flags)
    n_pad = (8 - W % 8) % 8
    wl, wr, pads = [], [], []
    for pos, r in enumerate(live + dead):
        for i in range(T):
            p = pos * T + i
            wr.append(len(wl) if flags[r] else W)
            if (flags[r] >> i) & 1:
                wl.append(p)
            elif p - (len(wl) if flags[r] else W) < n_pad:       # all-zero tiles below this one
                pads.append(p)
    assert len(wl) == W and len(pads) == n_pad
    return wl + pads, wr + [W], W + n_pad


def _nz_from_flags(flags, T):
    return np.array([[(f >> i) & 1 for i in range(T)] for f in flags], bool)


def _check(flags, N):
    T = N // 32
    nz = _nz_from_flags(flags, T)
    w = weights_from_tiles(nz, N)
    got_l, got_r, got_n = padded_tiles(w)
    ref_l, ref_r, ref_n = _scalar_scan(flags, T)
    assert got_l.tolist() == ref_l and got_r.tolist() == ref_r and got_n == ref_n
    wl, wr = live_tiles(w)
    W = len(wl)
    # wtile_rank and the first W entries keep their meaning; the pads are distinct all-zero tiles
    assert np.array_equal(got_r, wr) and np.array_equal(got_l[:W], wl)
    assert got_n % 8 == 0 and 0 <= got_n - W < 8 and len(got_l) == got_n <= len(flags) * T
    pads = got_l[W:]
    assert (np.diff(pads) > 0).all() and not set(pads.tolist()) & set(wl.tolist())
    return W, got_n


@pytest.mark.parametrize("N", (32, 64, 128, 256))
def test_random_flag_words(N):
    T, G = N // 32, 256 // N
    rng = np.random.default_rng(N)
    seen = set()
    for trial in range(60):
        R = G * int(rng.integers(1, 12))
        flags = rng.integers(0, 1 << T, R)
        flags[rng.random(R) < 0.3] = 0
        W, n = _check([int(f) for f in flags], N)
        seen.add(W % 8)
    assert seen == set(range(8))


@pytest.mark.parametrize("N", (32, 64, 128, 256))
def test_edges(N):
    T, G = N // 32, 256 // N
    full = (1 << T) - 1
    for R in (G, 3 * G):
        assert _check([full] * R, N) == (R * T, R * T)          # no zero tile exists; W % 8 == 0, no pads
        assert _check([0] * R, N) == (0, 0)                     # no live ray
        assert _check([0] * (R - 1) + [1 << (T - 1)], N) == (1, 8)     # seven pads, most from dead rays
    # W % 8 == 0 with zero tiles around: no pads
    flags = [full] * (8 // T if T < 8 else 1) + [0] * G * 2
    flags = flags + [0] * (-len(flags) % G)
    W, n = _check(flags, N)
    assert W == n == 8
    # W % 8 == 7: one pad
    flags = [full] * (7 // T) + ([(1 << (7 % T)) - 1] if 7 % T else [])
    flags = flags + [0] * (-len(flags) % G)
    W, n = _check(flags, N)
    assert W == 7 and n == 8

