"""The nonzero-tile lists (tests/live_tiles_ref.py, the restatement mli_live_tiles is tested
against in test_gpu_live_tiles.py) on hand-made weights (CPU)."""
import numpy as np
import pytest

from live_ref import live_rays
from live_tiles_ref import live_tiles, tile_flags

NS = (32, 128, 256)


def weights_from_tiles(nz, N, value=0.5):
    """[R][T] bool -> [N][R] weights: one nonzero weight (sample 32 j + (5 r + 7 j) % 32) in
    every flagged tile."""
    R, T = nz.shape
    assert T == N // 32
    w = np.zeros((N, R), np.float32)
    for r, j in zip(*np.nonzero(nz)):
        w[32 * j + (5 * r + 7 * j) % 32, r] = value
    return w


def _check(w, nz):
    """The lists of weights w against their definition, written out by hand."""
    N, R = w.shape
    T = N // 32
    assert np.array_equal(tile_flags(w), nz)
    tl, tr, n = live_rays(w)
    wl, wr = live_tiles(w)
    assert wl.dtype == np.int32 and wr.dtype == np.int32 and wr.shape == (R * T + 1,)
    flat = nz.reshape(-1)
    want = [p for p in range(R * T) if flat[tl[p]]]
    assert wl.tolist() == want
    assert wr.tolist() == [sum(1 for q in want if q < p) for p in range(R * T + 1)]
    Lt = int(tr[-1])
    assert (wl < Lt).all() and (wr[Lt:] == len(want)).all()       # pad and dead rays drop out
    assert (np.diff(wl) > 0).all()
    # an aligned original range streams exactly its nonzero tiles, in order
    for k0 in range(0, R * T, 2):
        for k1 in (k0 + 2, R * T):
            got = tl[wl[wr[tr[k0]]:wr[tr[k1]]]]
            assert got.tolist() == [t for t in range(k0, k1) if flat[t]]
    return wl, wr


@pytest.mark.parametrize("N", NS)
def test_no_live_tile(N):
    R, T = 16, N // 32
    wl, wr = _check(np.zeros((N, R), np.float32), np.zeros((R, T), bool))
    assert len(wl) == 0 and not wr.any()


@pytest.mark.parametrize("N", NS)
def test_every_tile_live(N):
    R, T = 16, N // 32
    nz = np.ones((R, T), bool)
    wl, wr = _check(weights_from_tiles(nz, N), nz)
    assert wl.tolist() == list(range(R * T)) and wr.tolist() == list(range(R * T + 1))


@pytest.mark.parametrize("N", NS)
def test_one_tile_in_the_first_ray_and_one_in_the_last(N):
    R, T = 16, N // 32
    nz = np.zeros((R, T), bool)
    nz[0, T - 1] = nz[R - 1, 0] = True
    wl, _ = _check(weights_from_tiles(nz, N), nz)
    assert wl.tolist() == [T - 1, T]          # two live rays: compact tiles 0 .. 2 T


@pytest.mark.parametrize("N", (128, 256))
def test_live_rays_with_holes(N):
    R, T = 16, N // 32
    nz = np.zeros((R, T), bool)
    nz[::2, 0] = nz[::2, 2] = True            # tiles 0 and 2 of every other ray
    nz[5, 1] = True
    wl, _ = _check(weights_from_tiles(nz, N), nz)
    assert wl[:4].tolist() == [0, 2, T, T + 2]


@pytest.mark.parametrize("N", NS)
def test_pad_rays(N):
    """L live rays with L % G != 0: the dead rays that fill the last workgroup have no entry."""
    R, T, G = 16, N // 32, 256 // N
    nz = np.zeros((R, T), bool)
    nz[[3, 4, 9], :] = True
    nz[9, 0] = T == 1                         # (a ray needs one nonzero tile to be live)
    w = weights_from_tiles(nz, N)
    wl, wr = _check(w, nz)
    _, tr, n = live_rays(w)
    assert n == -(-3 // G) * G * T and len(wl) == int(nz.sum()) and wr[-1] == wr[3 * T]


@pytest.mark.parametrize("N", NS)
def test_negative_zero_and_denormals(N):
    R, T = 8, N // 32
    nz = np.zeros((R, T), bool)
    nz[2, T - 1] = nz[6, 0] = True
    w = weights_from_tiles(nz, N, value=1e-45)     # the smallest denormal: live
    w[::3, :] = np.where(w[::3, :] == 0, np.float32(-0.0), w[::3, :])   # -0.0: dead
    assert np.signbit(w).any()
    _check(w, nz)
    w[N - 1, 4] = np.nan                           # NaN: live
    nz[4, T - 1] = True
    _check(w, nz)


@pytest.mark.parametrize("N", NS)
def test_random(N):
    rng = np.random.default_rng(N)
    R, T = 24, N // 32
    nz = rng.random((R, T)) < 0.5
    nz[rng.random(R) < 0.3] = False
    _check(weights_from_tiles(nz, N), nz)

