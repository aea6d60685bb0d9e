"""numpy restatement of mli_live_rays (include/mli_hip.h): which rays of a batch the
heads have to process, and the compaction the heads and weight-gradient kernels address by.

A ray is live when at least one of its N composite weights is not exactly 0.0.  With T = N / 32
tiles per ray and G = 256 / N rays per 256-sample workgroup (256 % N == 0, R % G == 0):

  tile_list [R T]      compact position -> original tile r T + j: the live rays in ascending
                       order, then the dead rays in ascending order.  The first (-L mod G) dead
                       rays pad the last workgroup of live rays; they are processed like live ones.
  tile_rank [R T + 1]  live tiles before each original tile (pad rays are not counted); the last
                       element is L T.  The original sample range [k0, k1) (multiples of 32) holds
                       the compact tiles [tile_rank[k0 / 32], tile_rank[k1 / 32]).
  n_live_tiles         ceil(L / G) G T: the tiles the heads kernels process, a multiple of 8.
"""
import numpy as np


def live_flags(weights):
    """[N][R] weights -> [R] bool."""
    return (np.asarray(weights) != 0).any(axis=0)


def live_rays(weights):
    """(tile_list, tile_rank, n_live_tiles) as int32 arrays / int, from the [N][R] weights."""
    w = np.asarray(weights)
    N, R = w.shape
    if N % 32 or 256 % N or R % (256 // N):
        raise ValueError("live_rays: N = %d, R = %d" % (N, R))
    T, G = N // 32, 256 // N
    live = live_flags(w)
    L = int(live.sum())
    order = np.concatenate([np.flatnonzero(live), np.flatnonzero(~live)])
    j = np.arange(T)
    tile_list = (order[:, None] * T + j).reshape(-1).astype(np.int32)
    before = np.cumsum(live) - live          # live rays before each ray
    rank = before[:, None] * T + np.where(live[:, None], j, 0)
    tile_rank = np.concatenate([rank.reshape(-1), [L * T]]).astype(np.int32)
    return tile_list, tile_rank, -(-L // G) * G * T
