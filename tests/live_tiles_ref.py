"""numpy restatement of the nonzero-tile lists of mli_live_tiles (include/mli_hip.h), on top of
tests/live_ref.py.

A 32-sample tile is nonzero when at least one of its composite weights has a nonzero bit pattern
(+-0.0 dead; denormals and NaN live).  In the compact order of live_ref.live_rays (positions
0 .. R T, the live rays first):

  wtile_list [W]        the compact positions whose original tile tile_list[p] is nonzero,
                        ascending.  Only live rays have such tiles, so W <= L T; pad and dead rays
                        drop out.
  wtile_rank [R T + 1]  entries of wtile_list below compact position p; the last element is W.
                        The compact range [c0, c1) holds the entries
                        [wtile_rank[c0], wtile_rank[c1]) of wtile_list.
"""
import numpy as np

from live_ref import live_rays


def tile_flags(weights):
    """[N][R] float32 weights -> [R][T] bool: tile j of ray r has a nonzero bit pattern."""
    w = np.ascontiguousarray(weights, np.float32)
    N, R = w.shape
    bits = w.view(np.uint32) & np.uint32(0x7FFFFFFF)
    return (bits != 0).reshape(N // 32, 32, R).any(axis=1).T


def live_tiles(weights):
    """(wtile_list, wtile_rank) as int32 arrays, from the [N][R] weights."""
    tile_list, _, _ = live_rays(weights)
    nz = tile_flags(weights).reshape(-1)[tile_list]      # per compact position
    wtile_list = np.flatnonzero(nz).astype(np.int32)
    wtile_rank = np.concatenate([[0], np.cumsum(nz)]).astype(np.int32)
    return wtile_list, wtile_rank
