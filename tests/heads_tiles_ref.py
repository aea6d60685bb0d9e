"""numpy restatement of the padded nonzero-tile list of mli_live_tiles (n_wtiles_pad,
include/mli_hip.h), on top of tests/live_tiles_ref.py.

The heads take the nonzero tiles eight to a workgroup, so the scan appends (-W mod 8) pad entries
to wtile_list: the lowest compact positions whose tile has no nonzero weight, ascending.  R T is a
multiple of 8, so enough of them exist.  wtile_rank and the first W entries are those of
live_tiles_ref.live_tiles.
"""
import numpy as np

from live_ref import live_rays
from live_tiles_ref import live_tiles, tile_flags


def padded_tiles(weights):
    """(wtile_list with its pads [n_pad], wtile_rank, n_pad) from the [N][R] weights."""
    tile_list, _, _ = live_rays(weights)
    wl, wr = live_tiles(weights)
    W = len(wl)
    nz = tile_flags(weights).reshape(-1)[tile_list]          # per compact position
    pads = np.flatnonzero(~nz)[:(-W) % 8]
    return np.concatenate([wl, pads]).astype(np.int32), wr, (W + 7) // 8 * 8
