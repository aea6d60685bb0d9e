"""The inside-ray list (tests/inside_ref.py, the restatement mli_inside_list and the FIELD pass of
mli_sdf are tested against in test_gpu_field_inside.py) against a brute-force loop, and the
premise of the elision: the share of the benchmark's rays that miss the
bounding sphere (CPU)."""
import numpy as np
import pytest
import torch

from mli_nerf_amd import synthetic
from oracle import render as o_render

from inside_ref import inside_list, patterns, tile_map


def brute(outside, N, n_pad=0):
    """(list, n_inside, compact -> original tile) by plain loops."""
    R, T = len(outside), N // 32
    lst = [r for r in range(R) if not outside[r]]
    n = len(lst)
    for r in range(R):
        if outside[r]:
            lst.append(r)
            if n_pad > 0:   # the first n_pad outside rays are evaluated as well
                n, n_pad = n + 1, n_pad - 1
    tiles = []
    for rc in range(n):
        for j in range(T):
            tiles.append(lst[rc] * T + j)
    return lst, n, tiles


@pytest.mark.parametrize("R", [1, 5, 37, 64, 4096])
def test_list_matches_brute_force(R):
    for name, out in patterns(R).items():
        for N, n_pad in ((32, 0), (64, 0), (128, 0), (32, 7), (128, 1)):
            want_list, want_n, want_tiles = brute(out, N, n_pad)
            lst, n = inside_list(out.astype(np.uint8), n_pad)
            assert lst.dtype == np.int32 and lst.shape == (R,), name
            assert n == want_n and lst.tolist() == want_list, name
            assert np.array_equal(np.sort(lst), np.arange(R)), name   # a permutation of the rays
            tm = tile_map(out, N, n_pad)
            assert tm.tolist() == want_tiles, (name, N)
            # every tile of every evaluated ray exactly once, none of another ray: the inside rays
            # and the first n_pad outside ones
            ev = ~out | (np.cumsum(out) <= n_pad)
            assert np.array_equal(np.sort(tm), np.flatnonzero(np.repeat(ev, N // 32))), (name, N, n_pad)
    # any nonzero flag byte counts as outside
    assert inside_list(np.array([0, 2, 0, 255], np.uint8))[0].tolist() == [0, 2, 1, 3]


def test_tile_map_rejects_partial_tiles():
    with pytest.raises(ValueError):
        tile_map(np.zeros(4, bool), 48)


@pytest.mark.parametrize("frame", [0, 3])
def test_outside_share_of_the_benchmark_batches(frame):
    """The benchmark trains on 4096 uniformly drawn pixels of a 512 x 512 frame of a unit sphere
    seen from distance 4: 0.5908 / 0.5901 of the rays of its batches miss the sphere."""
    d = synthetic.make_batch(4096, 512, 512, frame=frame)
    center, ray = o_render.pixel_rays(d["pose"], d["intr"], d["ray_idx"], 512)
    unit = torch.nn.functional.normalize(ray, dim=-1)
    _, _, outside = o_render.sphere_bounds(center, unit)
    share = float(outside.float().mean())
    print("frame %d: outside share of the batch %.4f" % (frame, share))
    assert 0.57 <= share <= 0.61, share
    lst, n = inside_list(outside.reshape(-1).numpy())
    assert n == 4096 - int(outside.sum())

