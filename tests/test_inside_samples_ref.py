"""The compact sample map of the listed sampling rounds (tests/inside_samples_ref.py, which
test_gpu_sampler_inside.py tests the kernels against) and the premise of skipping those rounds:
a ray with sdf = outside_val and zero gradients has composite weights of exactly 0 whatever its
dists are, as long as they lie in [near, far] (CPU, the oracle alone)."""
import numpy as np
import pytest
import torch

from oracle import render as o_render

from inside_ref import inside_list, patterns, tile_map
from inside_samples_ref import fill_dists, listed_rays, sample_map


@pytest.mark.parametrize("R", [1, 5, 37, 64])
@pytest.mark.parametrize("n_per_ray", [1, 4, 16, 37, 64])
def test_sample_map_is_a_bijection_onto_the_listed_rays(R, n_per_ray):
    for name, out in patterns(R).items():
        for n_pad in (0, 3, 7):
            sm = sample_map(out, n_per_ray, n_pad)
            ev = listed_rays(out, n_pad)
            lst, n = inside_list(out, n_pad)
            assert int(ev.sum()) == n and sm.shape == (n * n_per_ray,), (name, n_pad)
            # every slot of every listed ray exactly once, no slot of another ray
            want = (np.arange(n_per_ray)[:, None] * R + np.flatnonzero(ev)[None]).reshape(-1)
            assert np.array_equal(np.sort(sm), np.sort(want)), (name, n_pad)
            assert len(np.unique(sm)) == len(sm), (name, n_pad)
            assert ev[sm % R].all(), (name, n_pad)
            if n_per_ray % 32 == 0:
                # sample-major compact points of tile ci are the 32 samples of FIELD's compact tile
                T = n_per_ray // 32
                tm = tile_map(out, n_per_ray, n_pad)
                r, k = sm % R, sm // R
                assert np.array_equal((r * n_per_ray + k) // 32, np.repeat(tm, 32)), (name, n_pad)
                assert np.array_equal(tm // T, r[::32]), (name, n_pad)


def test_fill_dists_contract():
    rng = np.random.default_rng(5)
    near = rng.uniform(0.0, 3.0, 50).astype(np.float32)
    far = near + rng.uniform(0.0, 2.0, 50).astype(np.float32)
    far[:3] = near[:3]                                  # an empty interval
    near[3], far[3] = 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))
    for N in (1, 32, 128, 256):
        d = fill_dists(near, far, N)
        assert d.dtype == np.float32 and d.shape == (N, 50)
        assert np.isfinite(d).all() and (d >= near).all() and (d <= far).all()
        assert (np.diff(d, axis=0) >= 0).all()


@pytest.mark.parametrize("s_var", [-3.9, 0.0, 3.0, 6.3, 12.0])
@pytest.mark.parametrize("progress", [0.0, 0.05, 1.0])
def test_outside_rays_have_exactly_zero_weights_for_any_dists_in_bounds(s_var, progress):
    R, N, outside_val = 64, 32, 1000.0
    g = torch.Generator().manual_seed(3)
    near = torch.full((1, R, 1), 1.0)
    far = torch.full((1, R, 1), 1.2)
    near[0, R // 2:, 0] = torch.rand(R - R // 2, generator=g) * 4.0
    far[0, R // 2:, 0] = near[0, R // 2:, 0] + torch.rand(R - R // 2, generator=g) * 3.0 + 1e-3
    unit = torch.nn.functional.normalize(torch.randn(1, R, 3, generator=g), dim=-1)
    sdfs = torch.full((1, R, N, 1), outside_val)
    grads = torch.zeros(1, R, N, 3)
    fill = torch.from_numpy(fill_dists(near[0, :, 0].numpy(), far[0, :, 0].numpy(), N)).t().reshape(1, R, N, 1)
    drawn = near[..., None] + torch.rand(1, R, N, 1, generator=g) * (far - near)[..., None]   # unsorted
    for dists in (fill, drawn):
        assert bool(((dists[..., 0] >= near) & (dists[..., 0] <= far)).all())
        alpha = o_render.neus_alphas(torch.tensor(s_var), unit, sdfs, grads, dists, far, progress, 0.1)
        w = o_render.exclusive_transmittance_weights(alpha)
        assert alpha.shape == (1, R, N) and bool((alpha == 0).all()) and bool((w == 0).all())
