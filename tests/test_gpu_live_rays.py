"""mli_live_rays alone against its numpy restatement (tests/live_ref.py), bit for bit (GPU).

Shapes R in {8, 16, 40} x N in {32, 64, 128, 256} (one to eight tiles per ray, one to eight rays
per workgroup, a ray count that is no multiple of the flag pass's 64 rays per workgroup or of the
scan's thread count), the patterns of test_live_ref.py (all live, all dead, one live ray first /
last, alternating, odd live counts -- the pad path --, runs, random).  Every output has canaries
behind it; the y rows of dead rays must be zero and those of live rays untouched.
"""
import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L

from live_ref import live_rays
from test_live_ref import SHAPES, patterns, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0x5A5A5A5A
PAD = 64


def _guarded(n, dtype):
    """n elements followed by PAD canary words (int32 views of the same storage)."""
    raw = torch.full((n + PAD,), CANARY, dtype=torch.int32, device=DEV)
    return raw, raw[:n].view(dtype)


@pytest.mark.parametrize("R,N", SHAPES)
def test_lists_match_the_restatement(R, N):
    T = N // 32
    for name, live in patterns(R).items():
        w = weights_of(live, N, seed=R + N)
        wd = torch.from_numpy(w).to(DEV)
        y0 = torch.rand(N, R, 8, generator=torch.Generator().manual_seed(R + N)) + 0.5
        raw_y, y = _guarded(N * R * 8, torch.float32)
        y.copy_(y0.reshape(-1).to(DEV))
        raw_f, flags = _guarded(R, torch.int32)
        raw_l, tl = _guarded(R * T, torch.int32)
        raw_r, tr = _guarded(R * T + 1, torch.int32)
        raw_n, nl = _guarded(1, torch.int32)
        L.call("mli_live_rays", L.LiveRaysArgs(R, N, L.ptr(wd), L.ptr(y), L.ptr(flags), L.ptr(tl), L.ptr(tr),
                                               L.ptr(nl)))
        torch.cuda.synchronize()
        ref_l, ref_r, ref_n = live_rays(w)
        assert np.array_equal(tl.cpu().numpy(), ref_l), name
        assert np.array_equal(tr.cpu().numpy(), ref_r), name
        assert int(nl.cpu()) == ref_n, name
        assert np.array_equal(flags.cpu().numpy() != 0, live), name
        for raw in (raw_y, raw_f, raw_l, raw_r, raw_n):
            assert bool((raw[-PAD:] == CANARY).all()), name
        got = y.view(N, R, 8).cpu()
        want = y0.clone()
        want[:, torch.from_numpy(~live)] = 0
        assert torch.equal(got, want), name


def test_y_is_optional_and_bad_shapes_are_refused():
    R, N = 8, 128
    w = torch.zeros(N, R, device=DEV)
    w[5, 3] = 1.0
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)  # noqa: E731
    flags, tl, tr, nl = i32(R), i32(R * 4), i32(R * 4 + 1), i32(1)
    L.call("mli_live_rays", L.LiveRaysArgs(R, N, L.ptr(w), None, L.ptr(flags), L.ptr(tl), L.ptr(tr), L.ptr(nl)))
    torch.cuda.synchronize()
    assert int(nl.cpu()) == 8 and tl[:4].tolist() == [12, 13, 14, 15] and int(tr[-1]) == 4
    for r, n in ((8, 192), (8, 96), (3, 128), (8, 48)):
        with pytest.raises(RuntimeError):
            L.call("mli_live_rays", L.LiveRaysArgs(r, n, L.ptr(w), None, L.ptr(flags), L.ptr(tl), L.ptr(tr),
                                                   L.ptr(nl)))
