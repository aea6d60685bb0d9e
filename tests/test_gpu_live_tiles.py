"""mli_live_tiles alone, through the C ABI (GPU): the weights pass with the live-ray and
nonzero-tile lists, in one launch (the last workgroup scans) and in two (scan_launch).

For every shape the pass runs twice back to back on the same buffers with different inputs (a
ticket that was not reset would leave the second run's lists unwritten or written early):
  * its weights are bit-equal to mli_composite_fwd(y = NULL) on the same inputs;
  * tile_list, tile_rank and n_live_tiles equal live_ref.live_rays of those weights;
  * wtile_list and wtile_rank equal live_tiles_ref.live_tiles; flags[r] is the ray's tile bits;
  * the y rows of dead rays are zero, every other row keeps its fill;
  * the canary words behind every output (and wtile_list's entries from W on) are untouched.

Inputs: sdf = 1000 (the renderer's outside value) saturates both NeuS sigmoids, so a tile of such
samples has weights of exactly 0; elsewhere a small random sdf gives alphas in (0, 1).  The tile
patterns: every ray dead, every tile nonzero, holes inside live rays, dead runs, random.

Shapes: R in {2, 8, 37 G, 4096} rounded up to whole workgroups of G = 256 / N rays, N in
{32, 128, 256}: one, four and eight tiles per ray, two rays per wave and one (N = 256), ray counts
below one workgroup of the pass, no multiple of it (37 G), and many workgroups.
"""
import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L

from live_ref import live_rays
from live_tiles_ref import live_tiles, tile_flags

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0x5A5A5A5A
PAD = 64


def _shapes():
    out = []
    for N in (32, 128, 256):
        G = 256 // N
        for R in sorted({-(-r // G) * G for r in (2, 8, 37 * G, 4096)}):
            out.append((R, N))
    return out


def _guarded(n, dtype):
    """n elements followed by PAD canary words (int32 views of the same storage)."""
    raw = torch.full((n + PAD,), CANARY, dtype=torch.int32, device=DEV)
    return raw, raw[:n].view(dtype)


def _tile_pattern(name, R, T, rng):
    r = np.arange(R)[:, None]
    j = np.arange(T)[None, :]
    if name == "none":
        return np.zeros((R, T), bool)
    if name == "all":
        return np.ones((R, T), bool)
    if name == "holes":      # tiles 0 and 2 of every other ray, the last tile of ray 1
        return ((r % 2 == 0) & (j % 2 == 0)) | ((r == 1) & (j == T - 1))
    if name == "runs":       # three live rays, three dead, the live ones lose their first tile
        return ((r // 3) % 2 == 1) & ((j > 0) | (T == 1))
    nz = rng.random((R, T)) < 0.6
    nz[rng.random(R) < 0.4] = False
    return nz


def _inputs(R, N, nz, seed):
    """Composite inputs whose tiles outside nz are all sdf = 1000 (weights exactly 0)."""
    g = torch.Generator().manual_seed(seed)
    dists = (torch.arange(N, dtype=torch.float32)[:, None] * 0.03 + 0.5 + 0.01 * torch.rand(N, R, generator=g))
    far = dists[-1] + 0.03
    ray = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    grad = torch.nn.functional.normalize(torch.randn(N, R, 3, generator=g), dim=-1)
    sdf = 0.05 * (torch.rand(N, R, generator=g) - 0.3)
    dead = torch.from_numpy(~np.repeat(nz, 32, axis=1).T.copy())     # [N][R]
    sdf[dead] = 1000.0
    t = dict(dists=dists, far=far, ray_unit=ray, ray_norm=torch.ones(R), sdf=sdf, grad=grad,
             s_var=torch.tensor([3.0]))
    return {k: v.contiguous().to(DEV) for k, v in t.items()}


def _comp(R, N, t, w):
    return L.CompositeArgs(R, N, L.ptr(t["dists"]), L.ptr(t["far"]), L.ptr(t["ray_unit"]), L.ptr(t["ray_norm"]),
                           L.ptr(t["sdf"]), L.ptr(t["grad"]), None, L.ptr(t["s_var"]), 0.5, 1, L.ptr(w))


@pytest.mark.parametrize("scan_launch", (0, 1))
@pytest.mark.parametrize("R,N", _shapes())
def test_pass_matches_the_restatements(R, N, scan_launch):
    T = N // 32
    rng = np.random.default_rng(R + N)
    raw_y, y = _guarded(N * R * 8, torch.float32)
    raw_w, w = _guarded(N * R, torch.float32)
    raw_f, flags = _guarded(R, torch.int32)
    raw_l, tl = _guarded(R * T, torch.int32)
    raw_r, tr = _guarded(R * T + 1, torch.int32)
    raw_n, nl = _guarded(1, torch.int32)
    raw_wl, wl = _guarded(R * T, torch.int32)
    raw_wr, wr = _guarded(R * T + 1, torch.int32)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)      # zeroed once
    w_ref = torch.empty(N * R, device=DEV)
    y0 = (torch.rand(N, R, 8, generator=torch.Generator().manual_seed(R)) + 0.5).to(DEV)
    zero_tiles = 0
    names = ("holes", "none", "random", "all", "runs") if R <= 512 else ("random", "holes")
    for i, name in enumerate(names):
        nz = _tile_pattern(name, R, T, rng)
        t = _inputs(R, N, nz, seed=R + N + i)
        y.copy_(y0.reshape(-1))
        raw_wl.fill_(CANARY)
        L.call("mli_composite_fwd", _comp(R, N, t, w_ref))
        L.call("mli_live_tiles", L.LiveTilesArgs(_comp(R, N, t, w), L.ptr(y), L.ptr(flags), L.ptr(tl), L.ptr(tr),
                                                 L.ptr(nl), L.ptr(wl), L.ptr(wr), L.ptr(ticket), scan_launch))
        torch.cuda.synchronize()
        assert int(ticket.cpu()) == 0, name
        assert torch.equal(w.view(torch.int32), w_ref.view(torch.int32)), name
        wn = w.view(N, R).cpu().numpy()
        got_nz = tile_flags(wn)
        assert not (got_nz & ~nz).any(), name                   # sdf = 1000 tiles are exactly zero
        ref_l, ref_r, ref_n = live_rays(wn)
        ref_wl, ref_wr = live_tiles(wn)
        assert np.array_equal(tl.cpu().numpy(), ref_l), name
        assert np.array_equal(tr.cpu().numpy(), ref_r), name
        assert int(nl.cpu()) == ref_n, name
        assert np.array_equal(wr.cpu().numpy(), ref_wr), name
        W = len(ref_wl)
        assert np.array_equal(wl[:W].cpu().numpy(), ref_wl), name
        assert bool((wl[W:] == CANARY).all()), name
        assert np.array_equal(flags.cpu().numpy(), (got_nz << np.arange(T)).sum(1)), name
        for raw in (raw_y, raw_w, raw_f, raw_l, raw_r, raw_n, raw_wl, raw_wr):
            assert bool((raw[-PAD:] == CANARY).all()), name
        live = got_nz.any(1)
        want = y0.clone()
        want[:, torch.from_numpy(~live).to(DEV)] = 0
        assert torch.equal(y.view(N, R, 8), want), name
        zero_tiles += int((~got_nz[live]).sum())
        if name == "all":
            assert got_nz.all()
    assert zero_tiles > 0 or T == 1        # all-zero tiles inside live rays were among the cases


def test_bad_arguments_are_refused():
    R, N = 8, 128
    t = _inputs(R, N, np.ones((R, 4), bool), seed=1)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)  # noqa: E731
    w, y = torch.empty(N * R, device=DEV), torch.zeros(N, R, 8, device=DEV)
    bufs = [i32(R), i32(R * 4), i32(R * 4 + 1), i32(1), i32(R * 4), i32(R * 4 + 1)]
    ok = L.LiveTilesArgs(_comp(R, N, t, w), None, *[L.ptr(b) for b in bufs], L.ptr(i32(1)), 0)
    L.call("mli_live_tiles", ok)                                # y is optional
    torch.cuda.synchronize()
    assert int(bufs[3].cpu()) == 32
    no_ticket = L.LiveTilesArgs(_comp(R, N, t, w), None, *[L.ptr(b) for b in bufs], None, 0)
    with_y = L.LiveTilesArgs(_comp(R, N, t, w), None, *[L.ptr(b) for b in bufs], L.ptr(i32(1)), 0)
    with_y.comp.y = L.ptr(y)                                    # the weights pass only
    for bad in (no_ticket, with_y):
        with pytest.raises(RuntimeError):
            L.call("mli_live_tiles", bad)
    for r, n in ((8, 192), (8, 96), (3, 128)):
        args = L.LiveTilesArgs(_comp(r, n, t, w), None, *[L.ptr(b) for b in bufs], L.ptr(i32(1)), 1)
        with pytest.raises(RuntimeError):
            L.call("mli_live_tiles", args)
