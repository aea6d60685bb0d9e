"""mli_inside_list and the FIELD pass of mli_sdf with its list, through the C ABI (GPU).

For every shape and outside pattern the FIELD pass runs twice on the same points: dense (no list)
and with the list of mli_inside_list.  Every output buffer is filled with NaN beforehand (the fp16
images h0 and enc with a NaN bit pattern) and has a canary tail.  Required, all bit for bit:
the rows (sdf, grad, hess) and the tiles (h0, enc) of the rays inside the bounds equal the dense
call's; the rows of the rays outside them are (outside_val, 0, 0); their h0 / enc tiles still hold
the fill; the canaries are intact; inside_list / n_inside equal tests/inside_ref.py.  The outside
flags are patterns, not geometry: the kernels read nothing else about a ray's bounds.  With
n_pad > 0 the first n_pad outside rays count as evaluated: their rows and tiles are the dense
call's too (the heads may process them as pads of their last workgroup)."""
import functools

import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L
from mli_nerf_amd import synthetic
from mli_nerf_amd.configs import preset

from inside_ref import inside_list, patterns, tile_map

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
NAN16 = 0x7E00  # an fp16 NaN
H0_TILE, ENC_TILE = 16 * 64 * 8, 5 * 8 * 64 * 8  # halves per 32-sample tile


@functools.lru_cache(maxsize=None)
def _engine():
    from mli_nerf_amd.model import Model
    log2T = 14
    cfg = preset("syn_hotdog_b", rays=64, n_coarse=16, n_fine=4, log2T=log2T)
    m = Model(cfg.model, cfg.data)
    m.load_state_dict(synthetic.make_state_dict(log2T=log2T))
    m = m.to(DEV).train()
    m.prepare()
    return m, m.engine


@functools.lru_cache(maxsize=None)
def _points(R, N):
    g = torch.Generator().manual_seed(100 * R + N)
    center = (torch.rand(R, 3, generator=g) - 0.5) * 0.6
    unit = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    dists = torch.rand(N, R, generator=g).sort(0).values
    return center.to(DEV), unit.to(DEV), dists.contiguous().to(DEV)


def _alloc(n, dtype):
    t = torch.empty(n + CANARY, dtype=dtype, device=DEV)
    t.fill_(float("nan") if dtype == torch.float32 else NAN16 if dtype == torch.int16 else -7)
    return t


def _intact(t, n):
    tail = t[n:]
    if t.dtype == torch.float32:
        return bool(torch.isnan(tail).all())
    return bool((tail == (NAN16 if t.dtype == torch.int16 else -7)).all())


def _field(R, N, outside, use_list, with_hessian=True, explicit_null=False, n_pad=0):
    """One FIELD call on fresh NaN-filled buffers -> dict of the buffers (with their tails)."""
    _, eng = _engine()
    center, unit, dists = _points(R, N)
    S, tiles = R * N, R * N // 32
    out = torch.from_numpy(outside.astype(np.uint8)).to(DEV)
    b = dict(sdf=_alloc(S, torch.float32), grad=_alloc(3 * S, torch.float32),
             hess=_alloc(3 * S, torch.float32) if with_hessian else None,
             h0=_alloc(tiles * H0_TILE, torch.int16), enc=_alloc(tiles * ENC_TILE, torch.int16),
             inside_list=_alloc(R, torch.int32), n_inside=_alloc(1, torch.int32))
    lists = ()
    if use_list:
        L.call("mli_inside_list", L.InsideListArgs(R, N, n_pad, L.ptr(out), L.ptr(b["inside_list"]),
                                                   L.ptr(b["n_inside"]),
                                                   eng.cfg.outside_val, L.ptr(b["sdf"]), L.ptr(b["grad"]),
                                                   L.ptr(b["hess"])))
        lists = (L.ptr(b["inside_list"]), L.ptr(b["n_inside"]))
    elif explicit_null:
        lists = (None, None)
    L.call("mli_sdf", L.SdfArgs(1, R, N, L.ptr(center), L.ptr(unit), L.ptr(dists), L.ptr(out), L.ptr(eng.table16),
                                eng.levels, L.ptr(eng.wsdf), eng.eps, eng.grad_den, eng.hess_den,
                                eng.cfg.outside_val, 1 if with_hessian else 0, L.ptr(b["sdf"]), L.ptr(b["grad"]),
                                L.ptr(b["hess"]), L.ptr(b["h0"]), L.ptr(b["enc"]), int(eng.active_levels), *lists))
    torch.cuda.synchronize()
    return b


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check(R, N, name, outside, with_hessian=True, n_pad=0):
    _, eng = _engine()
    S, tiles, T = R * N, R * N // 32, N // 32
    dense = _field(R, N, outside, False, with_hessian)
    lst = _field(R, N, outside, True, with_hessian, n_pad=n_pad)
    sizes = dict(sdf=S, grad=3 * S, hess=3 * S, h0=tiles * H0_TILE, enc=tiles * ENC_TILE, inside_list=R, n_inside=1)
    for k, n in sizes.items():
        for b in (dense, lst):
            if b[k] is not None:
                assert _intact(b[k], n), (name, k, "canary")
    # the lists
    want_list, want_n = inside_list(outside, n_pad)
    assert int(lst["n_inside"][0].cpu()) == want_n, name
    assert np.array_equal(lst["inside_list"][:R].cpu().numpy(), want_list), name
    # the dense call wrote everything
    for k in ("sdf", "grad", "hess"):
        if dense[k] is not None:
            assert not bool(torch.isnan(dense[k][:sizes[k]]).any()), (name, k)
    # the evaluated rays: inside the bounds, or one of the first n_pad outside them (those get the
    # dense pass's rows, sdf = outside_val and the real gradients, and tiles)
    ins = torch.from_numpy(~outside | (np.cumsum(outside) <= n_pad)).to(DEV)
    outv = torch.tensor(eng.cfg.outside_val, device=DEV)
    # rows, [N][R] (x 3)
    for k, w in (("sdf", 1), ("grad", 3), ("hess", 3)):
        if lst[k] is None:
            continue
        a = _bits(lst[k][:sizes[k]]).view(N, R, w)
        d = _bits(dense[k][:sizes[k]]).view(N, R, w)
        assert torch.equal(a[:, ins], d[:, ins]), (name, k, "inside rows")
        want = _bits(outv if k == "sdf" else torch.zeros((), device=DEV))
        assert bool((a[:, ~ins] == want).all()), (name, k, "outside rows")
    # tiles, addressed by the original tile
    tin = torch.zeros(tiles, dtype=torch.bool)
    tin[torch.from_numpy(tile_map(outside, N, n_pad))] = True
    assert int(tin.sum()) == want_n * T
    tin = tin.to(DEV)
    for k, per in (("h0", H0_TILE), ("enc", ENC_TILE)):
        a = lst[k][:sizes[k]].view(tiles, per)
        d = dense[k][:sizes[k]].view(tiles, per)
        assert torch.equal(a[tin], d[tin]), (name, k, "inside tiles")
        assert bool((a[~tin] == NAN16).all()), (name, k, "outside tiles were written")
        assert not bool((d == NAN16).any()), (name, k, "the dense call left fill")


@pytest.mark.parametrize("R", [1, 5, 37, 64])
@pytest.mark.parametrize("N", [32, 64, 128])
def test_list_mode_matches_dense(R, N):
    for name, outside in patterns(R).items():
        _check(R, N, name, outside)


@pytest.mark.parametrize("R,N,n_pad", [(37, 32, 7), (5, 32, 7), (64, 128, 1), (37, 64, 3)])
def test_pad_rays_are_evaluated(R, N, n_pad):
    for name, outside in patterns(R).items():
        _check(R, N, name, outside, n_pad=n_pad)


def test_without_hessian():
    _check(37, 64, "draw60", patterns(37)["draw60"], with_hessian=False)


def test_null_list_is_the_dense_call():
    outside = patterns(37)["draw60"]
    a = _field(37, 64, outside, False)
    b = _field(37, 64, outside, False, explicit_null=True)
    for k in ("sdf", "grad", "hess", "h0", "enc"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_rejects_partial_tiles_and_half_lists():
    _, eng = _engine()
    R = 8
    with pytest.raises(RuntimeError):
        _field(R, 48, patterns(R)["alternating"], True)
    center, unit, dists = _points(R, 32)
    out = torch.zeros(R, dtype=torch.uint8, device=DEV)
    bufs = [torch.empty(n, device=DEV) for n in (R * 32, 3 * R * 32, 3 * R * 32)]
    img = [torch.empty(n, dtype=torch.int16, device=DEV) for n in (R * H0_TILE, R * ENC_TILE)]
    il = torch.zeros(R, dtype=torch.int32, device=DEV)

    def args(mode, lists):
        return L.SdfArgs(mode, R, 32, L.ptr(center), L.ptr(unit), L.ptr(dists), L.ptr(out), L.ptr(eng.table16),
                         eng.levels, L.ptr(eng.wsdf), eng.eps, eng.grad_den, eng.hess_den, eng.cfg.outside_val, 1,
                         *[L.ptr(t) for t in bufs + img], int(eng.active_levels), *lists)
    with pytest.raises(RuntimeError):   # one of the two arrays
        L.call("mli_sdf", args(1, (L.ptr(il), None)))
    with pytest.raises(RuntimeError):   # the sampling rounds take no list
        L.call("mli_sdf", args(0, (L.ptr(il), L.ptr(il))))
    with pytest.raises(RuntimeError):   # rows without sdf
        L.call("mli_inside_list", L.InsideListArgs(R, 32, 0, L.ptr(out), L.ptr(il), L.ptr(il), 1000.0, None,
                                                   L.ptr(bufs[1]), None))
    torch.cuda.synchronize()
