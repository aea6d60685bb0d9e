"""The heads forward and backward on the nonzero tiles only, through the C ABI (GPU).

mli_rgb_fwd_args / mli_rgb_bwd_args .wtile_list + .n_wtiles_pad, mli_dw4_args.wtile_rank and
mli_live_tiles_args.n_wtiles_pad.  The rays and the h0 image of one small train step are kept; its
dists (evenly spaced with jitter), gradients and sdf are replaced so that the composite weights follow a chosen tile pattern (sdf = 1000
saturates both NeuS sigmoids: the tile's weights are exactly 0; elsewhere a small random sdf, with
inv_s = 1, no cosine annealing and random gradients shorter than 1, so that every other alpha is
positive).
Then the tail of the step runs twice on it, call by call -- mli_live_tiles, mli_rgb_fwd,
mli_composite_loss, mli_rgb_bwd, mli_dw4, mli_wgrad (deterministic) --:
  off  the new fields NULL: the ray-compact path the rest of the suite pins, the reference;
  on   the new fields set, after the x0 / X / dZ images, the q4 items and y were filled with NaN
       and the masks with ones: nothing of a skipped tile may reach a result.
torch.equal after ``+ 0.0`` on: y at the listed tiles, the composited outputs, the loss values,
dz4, every dW / db (dW4 / db4 included).  The device lists equal tests/heads_tiles_ref.py on the
weights the pass wrote, and y of every tile that is not listed is exactly 0 afterwards.

Shapes: R = 64 with N = 128, 64, 32 (T = 4, 2, 1 tiles per ray) and R = 8 with N = 256 (T = 8).
Patterns: every tile nonzero (no pads), no live ray (W = 0: every workgroup returns, dW4 = 0),
W % 8 = 1 and 7, a ray whose nonzero tiles straddle two workgroups, a ray with a single nonzero
tile in its last position, one live ray among dead ones.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L
from mli_nerf_amd import layout, synthetic

from heads_tiles_ref import padded_tiles
from live_ref import live_rays
from live_tiles_ref import tile_flags
from test_gpu_dead_rays import DEV, _trainer

pytestmark = pytest.mark.gpu
SHAPES = ((64, 64, 16), (64, 32, 8), (64, 16, 4), (8, 128, 32))        # (R, Nc, Nf): N = Nc + 4 Nf
PATTERNS = ("all", "none", "w1", "w7", "straddle", "last_single", "one_live")
PROGRESS = 0.0      # no cosine annealing: every sample's alpha is positive unless its sdf saturates


def _tiles(name, R, T):
    """[R][T] bool: the nonzero tiles of the pattern."""
    nz = np.zeros((R, T), bool)
    j = np.arange(T)
    if name == "all":
        nz[:] = True
    elif name in ("w1", "w7"):
        # the first 9 / 7 tiles in ray order among those that are not a ray's first / last tile
        keep = np.tile((j != 0) if name == "w1" else (j != T - 1), (R, 1)) | (T == 1)
        flat = np.flatnonzero(keep.reshape(-1))[:9 if name == "w1" else 7]
        nz.reshape(-1)[flat] = True
    elif name == "straddle":
        nz[0, 1:] = True                        # T - 1 entries (T = 1: the ray's only tile)
        nz[0, 0] = T == 1
        nz[1:5] = True                          # ... so a later ray crosses entry 8
    elif name == "last_single":
        nz[2, T - 1] = True
        nz[5] = True
    elif name == "one_live":
        nz[R // 2] = (j % 2 == 1) | (T == 1)
    return nz


def test_patterns_have_the_named_properties():
    """Host arithmetic on the patterns (no GPU work)."""
    for R, Nc, Nf in SHAPES:
        T = (Nc + 4 * Nf) // 32
        W = {p: int(_tiles(p, R, T).sum()) for p in PATTERNS}
        assert W["all"] == R * T and W["all"] % 8 == 0 and W["none"] == 0
        assert W["w1"] % 8 == 1 and W["w7"] % 8 == 7
        nz = _tiles("straddle", R, T)
        first = np.cumsum(nz.sum(1)) - nz.sum(1)          # a ray's first entry
        crosses = [(first[r] // 8) != ((first[r] + nz[r].sum() - 1) // 8) for r in range(R) if nz[r].any()]
        assert any(crosses) or T == 1
        assert _tiles("last_single", R, T)[2].tolist() == [False] * (T - 1) + [True]
        assert _tiles("one_live", R, T).any(1).sum() == 1


@functools.lru_cache(maxsize=None)
def _geometry(R, Nc, Nf):
    """A trainer after one fused step on a batch of rays that all hit the sphere, dense geometry."""
    tr = _trainer(True, R, Nc, Nf, log2T=14)
    tr.model.elide_outside = False               # h0 of every ray is written
    d = {k: v.to(DEV) for k, v in synthetic.make_batch(R, frame=3).items()}
    tr.train_step(d, u=synthetic.stratified_uniforms(R, Nc, seed=1).to(DEV))
    torch.cuda.synchronize()
    rays, dists, fld = tr.model._last_state[:3]
    assert not fld.get("elided") and bool(torch.isfinite(fld["h0"][:R * (Nc + 4 * Nf) * 256].float()).all())
    return tr, d, rays, dists, fld


def _i32(n, fill=0):
    return torch.full((n,), fill, dtype=torch.int32, device=DEV)


def _tail(R, Nc, Nf, nz, on):
    """The step's tail, call by call; ``on``: the new fields set, the skipped work's buffers poisoned."""
    tr, data, rays, dists, fld = _geometry(R, Nc, Nf)
    eng, m = tr.model.engine, tr.model
    N = Nc + 4 * Nf
    S, T, tiles = R * N, N // 32, R * N // 32
    nan, f16 = float("nan"), torch.float16
    g = torch.Generator().manual_seed(R + N)
    sdf = 0.05 * (torch.rand(N, R, generator=g) - 0.3)
    sdf[torch.from_numpy(~np.repeat(nz, 32, axis=1).T.copy())] = 1000.0
    # (gradients of length 0.9 in random directions: |cos| < 1, so _get_iter_cos is never 0)
    grad = 0.9 * torch.nn.functional.normalize(torch.randn(N, R, 3, generator=g), dim=-1)
    fld = dict(fld, sdf=sdf.to(DEV), grad=grad.contiguous().to(DEV))
    # (the sampler puts its fine samples on top of each other: steps of exactly 0, alphas of 0)
    dists = torch.arange(N, dtype=torch.float32)[:, None] * 0.03 + 0.5 + 0.01 * torch.rand(N, R, generator=g)
    rays = dict(rays, far=(dists[-1] + 0.03).contiguous().to(DEV))
    dists = dists.contiguous().to(DEV)
    s_var = torch.tensor([0.0], device=DEV)       # inv_s = 1: small alphas, the transmittance stays positive
    fill = nan if on else 0.0
    y = torch.full((N, R, 8), fill, device=DEV)
    feat = torch.full((S * layout.K0,), fill, dtype=f16, device=DEV)
    xT = torch.full((3, 3, S * 256), fill, dtype=f16, device=DEV)
    dzT = torch.full((3, 4, S * 256), fill, dtype=f16, device=DEV)
    masks = _i32(3 * 4 * tiles * 256, -1 if on else 0).view(3, 4, tiles, 64, 4)
    q4 = torch.full((tiles, 3, 257, 4) if on else (S // 256, layout.q4_segs(N), 3, 257, 4), fill, device=DEV)
    w = torch.full((N, R), nan, device=DEV)
    tl, tk, nl, wl, wr, npad = _i32(tiles), _i32(tiles + 1), _i32(1), _i32(tiles, -1), _i32(tiles + 1), _i32(1, -1)
    hd = dict(y=y, x0T=feat, xT=xT, masks=masks, feat=feat, q4=q4, tile_list=tl, tile_rank=tk, n_live_tiles=nl,
              wtile_list=wl, wtile_rank=wr, n_wtiles_pad=npad if on else None)
    new = (lambda t: L.ptr(t)) if on else (lambda t: None)  # noqa: E731
    # mli_live_tiles: the weights and the lists (y = NULL inside comp: the weights pass)
    comp = eng._composite_args(rays, dists, fld, dict(y=None), s_var, PROGRESS, dict(weights=w, rgb=None, o_r=None,
                                                                                      o_s=None, o_re=None))
    L.call("mli_live_tiles", L.LiveTilesArgs(comp, L.ptr(y), L.ptr(_i32(R)), L.ptr(tl), L.ptr(tk), L.ptr(nl),
                                             L.ptr(wl), L.ptr(wr), None, 1, new(npad)))
    # mli_rgb_fwd
    L.call("mli_rgb_fwd", L.RgbFwdArgs(R, N, L.ptr(rays["center"]), L.ptr(rays["ray_unit"]), L.ptr(rays["pts_light"]),
                                       L.ptr(dists), L.ptr(fld["grad"]), L.ptr(fld["h0"]), L.ptr(eng.wfwd), L.ptr(y),
                                       L.ptr(feat), L.ptr(xT), L.ptr(masks), 3, L.ptr(w), L.ptr(q4), L.ptr(tl),
                                       L.ptr(nl), new(wl), new(npad)))
    # mli_composite_loss (the engine builds its arguments; it reads y of every sample)
    lv = torch.full((8,), nan, device=DEV)
    out, dz4 = eng.composite_loss(rays, dists, fld, hd, s_var, PROGRESS, tr._loss_args(rays, fld, None, data, lv))
    dz4 = dz4.clone()
    # mli_rgb_bwd (dZ3 rebuilt in the weight gradient, as in the fused step)
    L.call("mli_rgb_bwd", L.RgbBwdArgs(R, N, L.ptr(dz4), L.ptr(eng.wbwd), L.ptr(masks), L.ptr(dzT), None, 1,
                                       L.ptr(tl), L.ptr(nl), new(wl), new(npad)))
    # mli_dw4 and mli_wgrad into one dW buffer
    dwbuf = torch.full((sum(mm * k + mm for _, _, ko in layout.HEADS for mm, k in
                            [(256, layout.K0)] + [(256, 256)] * 3 + [(ko, 256)]),), nan, device=DEV)
    grad = torch.zeros_like(m.flat)
    jobs, _, (dw4, db4, k4) = eng._wgrad_plan(dzT, None, hd, dwbuf, m.flat.detach(), grad, S, (dz4, R, N))
    d4 = L.Dw4Args(R, N, 3, L.ptr(q4), L.ptr(eng._bufs["dray"]), eng.grad_scale(R) / L.Q4_SCALE,
                   (C.c_void_p * 3)(*dw4), (C.c_void_p * 3)(*db4), (C.c_int * 3)(*k4), None, L.ptr(tk), new(wr))
    ws4 = torch.full((L.workspace("mli_dw4", d4)[0] // 4,), nan, device=DEV)
    d4.workspace = L.ptr(ws4)
    L.call("mli_dw4", d4)
    assert eng.deterministic
    eng._wgrad(S, jobs, (1, 2), hd)
    torch.cuda.synchronize()
    eng._wplans.clear()                          # (the plan holds pointers into this call's tensors)
    res = dict(lv=lv, dz4=dz4, dw=dwbuf, weights=w, **{k: out[k] for k in ("rgb", "o_r", "o_s", "o_re")})
    res = {k: v.detach().cpu() + 0.0 for k, v in res.items()}
    res["y"] = y.cpu()
    lists = {k: v.cpu().numpy() for k, v in dict(tl=tl, tk=tk, nl=nl, wl=wl, wr=wr, npad=npad).items()}
    dw4_views = [dwbuf[(p - dwbuf.data_ptr()) // 4:(p - dwbuf.data_ptr()) // 4 + k * 256].cpu() for p, k in zip(dw4, k4)]
    return res, lists, dw4_views


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("R,Nc,Nf", SHAPES)
def test_tail_is_value_identical(R, Nc, Nf, pattern):
    N = Nc + 4 * Nf
    T = N // 32
    nz = _tiles(pattern, R, T)
    off, lists_off, _ = _tail(R, Nc, Nf, nz, on=False)
    on, lists, dw4 = _tail(R, Nc, Nf, nz, on=True)
    # the weights follow the pattern, and the device lists the restatement
    wn = on["weights"].numpy()
    assert torch.equal(on["weights"], off["weights"])
    assert np.array_equal(tile_flags(wn), nz)
    ref_tl, ref_tk, ref_nl = live_rays(wn)
    ref_wl, ref_wr, ref_n = padded_tiles(wn)
    W = int(nz.sum())
    assert np.array_equal(lists["tl"], ref_tl) and np.array_equal(lists["tk"], ref_tk) and int(lists["nl"]) == ref_nl
    assert np.array_equal(lists["wr"], ref_wr) and int(lists["npad"]) == ref_n == (W + 7) // 8 * 8
    assert np.array_equal(lists["wl"][:ref_n], ref_wl) and (lists["wl"][ref_n:] == -1).all()
    assert np.array_equal(lists_off["wl"][:W], ref_wl[:W]) and (lists_off["wl"][W:] == -1).all()
    print("R %d N %d %s: W %d, %d workgroups of %d" % (R, N, pattern, W, ref_n // 8, R * T // 8))
    # y: equal at the listed tiles, exactly 0 at every other one
    listed = np.zeros(R * T, bool)
    listed[ref_tl[ref_wl[:W]]] = True
    rows = torch.from_numpy(np.repeat(listed.reshape(R, T), 32, axis=1).T.copy())     # [N][R]
    assert torch.equal(on["y"][rows][:, :7] + 0.0, off["y"][rows][:, :7] + 0.0)
    assert bool((on["y"][~rows] == 0).all())
    for k in ("rgb", "o_r", "o_s", "o_re", "lv", "dz4", "dw"):
        assert torch.equal(on[k], off[k]), k
    assert bool(torch.isfinite(off["dw"]).all())
    if W == 0:
        assert all(not bool(v.any()) for v in dw4)
    else:
        assert all(bool(v.any()) for v in dw4) and bool(off["dz4"].any())


def test_new_pointers_need_each_other():
    R, Nc, Nf = 64, 16, 4
    tr, data, rays, dists, fld = _geometry(R, Nc, Nf)
    eng, N = tr.model.engine, Nc + 4 * Nf
    S, tiles = R * N, R * N // 32
    some = _i32(tiles + 1)
    f = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)  # noqa: E731
    y, feat, xT, masks = f(S * 8), f(S * layout.K0, torch.float16), f(9 * S * 256, torch.float16), _i32(12 * tiles * 256)
    q4, w, dzT = f(tiles * 3 * 257 * 4), f(S), f(12 * S * 256, torch.float16)

    def fwd(tl, nl, wl, npad):
        return L.RgbFwdArgs(R, N, L.ptr(rays["center"]), L.ptr(rays["ray_unit"]), L.ptr(rays["pts_light"]),
                            L.ptr(dists), L.ptr(fld["grad"]), L.ptr(fld["h0"]), L.ptr(eng.wfwd), L.ptr(y), L.ptr(feat),
                            L.ptr(xT), L.ptr(masks), 3, L.ptr(w), L.ptr(q4), tl, nl, wl, npad)

    def bwd(tl, nl, wl, npad):
        return L.RgbBwdArgs(R, N, L.ptr(y), L.ptr(eng.wbwd), L.ptr(masks), L.ptr(dzT), None, 1, tl, nl, wl, npad)

    p = L.ptr(some)
    for make, name in ((fwd, "mli_rgb_fwd"), (bwd, "mli_rgb_bwd")):
        for bad in ((p, p, p, None), (p, p, None, p), (None, None, p, p)):
            with pytest.raises(RuntimeError):
                L.call(name, make(*bad))
    ptrs3 = (C.c_void_p * 3)(*[L.ptr(f(3 * 256))] * 3)
    d4 = L.Dw4Args(R, N, 3, L.ptr(q4), L.ptr(f(R * 8)), 1.0, ptrs3, ptrs3, (C.c_int * 3)(3, 3, 1), L.ptr(f(2 ** 20)),
                   None, p)
    with pytest.raises(RuntimeError):
        L.call("mli_dw4", d4)
    torch.cuda.synchronize()
