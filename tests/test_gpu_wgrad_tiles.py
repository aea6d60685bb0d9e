"""mli_wgrad alone streams only the nonzero tiles (mli_wgrad_args.wtile_rank / wtile_list; GPU).

Seeded fragment images built by hand, the jobs of the stage-b step (engine._wgrad_plan: nine
one-tile BIG jobs, three WIDE jobs over one shared x0 image), two calls on the same lists of live
rays:
  (a) without the tile lists.  The A tiles of the chosen dead tiles -- and, for the jobs that
      rebuild dZ3, their dz4 rows and mask tiles -- are exact zeros, the B tiles finite: today's
      streaming adds +-0 for them;
  (b) with the lists.  The same tiles hold NaN in A, B, dz4 and all-ones masks: one read of a
      skipped tile poisons the result.
Deterministic mode: dW and db are array_equal after ``+ 0.0``.  Atomic mode: (b) against the
deterministic (a) at the bound tests/test_gpu_determinism.py holds that pair to (cosine > 0.999999).

S = 2048 (R 16, N 128) and 8192 (R 64): BIG k-slices of 4 tiles (one ray each) and of 10 tiles
(straddling rays, the last slice ragged), WIDE slices of 2 and 4 tiles.  The dead tiles are set per
BIG slice, cycling through: none, all (an empty slice), one live tile only, the first / the last
tile dead, alternating, a dead run longer than the ring depth (4), live runs shorter than it.  With
``dead_rays`` every fourth ray is dead as well, so the images are compact and both indirections
(tile_list and wtile_list) act.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L
from mli_nerf_amd import layout

from live_ref import live_rays
from live_tiles_ref import live_tiles
from test_live_tiles_ref import weights_from_tiles

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 128
T = N // 32
KINDS = ("none", "all", "one", "first", "last", "alternating", "long_dead", "short_live")
W4_CHUNK = 1024 + 128     # one W4^T k-step of fp16 fragments + 32 fp32 biases (csrc/wgrad.hip)


def _big_slice_tiles(S):
    """Tiles per k-slice of the nine-job BIG launch: plan() of csrc/wgrad.hip."""
    return -(-(S // 64) // (256 // 9)) * 2


def _slice_pattern(kind, n, i):
    """[n] bool, True = nonzero tile, for slice i."""
    a = np.arange(n)
    if kind == "none":
        return np.ones(n, bool)
    if kind == "all":
        return np.zeros(n, bool)
    if kind == "one":
        return a == i % n
    if kind == "first":
        return a != 0
    if kind == "last":
        return a != n - 1
    if kind == "alternating":
        return a % 2 == i % 2
    if kind == "long_dead":          # L D D D D D L ... (n >= 7), else one live tile at the end
        return (a == 0) | (a >= 6) if n >= 7 else a == n - 1
    return np.resize(np.array([0, 1, 1, 0, 0, 1, 0, 1, 1, 0], bool), n)   # short_live


def _tiles(R, dead_rays):
    """[R][T] bool nonzero tiles."""
    S = R * N
    n = _big_slice_tiles(S)
    flat = np.concatenate([_slice_pattern(KINDS[i % len(KINDS)], n, i) for i in range(-(-S // 32 // n))])[:S // 32]
    nz = flat.reshape(R, T).copy()
    if dead_rays:
        nz[3::4] = False
    return nz


def test_patterns_of_the_cases():
    """Host arithmetic: the shapes give the slices and runs the docstring names."""
    assert _big_slice_tiles(2048) == 4 and _big_slice_tiles(8192) == 10
    for R in (16, 64):
        for dead_rays in (False, True):
            nz = _tiles(R, dead_rays)
            assert 0.2 < (~nz).mean() < 0.8
    flat = _tiles(64, False).reshape(-1)
    assert flat[60:70].tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 1, 1]   # slice 6: a dead run of 5 > ring depth 4
    assert flat[70:80].tolist() == [0, 1, 1, 0, 0, 1, 0, 1, 1, 0]   # slice 7: live runs of 1 and 2
    assert _slice_pattern("all", 10, 1).sum() == 0 and _slice_pattern("one", 4, 2).sum() == 1


def _images(R, nz, seed):
    """The step's operand images in compact order, random and finite, with the lists."""
    S = R * N
    tiles = S // 32
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g, device=DEV) * scale)  # noqa: E731
    w = weights_from_tiles(nz, N)
    tl, tr, n_live = live_rays(w)
    wl, wr = live_tiles(w)
    im = dict(dzT=rnd(3, 4, tiles, 8192, scale=0.05).half(), xT=rnd(3, 3, tiles, 8192).half(),
              x0T=rnd(tiles, layout.K0 * 32).half(), dz4=rnd(T, 32, R, 8, scale=0.05),
              masks=torch.randint(-2 ** 31, 2 ** 31 - 1, (3, 4, tiles, 256), generator=g, device=DEV,
                                  dtype=torch.int64).to(torch.int32))
    # W4^T chunks of the three heads: finite fp16 fragments, zero biases (the layer has none)
    w4 = torch.zeros(3, 8, W4_CHUNK, dtype=torch.uint8, device=DEV)
    w4[:, :, :1024] = rnd(3, 8, 512, scale=0.3).half().view(torch.uint8)
    im["w4"] = w4
    live_t = int(tr[-1])
    dead_pos = np.array([p for p in range(live_t) if not nz.reshape(-1)[tl[p]]], np.int64)
    lists = {k: torch.from_numpy(v.astype(np.int32)).to(DEV)
             for k, v in dict(tl=tl, tr=tr, wl=np.concatenate([wl, [0]]), wr=wr).items()}
    return im, lists, dead_pos, tl, live_t


def _fill(im, dead_pos, tl, live_t, value):
    """A copy of the images with the dead tiles (compact positions) set to ``value`` (0.0: A and
    the rebuild inputs only; NaN: B as well) and everything past the live tiles NaN."""
    nan = float("nan")
    out = {k: v.clone() for k, v in im.items()}
    dp = torch.from_numpy(dead_pos).to(DEV)
    orig = torch.from_numpy(tl[dead_pos].astype(np.int64)).to(DEV)
    out["dzT"][:, :, dp] = value
    out["masks"][:, :, dp] = 0 if value == 0.0 else -1
    dz4 = out["dz4"].permute(2, 0, 1, 3)          # [R][T][32][8] view: original tile r T + j
    flat = dz4.reshape(-1, 32, 8)                 # (a copy: permuted)
    flat[orig] = value
    dead_rays = torch.from_numpy(np.setdiff1d(np.arange(flat.shape[0]), tl[:live_t]).astype(np.int64)).to(DEV)
    flat[dead_rays] = nan                         # rays outside the compact range: never read
    out["dz4"] = flat.reshape(dz4.shape).permute(1, 2, 0, 3).contiguous()
    if value != 0.0:
        out["xT"][:, :, dp] = value
        out["x0T"][dp] = value
    for k in ("dzT", "xT"):
        out[k][:, :, live_t:] = nan
    out["x0T"][live_t:] = nan
    out["masks"][:, :, live_t:] = -1
    return out


def _jobs(im, R, config, out):
    """The stage-b jobs of one class over the images; ``out``: the fp32 dW / db buffer."""
    S = R * N
    jobs, off = [], 0
    for h, (_, _, k_out) in enumerate(layout.HEADS):
        for li in ((0,) if config == "wide" else (1, 2, 3)):
            m, k = 256, layout.K0 if li == 0 else 256
            dw, db = out[off:off + m * k], out[off + m * k:off + m * k + m]
            off += m * k + m
            if li == 0:
                jobs.append(L.frag_job(L.ptr(im["dzT"][h, 0]), L.ptr(im["x0T"]), m, k, L.ptr(dw), L.ptr(db), k, 16,
                                       layout.K0 // 16))
                continue
            j = L.frag_job(L.ptr(im["dzT"][h, li]), L.ptr(im["xT"][h, li - 1]), m, k, L.ptr(dw), L.ptr(db), k, 16, 16)
            if li == 3 and config == "big_rebuild":
                j.a_rows = None
                j.rb_dz4, j.rb_mask, j.rb_w4 = L.ptr(im["dz4"]), L.ptr(im["masks"][h, 3]), L.ptr(im["w4"][h])
                j.rb_col, j.rb_cnt, j.rb_R, j.rb_N = 3 * h, k_out, R, N
            jobs.append(j)
    return (L.WgradJob * len(jobs))(*jobs), off


def _run(im, lists, R, config, deterministic, with_tiles):
    S = R * N
    n_out = 9 * (256 * 256 + 256) if config != "wide" else 3 * (256 * layout.K0 + 256)
    out = torch.zeros(n_out, device=DEV)
    if deterministic:
        out.fill_(float("nan"))      # overwritten by the ordered reduction
    arr, used = _jobs(im, R, config, out)
    assert used == n_out
    cls = 2 if config == "wide" else 1
    jp = C.cast(arr, C.c_void_p)
    ws = None
    if deterministic:
        nbytes = L.workspace("mli_wgrad", L.WgradArgs(S, len(arr), jp, cls, 1, None))[0]
        ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    args = L.WgradArgs(S, len(arr), jp, cls, 1 if deterministic else 0, L.ptr(ws), L.ptr(lists["tr"]),
                       L.ptr(lists["tl"]))
    if with_tiles:
        args.wtile_rank, args.wtile_list = L.ptr(lists["wr"]), L.ptr(lists["wl"])
    L.call("mli_wgrad", args)
    torch.cuda.synchronize()
    return out.cpu().numpy() + 0.0


@pytest.mark.parametrize("dead_rays", (False, True))
@pytest.mark.parametrize("config", ("big_rebuild", "big_stored", "wide"))
@pytest.mark.parametrize("R", (16, 64))
def test_skipped_tiles_are_not_read(R, config, dead_rays):
    nz = _tiles(R, dead_rays)
    im, lists, dead_pos, tl, live_t = _images(R, nz, seed=R + len(config))
    assert len(dead_pos) > 0 and live_t == int(nz.any(1).sum()) * T
    zeros = _fill(im, dead_pos, tl, live_t, 0.0)
    nans = _fill(im, dead_pos, tl, live_t, float("nan"))
    ref = _run(zeros, lists, R, config, True, False)
    assert np.isfinite(ref).all() and np.abs(ref).sum() > 0
    got = _run(nans, lists, R, config, True, True)
    assert np.array_equal(got, ref)
    # with the lists the zero-filled images give the same again (the lists alone change nothing)
    assert np.array_equal(_run(zeros, lists, R, config, True, True), ref)
    atom = _run(nans, lists, R, config, False, True)
    cos = torch.nn.functional.cosine_similarity(torch.from_numpy(atom), torch.from_numpy(ref), dim=0)
    assert cos > 0.999999, float(cos)


def test_lists_need_each_other():
    R = 16
    im, lists, dead_pos, tl, live_t = _images(R, _tiles(R, False), seed=3)
    out = torch.zeros(3 * (256 * layout.K0 + 256), device=DEV)
    arr, _ = _jobs(im, R, "wide", out)
    jp = C.cast(arr, C.c_void_p)
    for kw in (dict(wtile_rank=L.ptr(lists["wr"])), dict(wtile_list=L.ptr(lists["wl"])),
               dict(wtile_rank=L.ptr(lists["wr"]), wtile_list=L.ptr(lists["wl"]))):      # no live-ray lists
        args = L.WgradArgs(R * N, len(arr), jp, 2, 0, None, **kw)
        with pytest.raises(RuntimeError):
            L.call("mli_wgrad", args)
