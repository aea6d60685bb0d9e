"""The heads, their backward and dW skip the rays whose composite weights are all zero (GPU).

One fused stage-b train step in deterministic mode with the elision on against off, on the same
batch and stratified uniforms: the flat gradient, every loss term and the PSNR, the composited
outputs and the parameters after AdamW must be equal (np.array_equal after ``+ 0.0``: the two
paths may differ in the sign of a zero and in nothing else -- every sum keeps its partition and
order, and what is skipped adds exact zeros).

The batches are built from one frame's rays (mli_rays over every pixel, once): a pattern says
which rays miss the bounding sphere (``outside``: sdf = 1000 at every sample, both NeuS sigmoids
saturate, every weight is exactly 0) and which hit it, centre pixels first.  A ray that hits the
sphere need not be live; the test reads the live rays back from the step's own weights and checks
the device arrays against tests/live_ref.py, and that every outside ray is dead.

Before the "on" step the buffers the skipped work would have written (y, the x0 / X / mask / dZ
images, q4, the split-K workspace) are filled with NaN (masks: all ones): equality then also
shows that no dead slot is read, and the images must still hold the fill beyond n_live_tiles.

Shapes (R, Nc, Nf; N = Nc + 4 Nf).  The BIG dW launch has 9 one-tile jobs, so its k-slices are
ceil(S / 64 / 28) * 64 samples, streamed in 32-sample stages through a ring of 4 buffers:
  (16, 64, 16)  S = 2048, N = 128: 128-sample slices = one ray each.  A dead ray is an empty slice
                (no DMA, a zero slab) and a slice next to it starts mid-image; live rays give
                4-stage ranges, and the WIDE slices (64 samples) ranges shorter than the ring.
  (64, 64, 16)  S = 8192, N = 128: 320-sample slices that straddle rays: ranges of 0 .. 10 stages.
  (32, 16, 4)   N = 32: eight rays per workgroup, the pad path with up to seven pad rays.
  (8, 128, 32)  N = 256: one ray per workgroup, no pads.
"""
import functools

import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L
from mli_nerf_amd import layout, synthetic
from mli_nerf_amd.configs import preset
from mli_nerf_amd.model import Model
from mli_nerf_amd.trainer import Trainer

from live_ref import live_rays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAME, H, W = 1, 512, 512


@functools.lru_cache(maxsize=None)
def _pixels():
    """(inside, outside): pixel indices of FRAME whose ray hits / misses the unit sphere, the hits
    ordered from the image centre outwards (mli_rays over the whole image, once)."""
    d = synthetic.make_batch(8, H, W, frame=FRAME)
    n = H * W
    f = lambda *s: torch.empty(*s, device=DEV)  # noqa: E731
    out = torch.empty(n, dtype=torch.uint8, device=DEV)
    keep = [d[k][0].contiguous().to(DEV) for k in ("intr", "pose", "pose_light")]
    bufs = [f(n, 3), f(n, 3), f(n), f(n, 3), f(n), f(n)]
    L.call("mli_rays", L.RaysArgs(L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), None, 0, n, W, 0,
                                  (L.F32 * 6)(-1, -1, -1, 1, 1, 1), *[L.ptr(b) for b in bufs], L.ptr(out)))
    torch.cuda.synchronize()
    outside = out.cpu().numpy() != 0
    idx = np.arange(n)
    dist = (idx // W - H / 2) ** 2 + (idx % W - W / 2) ** 2
    inside = idx[~outside]
    return inside[np.argsort(dist[inside], kind="stable")], idx[outside]


def _batch(hit, Nc, seed=1):
    """The training sample of FRAME with ray r on a pixel that hits (hit[r]) or misses the sphere."""
    R = len(hit)
    inside, outside = _pixels()
    d = synthetic.make_batch(R, H, W, frame=FRAME)
    idx = np.empty(R, np.int64)
    idx[hit] = inside[:int(hit.sum())]
    idx[~hit] = outside[::97][:int((~hit).sum())]
    d["ray_idx"] = torch.from_numpy(idx)[None]
    return {k: v.to(DEV) for k, v in d.items()}, synthetic.stratified_uniforms(R, Nc, seed=seed).to(DEV)


def _trainer(elide, R, Nc, Nf, deterministic=True, log2T=16):
    cfg = preset("syn_hotdog_b", rays=R, n_coarse=Nc, n_fine=Nf, log2T=log2T)
    cfg.trainer["deterministic"] = deterministic
    m = Model(cfg.model, cfg.data)
    m.load_state_dict(synthetic.make_state_dict(log2T=log2T))
    m.elide_dead_rays = elide
    tr = Trainer(cfg, is_inference=False, model=m.to(DEV))
    tr.current_iteration = 10000
    return tr


def _poison(tr, R, N):
    """Allocate the step's buffers under the engine's own names and fill them: NaN, masks all ones."""
    tr.model.prepare()
    eng = tr.model.engine
    S = R * N
    f16 = torch.float16
    bufs = dict(y=eng._buf("y", (N, R, 8)), feat=eng._buf("feat", (S * layout.K0,), f16),
                xT=eng._buf("xT", (3, 3, S * 256), f16), dzT=eng._buf("dzT", (3, 4, S * 256), f16),
                q4=eng._buf("q4", (S // 256, layout.q4_segs(N), 3, 257, 4)),
                wgrad_ws=eng._buf("wgrad_ws", (24 * 2 ** 20,)))
    for t in bufs.values():
        t.fill_(float("nan"))
    bufs["masks"] = eng._buf("masks", (3, 4, S // 32, 64, 4), torch.int32)
    bufs["masks"].fill_(-1)
    return bufs


def _step(tr, d, u):
    tr.train_step(d, u=u)
    torch.cuda.synchronize()
    comp = tr.model._last_state[4]
    out = {"grad": tr.model.flat.grad, "params": tr.model.flat.detach(), "psnr": tr.metrics["psnr"]}
    out.update({"loss_" + k: v for k, v in tr.losses.items()})
    out.update({k: comp[k] for k in ("rgb", "o_r", "o_s", "o_re")})
    return {k: v.detach().cpu().numpy() + 0.0 for k, v in out.items()}


def _on_off(hit, Nc, Nf, deterministic=True, poison=True):
    R, N = len(hit), Nc + 4 * Nf
    d, u = _batch(hit, Nc)
    off = _step(_trainer(False, R, Nc, Nf), d, u)
    assert np.isfinite(off["grad"]).all()
    tr = _trainer(True, R, Nc, Nf, deterministic)
    bufs = _poison(tr, R, N) if poison else None
    on = _step(tr, d, u)
    return tr, bufs, on, off


def _check_lists(tr, hit, N):
    """The device arrays against the restatement on the step's own weights; outside rays are dead.
    Returns (live flags, n_live_tiles)."""
    eng = tr.model.engine
    rays, dists, fld, hd, comp = tr.model._last_state
    R = len(hit)
    assert hd["tile_list"] is not None, "the fused train step did not elide"
    w = comp["weights"].cpu().numpy()
    tl, rk, n = live_rays(w)
    assert np.array_equal(hd["tile_list"].cpu().numpy(), tl)
    assert np.array_equal(hd["tile_rank"].cpu().numpy(), rk)
    assert int(hd["n_live_tiles"].cpu()) == n
    live = (w != 0).any(0)
    outside = rays["outside"].cpu().numpy() != 0
    assert np.array_equal(outside, ~hit)
    assert not live[outside].any()
    print("R %d N %d: %d hit, %d live, %d tiles processed of %d" % (R, N, hit.sum(), live.sum(), n, R * N // 32))
    return live, n


def _check_images(bufs, R, N, n):
    """Nothing was written beyond the processed tiles; everything before them was."""
    S = R * N
    tiles = S // 32
    feat = bufs["feat"].view(tiles, -1)
    assert bool(torch.isnan(feat[n:]).all()) and not bool(torch.isnan(feat[:n]).any())
    xT = bufs["xT"].view(3, 3, tiles, -1)
    assert bool(torch.isnan(xT[:, :, n:]).all()) and not bool(torch.isnan(xT[:, :, :n]).any())
    dzT = bufs["dzT"].view(3, 4, tiles, -1)   # (dZ3 is not stored: rebuilt in the weight gradient)
    assert bool(torch.isnan(dzT[:, :3, n:]).all()) and not bool(torch.isnan(dzT[:, :3, :n]).any())
    masks = bufs["masks"].view(3, 4, tiles, -1)
    assert bool((masks[:, :, n:] == -1).all())
    # live rows written (their seven outputs; the eighth column is padding), dead rows zeroed
    assert not bool(torch.isnan(bufs["y"][..., :7]).any())


def _pattern(name, R):
    r = np.arange(R)
    return {"all_live": np.ones(R, bool), "all_dead": np.zeros(R, bool), "first": r == 0, "last": r == R - 1,
            "odd": (r == 2) | (r == 3) | (r == R - 3), "runs": (r // 3) % 2 == 1,
            "alternating": r % 2 == 1}[name]


CASES = [(16, 64, 16, p) for p in ("all_live", "all_dead", "first", "last", "odd", "runs")] + [
    (64, 64, 16, "runs"), (64, 64, 16, "odd"), (32, 16, 4, "odd"), (32, 16, 4, "alternating"), (8, 128, 32, "odd"),
    (8, 128, 32, "first")]


@pytest.mark.parametrize("R,Nc,Nf,pattern", CASES)
def test_elision_is_value_identical(R, Nc, Nf, pattern):
    hit = _pattern(pattern, R)
    N = Nc + 4 * Nf
    tr, bufs, on, off = _on_off(hit, Nc, Nf)
    live, n = _check_lists(tr, hit, N)
    if pattern == "all_dead":
        assert n == 0
    for k in off:
        assert np.array_equal(on[k], off[k]), k
    if hit.any():
        assert np.abs(off["grad"]).sum() > 0
    _check_images(bufs, R, N, n)


def test_elision_with_atomic_reductions():
    """fp32 atomics reorder the split-K sums: the elided atomic gradient against the dense
    deterministic one, at the bound test_gpu_determinism.py holds that pair to."""
    hit = _pattern("runs", 64)
    tr, _, on, off = _on_off(hit, 64, 16, deterministic=False)
    _check_lists(tr, hit, 128)
    g_on, g_off = torch.from_numpy(on["grad"]), torch.from_numpy(off["grad"])
    cos = torch.nn.functional.cosine_similarity(g_on, g_off, dim=0)
    assert cos > 0.999999, float(cos)
    assert float(on["loss_total"]) == pytest.approx(float(off["loss_total"]), rel=1e-6)
    for k in ("rgb", "o_r", "o_s", "o_re"):
        assert np.array_equal(on[k], off[k]), k


def test_elision_with_stored_dz3(monkeypatch):
    """MLI_DZ3_REBUILD=0: the layer-3 dW reads the stored dZ3 image, compact like the others."""
    monkeypatch.setenv("MLI_DZ3_REBUILD", "0")
    hit = _pattern("odd", 16)
    tr, bufs, on, off = _on_off(hit, 64, 16)
    assert tr.model.engine.dz3_rebuild is False
    _, n = _check_lists(tr, hit, 128)
    for k in off:
        assert np.array_equal(on[k], off[k]), k
    dz3 = bufs["dzT"].view(3, 4, 16 * 128 // 32, -1)[:, 3]
    assert bool(torch.isnan(dz3[:, n:]).all()) and not bool(torch.isnan(dz3[:, :n]).any())


def test_n192_runs_dense():
    """256 % 192 != 0: a workgroup would hold parts of rays, so the step stays dense."""
    hit = _pattern("runs", 16)
    tr, _, on, off = _on_off(hit, 128, 16, poison=False)
    hd = tr.model._last_state[3]
    assert hd["q4"] is not None and hd["tile_list"] is None and not tr.model.engine.elides(192, True)
    for k in off:
        assert np.array_equal(on[k], off[k]), k
