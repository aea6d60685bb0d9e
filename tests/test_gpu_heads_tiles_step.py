"""Two fused stage-b train steps with the heads on the nonzero tiles against every live tile (GPU).

RenderEngine.skip_zero_tiles_heads / Model.skip_zero_tiles_heads / MLI_SKIP_ZERO_TILES_HEADS: the
heads forward and backward take the entries of the padded nonzero-tile list, eight to a workgroup,
and mli_dw4 forms the per-ray Q from one q4 item per tile.  Both arms elide the dead rays, skip
the zero tiles in the dW kernels and run in deterministic mode at R = 64, N = 128, log2T = 14 on the
batches of tests/test_gpu_zero_tiles_step.py (rays spread to the rim of the sphere, so live rays
have all-zero tiles).  Losses, PSNR, flat gradient, composited outputs and the parameters after
AdamW of both steps must be equal (np.array_equal after ``+ 0.0``: what is skipped adds +-0 and
every sum keeps its partition and order).  The same with the geometry prefetched two batches ahead.
"""
import functools

import numpy as np
import pytest
import torch

from heads_tiles_ref import padded_tiles
from live_tiles_ref import tile_flags
from test_gpu_dead_rays import DEV, _pattern, _trainer
from test_gpu_zero_tiles_step import _batch

pytestmark = pytest.mark.gpu
R, NC, NF, LOG2T = 64, 64, 16, 14
N = NC + 4 * NF


def _make(switch):
    tr = _trainer(True, R, NC, NF, log2T=LOG2T)
    tr.model.skip_zero_tiles_heads = switch
    return tr


def _result(tr):
    torch.cuda.synchronize()
    comp = tr.model._last_state[4]
    out = {"grad": tr.model.flat.grad, "params": tr.model.flat.detach(), "psnr": tr.metrics["psnr"]}
    out.update({"loss_" + k: v for k, v in tr.losses.items()})
    out.update({k: comp[k] for k in ("rgb", "o_r", "o_s", "o_re", "weights")})
    return {k: v.detach().cpu().numpy() + 0.0 for k, v in out.items()}


def _batches():
    return [_batch(_pattern(p, R), NC, seed=i + 1) for i, p in enumerate(("all_live", "runs", "odd", "all_live"))]


def _check_lists(tr, switch):
    """The step took the path the switch names; on: the device lists equal the restatement on the
    step's own weights.  Returns (tiles of live rays, all-zero ones among them)."""
    hd, comp = tr.model._last_state[3], tr.model._last_state[4]
    assert hd["tile_list"] is not None and hd["wtile_list"] is not None
    assert (hd["n_wtiles_pad"] is not None) == switch and tr.model.engine.skip_zero_tiles_heads == switch
    nz = tile_flags(comp["weights"].cpu().numpy())
    live = nz.any(1)
    if switch:
        wl, wr, n = padded_tiles(comp["weights"].cpu().numpy())
        assert int(hd["n_wtiles_pad"].cpu()) == n
        assert np.array_equal(hd["wtile_list"].cpu().numpy()[:n], wl)
        assert np.array_equal(hd["wtile_rank"].cpu().numpy(), wr)
        assert tuple(hd["q4"].shape) == (R * N // 32, 3, 257, 4)
    return int(live.sum()) * nz.shape[1], int((~nz[live]).sum())


@functools.lru_cache(maxsize=None)
def _serial(switch):
    tr = _make(switch)
    hist, tiles, zero = [], 0, 0
    for d, u in _batches()[:2]:
        tr.train_step(d, u=u)
        hist.append(_result(tr))
        t, z = _check_lists(tr, switch)
        tiles, zero = tiles + t, zero + z
    return hist, tiles, zero


def _same(on, off, what):
    assert set(on) == set(off), what
    for k in off:
        assert np.array_equal(on[k], off[k]), (what, k)
    assert np.isfinite(off["grad"]).all() and np.abs(off["grad"]).sum() > 0, what


def test_two_steps_are_value_identical():
    (on, tiles, zero), (off, _, _) = _serial(True), _serial(False)
    print("all-zero tiles of live rays: %d of %d" % (zero, tiles))
    assert zero >= 0.05 * tiles, (zero, tiles)      # the heads really left tiles out
    for k, (a, b) in enumerate(zip(on, off)):
        _same(a, b, "step %d" % k)


def test_switch_needs_the_dw_skip():
    """skip_zero_tiles off: the dW kernels stream every live tile, so the heads write every one."""
    tr = _make(True)
    tr.model.skip_zero_tiles = False
    d, u = _batches()[0]
    tr.train_step(d, u=u)
    hd = tr.model._last_state[3]
    assert hd["wtile_list"] is None and hd["n_wtiles_pad"] is None
    _same(_result(tr), _serial(False)[0][0], "skip_zero_tiles off")


def _pipeline(switch):
    """Two steps with the geometry two batches ahead (three lanes), gate 'heads'."""
    tr = _make(switch)
    tr.prefetch_gate, tr.prefetch_depth = "heads", 2
    batches = _batches()
    hist = []
    for j in range(2):
        tr.prefetch(batches[j][0], u=batches[j][1])
    for k in range(2):
        tr.train_step(batches[k][0])
        hist.append(_result(tr))
        _check_lists(tr, switch)
        tr.prefetch(batches[k + 2][0], u=batches[k + 2][1])
    torch.cuda.synchronize()
    return hist


def test_prefetched_steps_are_value_identical():
    on, off = _pipeline(True), _pipeline(False)
    for k, (a, b) in enumerate(zip(on, off)):
        _same(a, b, "prefetched step %d" % k)
