"""dZ3 rebuilt inside the layer-3 weight gradient (ABI 18; GPU).

dZ3 = mask3 . (W4^T dz4) has rank <= 3 per head.  With the engine's ``dz3_rebuild`` switch on and
dz4 at hand (the fused train step) mli_rgb_bwd does not store the three dZ3 images
(mli_rgb_bwd_args.skip_dz3) and the layer-3 jobs of mli_wgrad rebuild their A operand in LDS from
the sample's dz4 row, the ReLU mask bits and the W4^T fragments (mli_wgrad_job.rb_*), by the
instruction sequence of mli_rgb_bwd's layer-3 phase on the same inputs: the same fp16 fragments,
so every gradient is bit-identical to the stored path (deterministic mode: fixed-order sums).

The BIG launch of stage b holds 9 one-tile jobs, so its k-slices are ceil(S / 64 / 28) * 64
samples (mli_wgrad's plan(), one workgroup per CU) and a slice is streamed in 32-sample stages
through a ring of 4 buffers, 3 in flight.  The shapes (R, Nc, Nf; N = Nc + 4 Nf):

  (32, 16, 4)    S = 1024   64-sample slices: 2 stages, fewer than the ring's prologue issues, so
                            the clamped dummy refetches (and a rebuild past the slice end) run
  (64, 16, 4)    S = 2048   128-sample slices: 4 stages, every ring buffer used once
  (232, 16, 4)   S = 7424   320-sample slices, the last one ragged (64 samples)
  (96, 32, 8)    S = 6144   256-sample slices: 8 stages, the ring wraps
  (16, 64, 16)   S = 2048   the workload's N = 128
  (32, 24, 4)    S = 1280   N = 40: 32-sample tiles straddle two rays (and PQ falls back)
"""
import pytest
import torch

from mli_nerf_amd import _lib as L
from mli_nerf_amd import synthetic
from mli_nerf_amd.configs import preset
from mli_nerf_amd.model import Model
from mli_nerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [(32, 16, 4), (64, 16, 4), (232, 16, 4), (96, 32, 8), (16, 64, 16), (32, 24, 4)]


def _trainer(rebuild, R, Nc, Nf, pq=True, deterministic=True, log2T=16):
    cfg = preset("syn_hotdog_b", rays=R, n_coarse=Nc, n_fine=Nf, log2T=log2T)
    cfg.trainer["deterministic"] = deterministic
    m = Model(cfg.model, cfg.data)
    m.load_state_dict(synthetic.make_state_dict(log2T=log2T))
    m.pq = pq
    m.dz3_rebuild = rebuild
    tr = Trainer(cfg, is_inference=False, model=m.to(DEV))
    tr.current_iteration = 10000
    return tr


def _step(tr, R, Nc, seed=1):
    d = {k: v.to(DEV) for k, v in synthetic.make_batch(R, frame=seed).items()}
    u = synthetic.stratified_uniforms(R, Nc, seed=seed).to(DEV)
    tr.train_step(d, u=u)
    torch.cuda.synchronize()
    return tr.model.flat.grad.clone()


def _big_slices(S):
    """(samples per k-slice, slices) of the stage-b BIG launch: plan() of csrc/wgrad.hip."""
    want = 256 // 9
    k_split = -(-(S // 64) // want) * 64
    return k_split, -(-S // k_split)


def test_slice_shapes_of_the_cases():
    """The shapes exercise what the docstring says of them (host arithmetic only)."""
    got = {(R, Nc, Nf): _big_slices(R * (Nc + 4 * Nf)) for R, Nc, Nf in CASES}
    assert got[(32, 16, 4)] == (64, 16)          # 2 stages < the 3 the prologue issues
    assert got[(64, 16, 4)] == (128, 16)
    assert got[(232, 16, 4)] == (320, 24) and 7424 - 23 * 320 == 64   # ragged last slice
    assert got[(96, 32, 8)] == (256, 24)         # 8 stages > 4 buffers
    assert got[(16, 64, 16)] == (128, 16)
    assert got[(32, 24, 4)] == (64, 20) and (24 + 4 * 4) % 32 != 0


def _on_off(R, Nc, Nf, pq):
    ta, tb = _trainer(True, R, Nc, Nf, pq), _trainer(False, R, Nc, Nf, pq)
    ga, gb = _step(ta, R, Nc), _step(tb, R, Nc)
    assert float(gb.abs().sum()) > 0 and bool(torch.isfinite(gb).all())
    assert torch.equal(ga, gb)                                   # the whole flat gradient
    assert torch.equal(ta.model.flat.detach(), tb.model.flat.detach())   # and the parameters after the step
    return ta, tb


@pytest.mark.parametrize("R,Nc,Nf", CASES)
def test_rebuild_is_bit_identical(R, Nc, Nf):
    ta, tb = _on_off(R, Nc, Nf, True)
    N = Nc + 4 * Nf
    assert (ta.model.engine._bufs.get("q4") is not None) == (N % 32 == 0)


def test_rebuild_without_pq():
    _on_off(96, 32, 8, False)


def test_rebuild_with_atomic_reductions():
    """fp32 atomics reorder the split-K sums: per tensor, the rebuild-on atomic gradient within
    1e-5 relative of the ordered (deterministic) one.  The stored path's own distance is printed
    beside it."""
    R, Nc, Nf = 96, 32, 8
    ref = _step(_trainer(False, R, Nc, Nf), R, Nc)
    tr = _trainer(True, R, Nc, Nf, deterministic=False)
    g_on = _step(tr, R, Nc)
    g_off = _step(_trainer(False, R, Nc, Nf, deterministic=False), R, Nc)
    worst = 0.0
    for name, shape, off, n in tr.model._trainable_items():
        r = ref[off:off + n]
        d_on = float((g_on[off:off + n] - r).norm() / r.norm().clamp_min(1e-30))
        d_off = float((g_off[off:off + n] - r).norm() / r.norm().clamp_min(1e-30))
        print("%-44s rebuild %.3e  stored %.3e" % (name, d_on, d_off))
        worst = max(worst, d_on)
    assert worst < 1e-5, worst


def test_rgb_bwd_skip_dz3_leaves_the_layer3_images():
    """mli_rgb_bwd called directly on a train step's own inputs, dzT prefilled with a sentinel:
    skip_dz3 leaves every layer-3 image untouched and writes dZ0..dZ2 bit-identically."""
    R, Nc, Nf = 64, 16, 4
    N = Nc + 4 * Nf
    S = R * N
    tr = _trainer(True, R, Nc, Nf)
    _step(tr, R, Nc)
    eng = tr.model.engine
    hd = tr.model._last_state[3]
    dz4 = eng._bufs["dz4"]
    out = []
    for skip in (0, 1):
        dzT = torch.full((3, 4, S * 256), 0x7BFF, dtype=torch.int16, device=DEV)
        L.call("mli_rgb_bwd", L.RgbBwdArgs(R, N, L.ptr(dz4), L.ptr(eng.wbwd), L.ptr(hd["masks"]), L.ptr(dzT),
                                           None, skip))
        torch.cuda.synchronize()
        out.append(dzT)
    off, on = out
    assert torch.equal(on[:, :3], off[:, :3])
    assert bool((on[:, 3] == 0x7BFF).all())
    assert not bool((off[:, 3] == 0x7BFF).all()) and bool((off[:, :3] != 0x7BFF).any())
    # and the train step with the switch on takes that path: a second step leaves a sentinel in
    # the engine's own layer-3 images and gives the gradient of the first
    g1 = tr.model.flat.grad.clone()
    own = eng._bufs["dzT"][:3 * 4 * S * 256].view(torch.int16).view(3, 4, S * 256)
    own.fill_(0x7BFF)
    tr2 = _trainer(True, R, Nc, Nf)
    assert torch.equal(_step(tr2, R, Nc), g1)
    _step(tr, R, Nc)
    assert bool((own[:, 3] == 0x7BFF).all()) and not bool((own[:, :3] == 0x7BFF).all())
