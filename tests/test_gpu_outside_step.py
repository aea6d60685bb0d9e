"""The FIELD pass of the fused stage-b train step skips the rays outside the bounds (GPU).

Deterministic train steps with the elision on (Model.elide_outside = True) against off, on the
same batches and stratified uniforms: the flat gradient, the parameters after AdamW, every loss
term, the PSNR, the composited outputs and the weights must be equal (np.array_equal after
``+ 0.0``), and so must every entry of the reference output dict -- gradients, hessians and dists
of every ray included -- which the elided state gives only after RenderEngine.densify.

The batches are test_gpu_dead_rays.py's: rays of one frame placed on pixels that hit or miss the
bounding sphere by a mask.  R = 64 rays of N = 32 samples (Nc 16, Nf 4), a 2^14 table."""
import numpy as np
import pytest
import torch

from test_gpu_dead_rays import _batch, _trainer

pytestmark = pytest.mark.gpu
R, NC, NF = 64, 16, 4
N = NC + 4 * NF


def _hit(name):
    r = np.arange(R)
    return {"none": np.zeros(R, bool), "one": r == 5, "some": np.random.default_rng(40).random(R) < 0.4,
            "all": np.ones(R, bool)}[name]


def _make(switch, fused_tail=True):
    tr = _trainer(True, R, NC, NF, log2T=14)
    tr.model.elide_outside = switch
    tr.fused_tail = fused_tail
    return tr


def _np(v):
    return v.detach().cpu().numpy() + 0.0


def _result(tr, outputs=None):
    """What the step left its caller; ``outputs``: the reference dict (None: not asked for)."""
    torch.cuda.synchronize()
    comp = tr.model._last_state[4]
    out = {"grad": tr.model.flat.grad, "params": tr.model.flat.detach(), "psnr": tr.metrics["psnr"]}
    out.update({"loss_" + k: v for k, v in tr.losses.items()})
    out.update({k: comp[k] for k in ("rgb", "o_r", "o_s", "o_re", "weights")})
    if outputs is not None:
        assert outputs["hessians"] is not None
        out.update({"out_" + k: v for k, v in outputs.items() if v is not None})
    return {k: _np(v) for k, v in out.items()}


def _same(on, off, what):
    assert set(on) == set(off), what
    for k in off:
        assert np.array_equal(on[k], off[k]), (what, k)
    assert np.isfinite(off["grad"]).all(), what


@pytest.mark.parametrize("pattern", ["none", "one", "some", "all"])
def test_step_is_value_identical(pattern):
    hit = _hit(pattern)
    d, u = _batch(hit, NC)
    res = {}
    for switch in (False, True):
        tr = _make(switch)
        if switch:
            # the images the skipped rays' tiles live in hold NaN: equality then also shows that
            # nobody reads them -- the pad rays of the heads' last workgroup included
            tr.model.prepare()
            eng = tr.model.engine
            eng._buf("h0", (R * N * 256,), torch.float16).fill_(float("nan"))
            eng._buf("enc5", (R * N * 640,), torch.float16).fill_(float("nan"))
        tr.train_step(d, u=u)
        st = tr.model._last_state
        assert bool(st[2]["elided"]) == switch, "the FIELD pass of the fused step %s" % (
            "did not take the list" if switch else "took a list")
        assert st[3]["tile_list"] is not None
        first = _result(tr)
        full = _result(tr, tr.model.outputs(st))    # the densify path
        assert not st[2]["elided"]
        _same({k: full[k] for k in first}, first, "densify changed the step's results")
        res[switch] = full
        outside = st[0]["outside"].cpu().numpy() != 0
        assert np.array_equal(outside, ~hit)
    _same(res[True], res[False], pattern)
    if hit.any():
        assert np.abs(res[False]["grad"]).sum() > 0
    g = res[False]["out_gradients"][0]
    if (~hit).any():   # the dense gradients of the outside rays are not the rows the elided pass leaves
        assert np.abs(g[~hit]).sum() > 0


def _pipeline(switch):
    """Four steps, two batches ahead (three lanes), gate 'heads'; step 1 returns the outputs, step
    3's are asked for afterwards, steps 0 and 2 leave their lanes elided."""
    tr = _make(switch)
    tr.prefetch_gate, tr.prefetch_depth = "heads", 2
    batches = [_batch(_hit(p), NC, seed=i + 1) for i, p in enumerate(("some", "none", "all", "one", "some", "all"))]
    hist = []
    for j in range(2):
        tr.prefetch(batches[j][0], u=batches[j][1])
    for k in range(4):
        out = tr.train_step(batches[k][0], return_outputs=(k == 1))
        if k == 3:
            assert bool(tr.model._last_state[2]["elided"]) == switch
            out = tr.model.outputs(tr.model._last_state)
        hist.append(_result(tr, out))
        tr.prefetch(batches[k + 2][0], u=batches[k + 2][1])
    torch.cuda.synchronize()
    return hist


def test_prefetched_steps_are_value_identical():
    on, off = _pipeline(True), _pipeline(False)
    for k, (a, b) in enumerate(zip(on, off)):
        _same(a, b, "step %d" % k)
    assert "out_gradients" in on[1] and "out_gradients" in on[3] and "out_gradients" not in on[0]


def test_unfused_tail_after_an_elided_prefetch_densifies():
    """fused_tail turned off between prefetch and train_step: the heads then read every ray."""
    d, u = _batch(_hit("some"), NC)
    ref = _make(True, fused_tail=False)
    ref.train_step(d, u=u)
    assert not ref.model._last_state[2]["elided"] and ref.model._last_state[3]["tile_list"] is None
    want = _result(ref, ref.model.outputs(ref.model._last_state))
    tr = _make(True)
    tr.prefetch(d, u=u)
    assert tr._pending[0][4]["elided"]
    tr.fused_tail = False
    tr.train_step(d)
    st = tr.model._last_state
    assert not st[2]["elided"] and st[3]["tile_list"] is None
    _same(_result(tr, tr.model.outputs(st)), want, "unfused tail")


def test_switch(monkeypatch):
    monkeypatch.setenv("MLI_ELIDE_OUTSIDE", "0")
    d, u = _batch(_hit("some"), NC)
    tr = _make(None)
    tr.train_step(d, u=u)
    assert tr.model.engine.elide_outside is False and not tr.model._last_state[2]["elided"]
    monkeypatch.delenv("MLI_ELIDE_OUTSIDE")
    tr = _make(None)
    tr.train_step(d, u=u)
    assert tr.model.engine.elide_outside is True and tr.model._last_state[2]["elided"]
