"""The sampling rounds of the fused stage-b train step skip the rays outside the bounds (GPU).

Deterministic train steps in three arms -- the sampling elision on (the default), off (the FIELD
pass alone skips those rays: Model.elide_outside_sampling = False) and everything off
(Model.elide_outside = False) -- on the same batches and stratified uniforms: the flat gradient,
the parameters after AdamW, every loss term, the PSNR, the composited outputs and the weights must
be equal across the arms (np.array_equal after ``+ 0.0``), and so must every entry of the reference
output dict, the dists of every ray included, which an elided state gives after
RenderEngine.densify has re-run the dense sampler and the dense FIELD pass.

Before each step every sampler lane buffer, h0 and enc5 hold NaN: equality then also shows that
nobody reads what the skipped rays' rounds would have written.  The batches are
test_gpu_dead_rays.py's; R = 64 rays of N = 32 samples (Nc 16, Nf 4, seven pad rays), a 2^14 table."""
import numpy as np
import pytest
import torch

from test_gpu_dead_rays import _batch, _trainer
from test_gpu_outside_step import N, NC, NF, R, _hit, _result, _same

pytestmark = pytest.mark.gpu
ARMS = {"sampling": (True, True), "field": (True, False), "off": (False, False)}
SAMPLER_BUFS = ("d_coarse", "s_coarse", "d_m0", "d_m1", "s_m0", "s_m1", "d_f0", "d_f1", "s_f0", "s_f1", "dists")


def _make(arm):
    tr = _trainer(True, R, NC, NF, log2T=14)
    tr.model.elide_outside, tr.model.elide_outside_sampling = ARMS[arm]
    return tr


def _poison(eng):
    """NaN into the sampler's buffers and the FIELD images of the engine's current lane."""
    for k in SAMPLER_BUFS:
        eng._buf(k, (N, R)).fill_(float("nan"))
    eng._buf("h0", (R * N * 256,), torch.float16).fill_(float("nan"))
    eng._buf("enc5", (R * N * 640,), torch.float16).fill_(float("nan"))


@pytest.mark.parametrize("pattern", ["none", "one", "some", "all"])
def test_step_is_value_identical_across_the_arms(pattern):
    hit = _hit(pattern)
    d, u = _batch(hit, NC)
    res = {}
    for arm, (field, sampling) in ARMS.items():
        tr = _make(arm)
        tr.model.prepare()
        _poison(tr.model.engine)
        tr.train_step(d, u=u)
        st = tr.model._last_state
        assert bool(st[2]["elided"]) == field and bool(st[2]["sampling_elided"]) == sampling, arm
        assert st[3]["tile_list"] is not None
        first = _result(tr)
        full = _result(tr, tr.model.outputs(st))    # the densify path: dense sampler, dense FIELD
        assert not st[2]["elided"] and not st[2]["sampling_elided"]
        _same({k: full[k] for k in first}, first, "densify changed the step's results (%s)" % arm)
        assert "out_dists" in full and np.isfinite(full["out_dists"]).all(), arm
        res[arm] = full
    for arm in ("sampling", "field"):
        _same(res[arm], res["off"], (pattern, arm))
    if hit.any():
        assert np.abs(res["off"]["grad"]).sum() > 0


def _pipeline(arm):
    """Four steps, two batches ahead (three lanes), gate 'heads'; step 1 returns the outputs, step
    3's are asked for afterwards, steps 0 and 2 leave their lanes elided.  Every lane is poisoned
    before its first use."""
    tr = _make(arm)
    tr.prefetch_gate, tr.prefetch_depth = "heads", 2
    tr.model.prepare()
    eng = tr.model.engine
    for lane in range(3):
        with eng.lane(("pf", lane), geometry_only=True):
            _poison(eng)
    batches = [_batch(_hit(p), NC, seed=i + 1) for i, p in enumerate(("some", "none", "all", "one", "some", "all"))]
    hist = []
    for j in range(2):
        tr.prefetch(batches[j][0], u=batches[j][1])
    for k in range(4):
        out = tr.train_step(batches[k][0], return_outputs=(k == 1))
        if k == 3:
            assert bool(tr.model._last_state[2]["sampling_elided"]) == ARMS[arm][1]
            out = tr.model.outputs(tr.model._last_state)
        hist.append(_result(tr, out))
        tr.prefetch(batches[k + 2][0], u=batches[k + 2][1])
    torch.cuda.synchronize()
    return hist


def test_prefetched_steps_are_value_identical_across_the_arms():
    runs = {arm: _pipeline(arm) for arm in ARMS}
    for arm in ("sampling", "field"):
        for k, (a, b) in enumerate(zip(runs[arm], runs["off"])):
            _same(a, b, "%s, step %d" % (arm, k))
    on = runs["sampling"]
    assert "out_dists" in on[1] and "out_dists" in on[3] and "out_dists" not in on[0]


def test_switch(monkeypatch):
    d, u = _batch(_hit("some"), NC)
    monkeypatch.setenv("MLI_ELIDE_OUTSIDE_SAMPLING", "0")
    tr = _trainer(True, R, NC, NF, log2T=14)
    tr.train_step(d, u=u)
    eng, fld = tr.model.engine, tr.model._last_state[2]
    assert eng.elide_outside_sampling is False and eng.elide_outside is True
    assert fld["elided"] and not fld["sampling_elided"]       # the FIELD pass alone
    monkeypatch.delenv("MLI_ELIDE_OUTSIDE_SAMPLING")
    tr = _trainer(True, R, NC, NF, log2T=14)
    tr.train_step(d, u=u)
    eng, fld = tr.model.engine, tr.model._last_state[2]
    assert eng.elide_outside_sampling is True and fld["elided"] and fld["sampling_elided"]
    # the attribute overrides the environment; no effect with elide_outside off
    tr = _trainer(True, R, NC, NF, log2T=14)
    tr.model.elide_outside_sampling = False
    tr.train_step(d, u=u)
    assert tr.model.engine.elide_outside_sampling is False and not tr.model._last_state[2]["sampling_elided"]
    tr = _trainer(True, R, NC, NF, log2T=14)
    tr.model.elide_outside, tr.model.elide_outside_sampling = False, True
    tr.train_step(d, u=u)
    fld = tr.model._last_state[2]
    assert not fld["elided"] and not fld["sampling_elided"]
