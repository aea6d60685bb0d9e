"""tests/loss_ref.py against a second, independent statement of the stage-b losses:
mli_nerf_amd.trainer.stage_b_losses (the torch functions of the eager path) run in float64 with
autograd for d total / d outputs, on the default inputs and on every edge case of
tests/test_gpu_loss.py; and the bars of that test against deliberately wrong variants of the
arithmetic, redone in fp32 on the CPU (no GPU)."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_ref
from mli_nerf_amd import trainer

W_NAMES = dict(render="w_render", eikonal="w_eikonal", curvature="w_curvature", intrinsic="w_intrinsic",
               regularize_re="w_re")


def _torch_statement(inp, cfg):
    t64 = lambda x, rg=False: torch.tensor(np.asarray(x, dtype=np.float32), dtype=torch.float64,  # noqa: E731
                                           requires_grad=rg)
    f = loss_ref.f32
    R = inp["rgb"].shape[0]
    out = {k: t64(inp[k], True) for k in ("rgb", "o_r", "o_re")}
    out["o_s"] = t64(inp["o_s"].reshape(R, 1), True)   # [R][1] maps, as the data loader gives them
    out["outside"] = torch.tensor(np.asarray(inp["outside"]) != 0)
    weights = {k: f(cfg[w]) for k, w in W_NAMES.items()}
    if inp.get("grad") is None:
        weights.pop("eikonal")
    else:
        out["gradients"] = t64(inp["grad"])
    out["hessians"] = None if inp.get("hess") is None else t64(inp["hess"])
    data = {"image_sampled": t64(inp["gt"])}
    if weights["intrinsic"] == 0.0:
        weights.pop("intrinsic")   # the kernel reads no pseudo map then; its loss value is 0
    else:
        data.update(pseudo_ref_sampled=t64(inp["ref"]), pseudo_sha_sampled=t64(inp["sha"].reshape(R, 1)),
                    pseudo_visibility_certainty_sampled=t64(inp["cert"].reshape(R, 1)))
    total, losses, psnr = trainer.stage_b_losses(
        out, data, weights, ranges=(tuple(map(f, cfg["range_sha"])), tuple(map(f, cfg["range_vis"]))),
        re_factors=(f(cfg["f_neg"]), f(cfg["f_pos"]), f(cfg["e_pos"])), intr_factors=(f(cfg["f_ref"]), f(cfg["f_sha"])))
    total.backward()
    mse = ((out["rgb"].detach() - data["image_sampled"]) ** 2).mean()
    losses = {k: v.detach() for k, v in losses.items()}
    vals = [float(losses.get(k, 0.0)) for k in ("render", "eikonal", "curvature", "intrinsic", "regularize_re")]
    grads = [np.zeros_like(inp[k], dtype=np.float64) if out[k].grad is None
             else out[k].grad.numpy().reshape(inp[k].shape) for k in ("rgb", "o_r", "o_s", "o_re")]
    return np.array(vals + [float(total.detach()), float(psnr), float(mse)]), grads


CASES = [(R, N, None) for R, N in lc.SHAPES] + [(R, N, e) for R, N in lc.EDGE_SHAPES for e in lc.EDGES]


@pytest.mark.parametrize("R,N,edge", CASES)
def test_losses64_equals_float64_autograd(R, N, edge):
    inp, cfg = lc.make_case(R, N, edge)
    got = loss_ref.losses64(inp, cfg)
    want_l, want_g = _torch_statement(inp, cfg)
    for name, a, b in zip(loss_ref.NAMES, got[0], want_l):
        if np.isinf(b):
            assert a == b, name
        else:
            assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300), (name, a, b)
    for name, a, b in zip(("d_rgb", "d_o_r", "d_o_s", "d_o_re"), got[1:], want_g):
        assert a.shape == b.shape and np.all(np.isfinite(a)), name
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (name, np.abs(a - b).max())
        assert np.array_equal(a == 0, b == 0), name


def test_edge_cases_reach_their_edges():
    """The cases hold what their names say (a case that lost its edge would test nothing)."""
    for R, N in lc.EDGE_SHAPES:
        inp, _ = lc.make_case(R, N, "zero_resid")
        assert ((inp["rgb"] == inp["gt"]).all(axis=1) == (np.arange(R) % 3 == 0)).all()
        assert (inp["o_s"] == inp["sha"]).sum() == len(range(0, R, 3))
        inp, cfg = lc.make_case(R, N, "ore_zero_e2")
        o = inp["o_re"].reshape(-1)
        assert (o == 0).any() and np.signbit(o[o == 0]).any() and not np.signbit(o[o == 0]).all()
        assert (o > 0).any() and (o < 0).any() and cfg["e_pos"] == 2.0 and cfg["f_pos"] == 0.5
        inp, _ = lc.make_case(R, N, "nonfinite")
        bad_g = ~np.isfinite(inp["grad"]).all(axis=-1)
        bad_h = ~np.isfinite(inp["hess"]).all(axis=-1)
        assert bad_g.any() and bad_h.any()
        assert not bad_g[:, inp["outside"] != 0].any() and not bad_h[:, inp["outside"] != 0].any()
        inp, _ = lc.make_case(R, N, "both_const")
        assert np.ptp(inp["sha"]) == 0 and np.ptp(inp["cert"]) == 0
        inp, _ = lc.make_case(R, N)
        n = np.linalg.norm(inp["grad"].astype(np.float64), axis=-1)
        assert n.min() >= 0.49 and n.max() <= 2.01 and (np.abs(n - 1) >= 0.099).all()
        assert 0 < inp["outside"].sum() < R


# ---------------------------------------------------------------- the bars against wrong arithmetic
def _fp32_kernel(inp, cfg, n_blocks, sgn0=0.0, skip_partial=None, drop_term=None):
    """The kernel's arithmetic redone in fp32 numpy, in ray order with per-workgroup partials (256
    rays each) summed in order -- and three deliberate defects: sgn(0) = sgn0, one workgroup partial
    skipped, one ray's render term dropped."""
    f = np.float32
    R = inp["rgb"].shape[0]
    d = inp["rgb"] - inp["gt"]
    sg = np.where(d > 0, f(1), np.where(d < 0, f(-1), f(sgn0)))
    d_rgb = f(cfg["w_render"]) * f(3) * sg * (f(1) / (f(3) * f(R)))
    term = np.abs(d).sum(axis=1, dtype=f)
    if drop_term is not None:
        term[drop_term] = 0
    parts = [term[b * 256:(b + 1) * 256].sum(dtype=f) for b in range((R + 255) // 256)]
    parts += [f(0)] * (n_blocks - len(parts))
    t = f(0)
    for b, p in enumerate(parts):
        if b != skip_partial:
            t = f(t + p)
    return f(t / (f(3) * f(R)) * f(3)), d_rgb


@pytest.mark.parametrize("R,N", [(3, 37), (257, 4), (196865, 1)])
def test_bars_catch_single_defects(R, N):
    """The value bound and the gradient bar of tests/test_gpu_loss.py pass the fp32 restatement and
    fail each single defect: sgn(0) = 1 (gradients), a skipped workgroup partial, a dropped term."""
    inp, cfg = lc.make_case(R, N, "zero_resid")
    n_blocks = (R + 255) // 256 + 256
    ref = loss_ref.losses64(inp, cfg)
    bound = lc.value_bounds(ref[0], cfg, lc.chain_stage_b(R, N, n_blocks))["render"]
    gbar = 1e-6 * loss_ref.grad_ceiling(cfg, R)["d_rgb"]

    def failures(**kw):
        render, d_rgb = _fp32_kernel(inp, cfg, n_blocks, **kw)
        return (abs(float(render) - ref[0][0]) > bound,
                bool((np.abs(d_rgb.astype(np.float64) - ref[1]) > gbar).any() or (d_rgb[ref[1] == 0] != 0).any()))

    assert failures() == (False, False)
    assert failures(sgn0=1.0) == (False, True)
    assert failures(skip_partial=0)[0]   # at R = 196865 one of 770 ray partials: 1.3e-3 against 6e-5
    if R <= 257:   # one of 3 R terms; at R = 196865 a term is 1e-6 of the sum, below the 1026-add bound
        assert failures(drop_term=R // 2)[0]
