"""mli_stage_b_loss and the loss values of mli_composite_loss through the C ABI against float64 (GPU).

The reference is tests/loss_ref.py (closed-form float64 from the fp32 inputs; tests/test_loss_ref.py
holds it to float64 autograd through the eager torch losses at 1e-12).  Outputs and scratch are
NaN-filled with canary tails.

Gradients: exactly 0 where the reference is exactly 0; elsewhere |err| <= 1e-6 x the largest magnitude
the output's gradient can take in the case (loss_ref.grad_ceiling): at most ten rounded fp32 operations
give 6e-7.  With e_pos != 1 (powf) the non-negative elements of d_o_re and the positive half of
regularize_re get 8 x the error of torch float32 on the CPU at the same inputs, floor 1e-6 (relative to
max |ref|).

Loss values: every accumulator is a sum of non-negative terms, so its relative error is at most the
longest chain of adds x 2^-24, the chain counted from the launch geometry (tests/loss_cases.py
chain_stage_b / chain_composite); total takes the weighted sum of the bounds, psnr 10 / ln 10 x the
relative mse bound.

What a single defect costs against the bound (relative size of one dropped term / the bound):
    (1, 1)       render 1/3 against 1.6e-5: 2e4 x;  eikonal, curvature: the only term
    (3, 37)      render 1/9: 7e3 x;  eikonal 1/111 less the outside rays: 6e2 x
    (255..257,4) render 1/770: 80 x;  eikonal 1/1000: 60 x
    (1025, 2)    render 1/3075 against 1.6e-5: 20 x
    (196865, 1)  a term is 1.7e-6 of its sum, below the 1039-add bound of 6.2e-5; a dropped workgroup
                 partial (256 rays of 196865, 1.3e-3) is 21 x the bound, and this is the shape whose
                 partials the finalize reads straight from global memory
(tests/test_loss_ref.py runs the render bound and the gradient bar against such defects on the CPU.)"""
import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L

import loss_cases as lc
import loss_ref
from margins import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64
GRADS = ("d_rgb", "d_o_r", "d_o_s", "d_o_re")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(n):
    return torch.full((n + TAIL,), float("nan"), device=DEV)


def _loss_args(R, N, dev, cfg, outs, losses, scratch):
    f = loss_ref.f32
    g = lambda k: L.ptr(dev.get(k))  # noqa: E731
    return L.LossArgs(R, N, g("rgb"), g("o_r"), g("o_s"), g("o_re"), g("gt"), g("ref"), g("sha"), g("cert"),
                      g("outside"), g("grad"), g("hess"),
                      f(cfg["w_render"]), f(cfg["w_eikonal"]), f(cfg["w_curvature"]), f(cfg["w_intrinsic"]),
                      f(cfg["w_re"]),
                      f(cfg["range_sha"][0]), f(cfg["range_sha"][1]), f(cfg["range_vis"][0]), f(cfg["range_vis"][1]),
                      f(cfg["f_ref"]), f(cfg["f_sha"]), f(cfg["f_neg"]), f(cfg["f_pos"]), f(cfg["e_pos"]),
                      *[L.ptr(t) for t in outs], L.ptr(losses), L.ptr(scratch))


def _stage_b(inp, cfg):
    """One mli_stage_b_loss call -> (losses [8], {d_*: numpy}, workgroups)."""
    R, N = inp["rgb"].shape[0], inp["N"]
    dev = {k: _dev(v) for k, v in inp.items() if k != "N"}
    ws = L.workspace("mli_stage_b_loss", L.LossArgs(R, N))
    assert ws[1:] == [R * 12, R * 12, R * 4, R * 12] and (ws[0] - 16) % 32 == 0
    scratch = _nan(ws[0] // 4)
    outs = [_nan(b // 4) for b in ws[1:]]
    losses = _nan(8)
    L.call("mli_stage_b_loss", _loss_args(R, N, dev, cfg, outs, losses, scratch))
    torch.cuda.synchronize()
    for t, n in zip([scratch, losses] + outs, [ws[0] // 4, 8] + [b // 4 for b in ws[1:]]):
        assert torch.isnan(t[n:]).all()                       # nothing past the sizes the query gives
    assert not torch.isnan(scratch[:ws[0] // 4]).any()        # min/max and every partial written
    got = {k: t[:b // 4].cpu().numpy().astype(np.float64).reshape((R, 3) if b == R * 12 else (R,))
           for k, t, b in zip(GRADS, outs, ws[1:])}
    return losses[:8].cpu().numpy().astype(np.float64), got, (ws[0] // 4 - 4) // 8


def _pow_bars(inp, cfg, R):
    """e_pos != 1: (relative bar of re_pos, relative bar of d_o_re on the non-negative elements) =
    max(8 x torch float32's error against float64 over max |ref|, 1e-6)."""
    import torch as t
    v64, d64 = lc.pow_terms(inp["o_re"], cfg, R, t.float64)
    v32, d32 = lc.pow_terms(inp["o_re"], cfg, R, t.float32)
    return max(8 * abs(v32 - v64) / abs(v64), 1e-6), max(8 * np.abs(d32 - d64).max() / np.abs(d64).max(), 1e-6)


def _check_values(tag, got, inp, cfg, chain):
    ref, _, _, _, _, parts = loss_ref.evaluate(inp, cfg)
    bounds = lc.value_bounds(ref, cfg, chain)
    if loss_ref.f32(cfg["e_pos"]) != 1.0 and parts["re_pos"] > 0:
        rel_v, _ = _pow_bars(inp, cfg, inp["o_re"].shape[0])
        extra = rel_v * parts["re_pos"] - chain["ray"] * lc.EPS32 * parts["re_pos"]
        if extra > 0:
            bounds["regularize_re"] += extra
            bounds["total"] += abs(loss_ref.f32(cfg["w_re"])) * extra
    for i, name in enumerate(loss_ref.NAMES):
        g, r = got[i], ref[i]
        if not np.isfinite(r):
            assert g == r, (tag, name, g, r)                  # psnr = +inf on both sides
            continue
        assert np.isfinite(g), (tag, name, g)
        if r == 0.0 and name != "psnr":
            assert g == 0.0, (tag, name, g)
        check("%s %s: |err| (ref %.6g)" % (tag, name, r), abs(g - r), bounds[name])


def _check_grads(tag, got, inp, cfg):
    R = inp["rgb"].shape[0]
    ref = dict(zip(GRADS, loss_ref.losses64(inp, cfg)[1:]))
    ceil = loss_ref.grad_ceiling(cfg, R)
    for k in GRADS:
        g, r = got[k], ref[k]
        assert np.isfinite(g).all(), (tag, k)
        assert (g[r == 0] == 0).all(), (tag, k, int((g[r == 0] != 0).sum()))
        err = np.abs(g - r)
        if k == "d_o_re" and loss_ref.f32(cfg["e_pos"]) != 1.0:
            pos = inp["o_re"] >= 0
            _, rel_d = _pow_bars(inp, cfg, R)
            check("%s d_o_re (x >= 0, powf): max |err| / max |ref|" % tag, err[pos].max() / np.abs(r[pos]).max(),
                  rel_d)
            err = err[~pos]
        if err.size and ceil[k] > 0:
            check("%s %s: max |err| / ceiling" % (tag, k), err.max() / ceil[k], 1e-6)


@pytest.mark.parametrize("R,N", lc.SHAPES)
def test_stage_b_loss_shapes(R, N):
    inp, cfg = lc.make_case(R, N)
    losses, grads, nb = _stage_b(inp, cfg)
    assert nb == (R + 255) // 256 + 256 and (nb > 1024) == (R > 196608)
    tag = "stage_b R%d N%d" % (R, N)
    _check_grads(tag, grads, inp, cfg)
    _check_values(tag, losses, inp, cfg, lc.chain_stage_b(R, N, nb))


@pytest.mark.parametrize("edge", lc.EDGES)
@pytest.mark.parametrize("R,N", lc.EDGE_SHAPES)
def test_stage_b_loss_edges(R, N, edge):
    inp, cfg = lc.make_case(R, N, edge)
    losses, grads, nb = _stage_b(inp, cfg)
    tag = "stage_b R%d N%d %s" % (R, N, edge)
    _check_grads(tag, grads, inp, cfg)
    _check_values(tag, losses, inp, cfg, lc.chain_stage_b(R, N, nb))
    if edge == "rgb_eq_gt":
        assert losses[6] == np.inf and losses[7] == 0 and losses[0] == 0 and not grads["d_rgb"].any()
    if edge == "all_outside":
        assert losses[1] == 0 and losses[2] == 0


# ---------------------------------------------------------------- mli_composite_loss: the loss values
CN = 32


class _Composite:
    """Seeded composite inputs at N = 32 and the buffers of one mli_composite_loss call."""

    def __init__(self, R, white_bg, zero_heads, grad):
        rng = np.random.default_rng(R)
        f = np.float32
        self.R, self.white_bg = R, white_bg
        dists = np.sort(rng.random((R, CN)) * 2 + 0.5, axis=1).T.astype(f)
        v = rng.standard_normal((R, 3))
        y = rng.random((CN, R, 8)).astype(f)
        if zero_heads:                       # rgb = o_r = 0, so o_re = 0 - 0 * o_s is an exact zero
            y[:, ::3, :6] = 0
        self.dev = dict(dists=_dev(dists), far=_dev((dists[-1] + 0.1).astype(f)),
                        v=_dev((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f)),
                        ray_norm=_dev((rng.random(R) + 0.5).astype(f)),
                        sdf=_dev(((rng.random((CN, R)) - 0.5) * 0.2).astype(f)),
                        y=_dev(y), s_var=_dev(np.array([3.0], dtype=f)), grad=_dev(grad))

    def run(self, inp, cfg, defer=False):
        """-> (losses [8] bits, outputs dict numpy fp32, partial count)."""
        R, d = self.R, self.dev
        lab = {k: _dev(inp.get(k)) for k in ("gt", "ref", "sha", "cert", "outside", "grad", "hess")}
        o = dict(weights=_nan(CN * R), rgb=_nan(3 * R), o_r=_nan(3 * R), o_s=_nan(R), o_re=_nan(3 * R))
        comp = L.CompositeArgs(R, CN, L.ptr(d["dists"]), L.ptr(d["far"]), L.ptr(d["v"]), L.ptr(d["ray_norm"]),
                               L.ptr(d["sdf"]), L.ptr(d["grad"]), L.ptr(d["y"]), L.ptr(d["s_var"]), 0.3, self.white_bg,
                               L.ptr(o["weights"]), L.ptr(o["rgb"]), L.ptr(o["o_r"]), L.ptr(o["o_s"]), L.ptr(o["o_re"]),
                               None, None, None, None)
        ws = L.workspace("mli_composite_loss", L.CompositeLossArgs(comp, L.LossArgs(R, CN), 1.0, None))
        assert ws[0] % 32 == 0 and ws[1] == CN * R * 32
        scratch, dz4, losses = _nan(ws[0] // 4), _nan(ws[1] // 4), _nan(8)
        args = L.CompositeLossArgs(comp, _loss_args(R, CN, lab, cfg, [None] * 4, losses, scratch), 1024.0, L.ptr(dz4),
                                   1 if defer else 0, None)
        L.call("mli_composite_loss", args)
        if defer:
            torch.cuda.synchronize()
            assert torch.isnan(losses).all()
            L.call("mli_composite_loss_finalize", args)
        torch.cuda.synchronize()
        for t, n in ((scratch, ws[0] // 4), (dz4, ws[1] // 4), (losses, 8), (o["rgb"], 3 * R), (o["o_s"], R)):
            assert torch.isnan(t[n:]).all() and not torch.isnan(t[:n]).any()
        outs = {k: o[k][:n].cpu().numpy().reshape(s) for k, n, s in
                (("rgb", 3 * R, (R, 3)), ("o_r", 3 * R, (R, 3)), ("o_s", R, (R,)), ("o_re", 3 * R, (R, 3)))}
        return losses[:8].cpu().numpy(), outs, ws[0] // 32


def _composite_case(R, edge):
    """The labels of make_case moved onto the outputs the kernel composites (so that a residual of the
    case, an exact zero included, is the residual the kernel sees), two runs, and the checks."""
    inp, cfg = lc.make_case(R, CN, edge)
    if edge == "nonfinite":              # this kernel composites from grad: non-finite values in hess only
        inp["grad"] = lc.make_case(R, CN)[0]["grad"]
    cgrad = inp["grad"] if inp["grad"] is not None else lc.make_case(R, CN)[0]["grad"]   # grad_null: the loss's pointer
    comp = _Composite(R, white_bg=0 if edge in ("ore_zero_e1", "ore_zero_e2") else 1,
                      zero_heads=edge in ("ore_zero_e1", "ore_zero_e2"), grad=cgrad)
    _, out0, nb = comp.run(inp, cfg)
    f = np.float32
    lab = dict(inp)
    lab["gt"] = (out0["rgb"] - (inp["rgb"] - inp["gt"])).astype(f)
    if inp["ref"] is not None:
        lab["ref"] = (out0["o_r"] - (inp["o_r"] - inp["ref"])).astype(f)
        if edge not in ("sha_const", "both_const"):
            lab["sha"] = (out0["o_s"] - (inp["o_s"] - inp["sha"])).astype(f)
    got, out, nb = comp.run(lab, cfg)
    for k in out:
        assert np.array_equal(out[k].view(np.uint32), out0[k].view(np.uint32)), k
    ref_in = dict(lab, N=CN, **out)
    tag = "composite R%d %s" % (R, edge or "default")
    _check_values(tag, got.astype(np.float64), ref_in, cfg, lc.chain_composite(R, CN, nb))
    got_d, _, _ = comp.run(lab, cfg, defer=True)
    assert np.array_equal(got_d.view(np.uint32), got.view(np.uint32))
    return ref_in, out, nb


# partial counts: below 32 (the tail loop alone), 32..255 (the tail loop, several rounds), above 256 and
# not a multiple of 32 (the 8-deep unrolled loop, then the tail); every lane of the 32-lane tree used
@pytest.mark.parametrize("R,lo,hi", [(203, 1, 31), (1001, 32, 255), (2397, 257, 10 ** 9)])
def test_composite_loss_values_by_partial_count(R, lo, hi):
    _, _, nb = _composite_case(R, None)
    assert lo <= nb <= hi and (hi < 10 ** 9 or nb % 32 != 0), nb


@pytest.mark.parametrize("edge", lc.EDGES)
def test_composite_loss_values_edges(edge):
    ref_in, out, _ = _composite_case(203, edge)
    if edge in ("ore_zero_e1", "ore_zero_e2"):
        o = out["o_re"]
        assert (o == 0).any() and (o > 0).any() and (o < 0).any()
    if edge == "zero_resid":
        assert ((out["rgb"] == ref_in["gt"]).all(axis=1) == (np.arange(203) % 3 == 0)).all()
        assert ((out["o_s"] == ref_in["sha"]) == (np.arange(203) % 3 == 0)).all()
