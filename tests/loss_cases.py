"""Seeded inputs, edge cases and error bounds of the loss-kernel tests (tests/test_gpu_loss.py), shared
with the CPU tests of the reference (tests/test_loss_ref.py).  numpy only."""
import math

import numpy as np

import loss_ref

EPS32 = 2.0 ** -24

# (R, N) of mli_stage_b_loss: one ray; odd sizes; around one 256-ray workgroup; R > 1024 (the strided
# loop of the min/max block); 1026 workgroups (the finalize reads the partials from global memory)
SHAPES = ((1, 1), (3, 37), (255, 4), (256, 4), (257, 4), (1025, 2), (196865, 1))
EDGE_SHAPES = ((257, 4), (3, 37))
EDGES = ("zero_resid", "ore_zero_e1", "ore_zero_e2", "sha_const", "cert_const", "both_const", "range_reversed",
         "nonfinite", "all_outside", "none_outside", "grad_null", "hess_null", "intr_off_null", "render_only",
         "rgb_eq_gt")


def _signed(rng, shape, lo=0.5, hi=1.5):
    return rng.uniform(lo, hi, shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def draw_grad(rng, N, R):
    """[N][R][3] with |grad| in [0.5, 0.9] or [1.1, 2]."""
    d = rng.standard_normal((N, R, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    mag = np.where(rng.random((N, R, 1)) < 0.4, rng.uniform(0.5, 0.9, (N, R, 1)), rng.uniform(1.1, 2.0, (N, R, 1)))
    return (d * mag).astype(np.float32)


def draw_hess(rng, N, R):
    """[N][R][3] rows of one sign whose sum has magnitude in [0.5, 1.5]."""
    p = rng.uniform(0.2, 1.0, (N, R, 3))
    p /= p.sum(axis=-1, keepdims=True)
    return (p * _signed(rng, (N, R, 1))).astype(np.float32)


def make_case(R, N, edge=None, seed=0):
    """(inputs, cfg) of one case: every loss term has magnitude in [0.5, 1.5] (before its pseudo
    weight), then the edge's change.  inputs are fp32 numpy arrays (None: a NULL pointer)."""
    rng = np.random.default_rng(1000003 * seed + 1009 * R + N)
    f = np.float32
    gt, ref = rng.random((R, 3)).astype(f), rng.random((R, 3)).astype(f)
    sha, cert = rng.random(R).astype(f), rng.random(R).astype(f)
    inp = dict(N=N, gt=gt, ref=ref, sha=sha, cert=cert,
               rgb=(gt + _signed(rng, (R, 3)).astype(f)).astype(f),
               o_r=(ref + _signed(rng, (R, 3)).astype(f)).astype(f),
               o_s=(sha + _signed(rng, R).astype(f)).astype(f),
               o_re=_signed(rng, (R, 3)).astype(f),
               outside=(rng.random(R) < 0.2).astype(np.uint8),
               grad=draw_grad(rng, N, R), hess=draw_hess(rng, N, R))
    if R >= 3:
        inp["outside"][0], inp["outside"][1] = 1, 0
    else:
        inp["outside"][:] = 0
    cfg = dict(loss_ref.DEFAULT_CFG)
    third = np.arange(R) % 3 == 0
    if edge == "zero_resid":
        inp["rgb"][third], inp["o_r"][third], inp["o_s"][third] = gt[third], ref[third], sha[third]
    elif edge in ("ore_zero_e1", "ore_zero_e2"):
        flat = inp["o_re"].reshape(-1)
        flat[0::4], flat[2::4] = 0.0, -0.0
        if edge == "ore_zero_e2":
            cfg.update(e_pos=2.0, f_pos=0.5)
    elif edge in ("sha_const", "both_const", "cert_const"):
        if edge != "cert_const":
            inp["sha"][:] = 0.625
        if edge != "sha_const":
            inp["cert"][:] = 0.375
    elif edge == "range_reversed":
        cfg.update(range_sha=(0.9, 0.2), range_vis=(1.0, 0.25))
    elif edge == "nonfinite":
        inside = np.nonzero(inp["outside"] == 0)[0]
        assert inside.size >= 1
        bad = [np.inf, -np.inf, np.nan]
        for i, r in enumerate(inside[::2]):
            inp["grad"][i % N, r, i % 3] = bad[i % 3]
        for i, r in enumerate(inside[::3] if inside.size > 2 else inside):
            inp["hess"][(i + 1) % N, r, i % 3] = bad[i % 2]
            if i % 4 == 3:   # +inf and -inf in one row: the sum is NaN
                inp["hess"][(i + 1) % N, r, (i + 1) % 3] = -bad[i % 2]
    elif edge == "all_outside":
        inp["outside"][:] = 1
    elif edge == "none_outside":
        inp["outside"][:] = 0
    elif edge == "grad_null":
        inp["grad"] = None
    elif edge == "hess_null":
        inp["hess"] = None
    elif edge == "intr_off_null":
        cfg.update(w_intrinsic=0.0)
        inp["ref"] = inp["sha"] = inp["cert"] = None
    elif edge == "render_only":
        cfg.update(w_eikonal=0.0, w_curvature=0.0, w_intrinsic=0.0, w_re=0.0)
    elif edge == "rgb_eq_gt":
        inp["rgb"] = gt.copy()
    else:
        assert edge is None, edge
    return inp, cfg


# ---------------------------------------------------------------- value bounds
# Every accumulator is a sum of non-negative fp32 terms, so its relative error is at most the number of
# rounded adds on the longest path from a term to the total, times 2^-24 (first order; a term's own few
# roundings are counted by the adds of exact zeros the chain also holds: at least 256 empty workgroups
# in mli_stage_b_loss, the idle lanes of the fused kernel).
def chain_stage_b(R, N, n_blocks):
    """mli_stage_b_loss: 256-thread workgroups, one ray per thread (3 terms of an accumulator) in the
    first ceil(R / 256), the R N samples grid-strided over the other 256; 6 shuffle steps, 4 waves per
    workgroup, and the finalize adds the n_blocks partials one after the other."""
    nb_ray = (R + 255) // 256
    assert n_blocks == nb_ray + 256, (n_blocks, nb_ray)
    smp = -(-R * N // (256 * 256))
    return dict(ray=3 + 6 + 4 + n_blocks, sample=smp + 6 + 4 + n_blocks)


def chain_composite(R, N, nb):
    """mli_composite_loss: a lane holds 4 samples of one ray, lane 0 of a ray its 3 terms; 6 shuffle
    steps, 4 waves per workgroup; the finalize gives lane j of 32 the partials j, j + 32, ... and
    adds the lanes in a 5-step tree."""
    tail = -(-nb // 32) + 5
    return dict(ray=3 + 6 + 4 + tail, sample=4 + 6 + 4 + tail)


VALUE_KIND = dict(render="ray", mse="ray", intrinsic="ray", regularize_re="ray", eikonal="sample", curvature="sample")


def value_bounds(ref_losses, cfg, chain):
    """name -> absolute bound of each of the 8 loss values from the chain lengths."""
    ref = dict(zip(loss_ref.NAMES, ref_losses))
    b = {k: chain[VALUE_KIND[k]] * EPS32 * abs(ref[k]) for k in VALUE_KIND}
    b["total"] = sum(abs(loss_ref.f32(cfg["w_" + ("re" if k == "regularize_re" else k)])) * b[k]
                     for k in ("render", "eikonal", "curvature", "intrinsic", "regularize_re"))
    b["psnr"] = 10.0 / math.log(10.0) * chain["ray"] * EPS32
    return b


def pow_terms(o_re, cfg, R, dtype):
    """torch restatement in ``dtype`` of the e_pos != 1 arithmetic: (f_pos mean max(o_re, 0)^e,
    d total / d o_re of the non-negative elements, 0 elsewhere)."""
    import torch
    x = torch.as_tensor(np.asarray(o_re, dtype=np.float32)).to(dtype)
    e = torch.tensor(loss_ref.f32(cfg["e_pos"]), dtype=dtype)
    f_pos, w_re = (torch.tensor(loss_ref.f32(cfg[k]), dtype=dtype) for k in ("f_pos", "w_re"))
    pos = x >= 0
    xp = torch.where(pos, x, torch.zeros_like(x))
    re_pos = torch.where(pos, torch.pow(xp, e), torch.zeros_like(x)).sum() / (3 * R) * f_pos
    d = torch.where(pos, w_re * (f_pos * e * torch.pow(xp, e - 1.0)) / (3 * R), torch.zeros_like(x))
    return float(re_pos), d.double().numpy()
