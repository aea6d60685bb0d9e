"""mli_hash_bwd (hash_bwd_kernel, csrc/sdf.hip) called directly, against tests/hash_bwd_ref.py:
the float64 scatter of a seeded d enc over the 5 points' corners, element by element.

No Trainer and no Model: rays, depths and the d enc image are built on the host, the levels are
engine._grid_levels at log2T = 18 (levels 0-2 dense with fastmod indexing, 3-15 hashed; the pair
(2, 3) runs one of each in the two halves of a wave).  Random rays cover the launch shapes, odd
and single active levels, both eps (taps inside / outside the centre's cell) and out-of-range
points; hash_bwd_ref.crafted_runs puts every run length 1..32 at every start lane in front of
the segmented scan (tests/test_hash_bwd_ref.py asserts these input properties on the CPU).

The bar is derived, not measured (hash_bwd_ref.tolerance): per element
|gpu - g| <= (n + 8) 2^-23 A, plus n 2^-41 in deterministic mode; where A == 0 the element is
exactly 0, and nothing outside the reference's rows is written.  The worst err / tol of every
case goes through margins.check (recorded with MLI_MARGINS_OUT)."""
import numpy as np
import pytest
import torch

import hash_bwd_ref as H
from margins import check
from oracle import hashgrid as o_hash

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS_FINE = float(np.float32(1.4e-4))
EPS_COARSE = 0.02

# name -> (rays, active_levels, eps, log2T); rays = ("random", R, N, seed, spread),
# ("crafted", variant[, spread]) or ("idle_neighbour",)
CASES = {
    "r2x32_a16_fine": (("random", 2, 32, 11, "in_range"), 16, EPS_FINE, 18),     # one workgroup, two idle waves
    "r2x32_a1_coarse": (("random", 2, 32, 12, "in_range"), 1, EPS_COARSE, 18),
    "r6x32_a15_fine": (("random", 6, 32, 13, "in_range"), 15, EPS_FINE, 18),     # last workgroup half full
    "r6x32_a16_coarse": (("random", 6, 32, 14, "in_range"), 16, EPS_COARSE, 18),
    "r16x20_a16_fine": (("random", 16, 20, 15, "in_range"), 16, EPS_FINE, 18),   # tiles straddle rays
    "r16x20_a15_coarse": (("random", 16, 20, 16, "in_range"), 15, EPS_COARSE, 18),
    "r8x80_a16_coarse": (("random", 8, 80, 17, "in_range"), 16, EPS_COARSE, 18),
    "r8x80_a1_fine": (("random", 8, 80, 18, "in_range"), 1, EPS_FINE, 18),
    "r6x32_out_of_range": (("random", 6, 32, 0, "out_of_range"), 16, EPS_COARSE, 18),
    # a tap in cell (-1, l, -1) next to lane l, which adds nothing to that tap's scatter
    "idle_neighbour": (("idle_neighbour",), 16, EPS_FINE, 18),
    "r8x80_log2T14": (("random", 8, 80, 19, "in_range"), 16, EPS_FINE, 14),      # all hashed
    "crafted_center": (("crafted", "center"), 16, EPS_FINE, 18),
    "crafted_face": (("crafted", "face"), 16, EPS_FINE, 18),
    "crafted_jitter": (("crafted", "jitter"), 16, EPS_FINE, 18),
    # the same runs, every ray in (y, z) cells of its own: n, and with it the bar, stays small
    "crafted_center_spread": (("crafted", "center", True), 16, EPS_FINE, 18),
    "crafted_face_spread": (("crafted", "face", True), 16, EPS_FINE, 18),
    "crafted_jitter_spread": (("crafted", "jitter", True), 16, EPS_FINE, 18),
}
_LEVELS, _BUILT = {}, {}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mli_nerf_amd import _lib
    return _lib


def _levels(log2T):
    if log2T not in _LEVELS:
        from mli_nerf_amd import engine
        g, total = engine._grid_levels(engine.PathConfig(log2T=log2T))
        _LEVELS[log2T] = (g, total * 8, o_hash.level_table(log2T=log2T)[0])
    return _LEVELS[log2T]


def _case(name):
    """Inputs and reference of a case, built once and shared by both modes."""
    if name not in _BUILT:
        spec, active, eps, log2T = CASES[name]
        if spec[0] == "crafted":
            rays = H.crafted_runs(spec[1], eps, spread=len(spec) > 2)
        elif spec[0] == "idle_neighbour":
            rays = H.idle_neighbour_rays(eps)
        else:
            rays = H.random_rays(*spec[1:])
        S = rays["R"] * rays["N"]
        mat = H.random_d_enc(S, seed=100 + list(CASES).index(name))
        pts = H.points5(rays["center"], rays["ray_unit"], rays["dists"], eps)
        ref = H.reference(pts, H.d_enc_points(mat), _levels(log2T)[2], active)
        _BUILT[name] = dict(rays=rays, mat=mat, ref=ref, active=active, eps=eps, log2T=log2T)
    return _BUILT[name]


def _run(L, rays, mat, active, eps, log2T, deterministic, prefill=0.0):
    """One mli_hash_bwd call into a d_table prefilled with ``prefill``; returns the d_table."""
    g, n_params, _ = _levels(log2T)
    dev = [rays[k].to(DEV).contiguous() for k in ("center", "ray_unit", "dists")] + [H.d_enc_image(mat).to(DEV)]
    d_table = torch.full((n_params,), prefill, device=DEV)
    ws = torch.zeros(n_params, dtype=torch.int64, device=DEV) if deterministic else None
    L.call("mli_hash_bwd", L.HashBwdArgs(rays["R"], rays["N"], L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]),
                                         L.ptr(dev[3]), g, eps, active, L.ptr(d_table), 1 if deterministic else 0,
                                         L.ptr(ws), n_params))
    torch.cuda.synchronize()
    return d_table


def _compare(label, out, ref, tol, base=0.0):
    """out - base against the reference: the per-element bar on the reference's rows, ``base``
    untouched everywhere else and where no nonzero contribution lands."""
    got = out.view(-1, 8)[ref["rows"].to(DEV)].cpu().double()
    outside = int((out != base).sum()) - int((got != base).sum())
    check(label + ": elements written outside the reference's rows", outside, 0, "<=")
    zero = ref["A"] == 0
    check(label + ": elements written where A == 0", int((got[zero] != base).sum()), 0, "<=")
    err = ((got - base) - ref["g"]).abs()
    ratio = err[~zero] / tol[~zero]
    i = int(ratio.argmax())
    print("%s: %d elements in %d rows, n <= %d, worst err / tol %.4f (err %.3g, tol %.3g, g %.3g)" % (
        label, int((~zero).sum()), ref["rows"].numel(), int(ref["n"].max()), float(ratio[i]), float(err[~zero][i]),
        float(tol[~zero][i]), float(ref["g"][~zero][i])))
    check(label + ": worst err / tol", float(ratio[i]), 1.0, "<=")


@pytest.mark.parametrize("mode", ["atomic", "deterministic"])
@pytest.mark.parametrize("name", list(CASES))
def test_hash_bwd_equals_the_reference(L, name, mode):
    c = _case(name)
    ref, det = c["ref"], mode == "deterministic"
    args = (L, c["rays"], c["mat"], c["active"], c["eps"], c["log2T"], det)
    if det:
        # d_table is overwritten: nothing of the 7.0 survives
        _compare("%s %s" % (name, mode), _run(*args, prefill=7.0), ref, H.tolerance(ref, True))
        return
    _compare("%s %s" % (name, mode), _run(*args), ref, H.tolerance(ref))
    # the call accumulates: onto a constant b every one of the <= n atomic adds of an element
    # rounds a value of at most b + A to fp32, n 2^-24 (b + A) more; elsewhere b stays.  (A power
    # of two is the tightest b: half an ulp just above it is exactly 2^-24 b, so an element with
    # one small contribution comes as close to this bar as rounding to nearest allows.)
    b = 0.25
    tol = H.tolerance(ref) + ref["n"] * 2.0 ** -24 * (b + ref["A"])
    _compare("%s %s onto %.2f" % (name, mode, b), _run(*args, prefill=b), ref, tol, base=b)


def test_deterministic_mode_is_invariant(L):
    """Bit-identical across two calls, and after permuting the rays: at N = 32 that permutes whole
    tiles, so the run totals are the same numbers and their integer sums do not depend on order."""
    c = _case("crafted_jitter")
    rays, mat = c["rays"], c["mat"]
    args = (c["active"], c["eps"], c["log2T"], True)
    first = _run(L, rays, mat, *args)
    assert int(torch.count_nonzero(first)) > 0
    assert torch.equal(first, _run(L, rays, mat, *args))
    R = rays["R"]
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(5))
    assert rays["N"] == 32 and not torch.equal(perm, torch.arange(R))
    rays_p = dict(R=R, N=32, center=rays["center"][perm], ray_unit=rays["ray_unit"][perm],
                  dists=rays["dists"][:, perm].contiguous())
    mat_p = mat.view(128, R, 160)[:, perm].reshape(128, R * 160)   # tile r = columns 160 r .. 160 r + 159
    assert not torch.equal(rays_p["dists"], rays["dists"])
    assert torch.equal(first, _run(L, rays_p, mat_p, *args))


def test_error_convention(L):
    rays = H.random_rays(3, 32, seed=1)                         # S = 96: no multiple of 64
    with pytest.raises(RuntimeError, match="mli_hash_bwd"):
        _run(L, rays, H.random_d_enc(96, 1), 16, EPS_FINE, 18, False)
    with pytest.raises(RuntimeError, match="mli_hash_bwd"):
        _run(L, rays, H.random_d_enc(96, 1), 16, EPS_FINE, 18, True)
    empty = dict(R=0, N=32, center=torch.zeros(1, 3), ray_unit=torch.zeros(1, 3), dists=torch.zeros(32, 1))
    for det in (False, True):                                   # R = 0: returns, d_table untouched
        out = _run(L, empty, H.random_d_enc(64, 1), 16, EPS_FINE, 18, det, prefill=7.0)
        assert bool((out == 7.0).all())
