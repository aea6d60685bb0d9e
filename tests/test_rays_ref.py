"""tests/rays_ref.py, the float64 restatement of the per-ray kernels, pinned to what is already
pinned to the reference: the fp32 functions of oracle/render.py (and torch autograd through
them), on the input recipes of tests/rays_cases.py that tests/test_gpu_rays.py feeds the kernels.
None of these measures a kernel.  No GPU, no library.

Each fp32-oracle-against-float64 error is recorded through ``margins.check``; the bars of
tests/test_gpu_rays.py are multiples of these errors, recomputed there per case.  The bars HERE
are 4 x the largest error this file measured over its cases (the second factor in BARS): a
restatement that drifts from the oracle by more than fp32 rounding fails."""
import pytest
import torch

import rays_cases as RC
import rays_ref as RR
from margins import check
from oracle import render as o_render

# quantity -> 4 x the largest fp32-oracle-against-float64 error measured over this file's cases
BARS = {
    "fine dists": 4 * 4.7e-7,
    "coarse dists": 4 * 2.1e-7,
    "weights": 4 * 1.1e-6,
    "outputs": 4 * 2.3e-6,
    "d_sdf": 4 * 1.1e-5,
    "d_grad": 4 * 1.7e-5,
    "dz4": 4 * 1.6e-6,
    "dray": 4 * 2.9e-7,
    "d_s_var": 4 * 2.1e-5,
    "rays": 4 * 1.5e-7,
    "bounds": 4 * 1.7e-6,
}
KNOT = 1e-5          # a u within this of a cdf knot may fall into the neighbouring bin
WSUM = 0.5           # rays compared elementwise: float64 weight sum of the sections >= 0.5
SAMPLER_R = 37


def fine_mask(ref):
    """The fine samples compared elementwise [Nf][R], and the share left out for a knot among
    the rays with a weight sum >= WSUM."""
    rays = ref["wsum"] >= WSUM
    near = ref["knot"] < KNOT
    n = int(rays.sum()) * ref["knot"].shape[0]
    return rays[None] & ~near, (float((near & rays[None]).sum()) / n if n else 0.0)


@pytest.mark.parametrize("kind", ["none", "repeat_a", "repeat_b", "all_last", "unsorted_b"])
def test_merge_is_the_stable_sort(kind):
    c = RC.sampler_case(5, 64, 16, 3) if kind == "none" else RC.tie_lists(5, 64, 16, kind, 4)
    d, s, order = RR.merge(c["da"].double(), c["sa"].double(), c["db"].double(), c["sb"].double())
    cat_d, cat_s = torch.cat([c["da"], c["db"]], 0).double(), torch.cat([c["sa"], c["sb"]], 0).double()
    assert torch.equal(d, torch.sort(cat_d, dim=0).values)
    assert torch.equal(d, cat_d.gather(0, order)) and torch.equal(s, cat_s.gather(0, order))
    # stable: among equal distances the source index rises (list a first, then list b)
    same = d[1:] == d[:-1]
    assert bool((order[1:][same] > order[:-1][same]).all())
    if kind != "none":
        assert int(same.sum()) > 0
    # Nb = 0
    d0, s0, _ = RR.merge(c["da"].double(), c["sa"].double(), None, None)
    assert torch.equal(d0, c["da"].double()) and torch.equal(s0, c["sa"].double())


@pytest.mark.parametrize("Na,Nb,Nf,inv_s", RC.SAMPLER_CASES)
def test_fine_samples_match_the_oracle(Na, Nb, Nf, inv_s):
    c = RC.sampler_case(SAMPLER_R, Na, Nb, 100 + Na)
    ref = RR.sample_fine(c["da"], c["sa"], c["db"] if Nb else None, c["sb"] if Nb else None, inv_s, RC.u_fine(Nf))
    d32, s32 = ref["dists"].float(), ref["sdf"].float()
    assert torch.equal(d32.double(), ref["dists"])                      # a merge only moves values
    assert bool((ref["dists"][1:] > ref["dists"][:-1]).all())           # tie-free
    o = RC.oracle_fine(d32, s32, inv_s, Nf)
    mask, share = fine_mask(ref)
    # the recipe alone leaves out 0 - 0.2 % of the samples for a knot
    check("share of fine samples within %g of a cdf knot" % KNOT, share, 0.01)
    assert int(mask.sum()) >= Nf                                        # at least one whole ray compared
    e = float((o.double() - ref["fine"])[mask].abs().max())
    print("fine", (Na, Nb, Nf, inv_s), "compared", int(mask.sum()), "left out %.4f" % share, "err %.3g" % e)
    check("fp32 oracle vs float64: fine dists", e, BARS["fine dists"])
    out = c["kinds"] == 1
    assert torch.equal(ref["fine"][:, out], ref["dists"][-1:, out].expand(Nf, -1))   # outside: all alphas 0
    assert torch.equal(o[:, out].double(), ref["fine"][:, out])
    assert bool(torch.isfinite(ref["fine"]).all())
    assert bool(((ref["fine"] >= ref["dists"][:1]) & (ref["fine"] <= ref["dists"][-1:])).all())


@pytest.mark.parametrize("Nc", [1, 16, 64])
def test_coarse_samples_match_the_oracle(Nc):
    g = torch.Generator().manual_seed(Nc)
    near = torch.rand(37, generator=g) + 0.2
    far = near + torch.rand(37, generator=g) * 2 + 0.1
    for u in (None, torch.rand(37, Nc, generator=g)):
        ref = RR.coarse(near, far, Nc, u)
        o = o_render.stratified_dists(near[None, :, None], far[None, :, None], Nc, None if u is None else u[None])
        check("fp32 oracle vs float64: coarse dists", float((o[0, :, :, 0].t().double() - ref).abs().max()),
              BARS["coarse dists"])


def composite_errors(p):
    """fp32 oracle against float64 on one COMPOSITE_CASES entry: quantity -> error."""
    R, N, anneal, white, s_var = p
    c = RC.composite_inputs(p)
    args = (c["dists"], c["far"], c["ray_unit"])
    ref = RR.composite(*args, c["ray_norm"], c["sdf"], c["grad"], c["y"], torch.tensor([s_var]), anneal, white)
    d = RC.loss_grads(c, ref)
    geo = RR.composite_bwd_geo(*args, c["sdf"], c["grad"], c["y"], torch.tensor([s_var]), anneal, white, c["d_rgb"],
                               1.0)
    bwd = RR.composite_bwd(*args, c["sdf"], c["grad"], c["y"], torch.tensor([s_var]), anneal, white, *d, 1.0)
    o = RC.oracle_composite(c, s_var, anneal, white, grads=True, d=d)
    e = {"weights": RC.err(o["weights"], ref["weights"])}
    e["outputs"] = max(RC.err(o[k], ref[k]) for k in ("rgb", "o_r", "o_s", "o_re", "opacity", "gradient", "depth",
                                                       "blend_dist"))
    e["d_sdf"], e["d_grad"] = RC.err(o["d_sdf"], geo["d_sdf"]), RC.err(o["d_grad"], geo["d_grad"])
    e["dz4"] = max(RC.err(o["dz4_geo"], geo["dz4"]), RC.err(o["dz4"], bwd["dz4"]))
    e["dray"] = RC.err(o["dray"], bwd["dray"])
    e["d_s_var"] = RC.err(o["d_s_var"], geo["d_s_var"])
    # the per-ray partials of the restatement sum to d s_var / exp(s_var)
    assert abs(float(geo["d_inv_s"].sum() * torch.tensor(s_var, dtype=torch.float64).exp() - geo["d_s_var"][0])) <= \
        1e-12 * max(1.0, abs(float(geo["d_s_var"][0])))
    return e, ref, geo


@pytest.mark.parametrize("p", RC.COMPOSITE_CASES, ids=RC.composite_case_id)
def test_composite_and_its_backwards_match_the_oracle(p):
    e, ref, geo = composite_errors(p)
    print(RC.composite_case_id(p), {k: "%.3g" % v for k, v in e.items()})
    c = RC.composite_inputs(p)
    out = c["kinds"] == 1
    assert bool((ref["weights"][:, out] == 0).all())                     # outside rays: every alpha exactly 0
    for k in ("d_sdf", "d_grad"):
        assert bool((geo[k][:, out] == 0).all())
    for k, v in e.items():
        check("fp32 oracle vs float64: " + k, v, BARS[k])


def test_steep_and_zero_alpha_recipes():
    """The two crafted composite cases do what their docstrings say, in the fp32 oracle."""
    c = RC.steep_case()
    o = RC.oracle_composite(c, 6.0, RC.ANNEAL_MID, 1, grads=True)
    ref = RR.composite(c["dists"], c["far"], c["ray_unit"], c["ray_norm"], c["sdf"], c["grad"], c["y"],
                       torch.tensor([6.0]), RC.ANNEAL_MID, 1)
    k = c["N"] // 2
    w = o["weights"]
    trans = w[k] / RC.ALPHA_MAX                                            # T_k of every ray
    assert bool((trans > 0).any())
    # alpha_k = ALPHA_MAX in fp32: w_k / T_k, T_k from the float64 restatement
    t64 = (1 - ref["alpha"][:k]).prod(0)
    live = t64 > 1e-3
    assert int(live.sum()) >= 2
    # (T_k in fp32: k factors and k products, each <= 2^-24 relative; 4 (k + 1) 2^-24 bounds them twice over)
    assert float(((w[k].double() / t64)[live] - RC.ALPHA_MAX).abs().max()) < 4 * (k + 1) * 2.0 ** -24
    assert float((ref["alpha"][k] - 1 / (1 + 1e-5)).abs().max()) < 1e-12
    z = RC.zero_alpha_case()
    oz = RC.oracle_composite(z, 3.0, 0.0, 1, grads=True)
    assert bool((oz["weights"] == 0).all())                               # x = 0 exactly, every sample
    assert bool((oz["d_grad"].abs().amax(-1) > 0).all())                  # and the clamp passes the gradient
    gz = RR.composite_bwd_geo(z["dists"], z["far"], z["ray_unit"], z["sdf"], z["grad"], z["y"], torch.tensor([3.0]),
                              0.0, 1, z["d_rgb"], 1.0)
    check("fp32 oracle vs float64: d_grad (zero-alpha rays)", RC.err(oz["d_grad"], gz["d_grad"]), BARS["d_grad"])


@pytest.mark.parametrize("bounding", ["sphere", "box"])
def test_rays_match_the_oracle(bounding):
    cam = RC.camera(11, bounding)
    pix = torch.arange(cam["W"] * cam["H"])
    ref = RR.rays(cam["intr"], cam["pose"], cam["pose_light"], pix, cam["W"], bounding, cam["aabb"])
    o = RC.oracle_rays(cam, pix, bounding)
    miss = float(ref["outside"].double().mean())
    assert 0.1 < miss < 0.9, miss                                         # rays that miss the volume, and rays that hit
    clear = ref["margin"].abs() > 1e-6
    check("share of rays within 1e-6 of the bound's edge (%s)" % bounding, 1.0 - float(clear.double().mean()), 0.01)
    assert torch.equal(o["outside"][clear], ref["outside"][clear])
    e = max(RC.err(o[k], ref[k]) for k in ("center", "ray_unit", "ray_norm", "pts_light"))
    check("fp32 oracle vs float64: rays (%s)" % bounding, e, BARS["rays"])
    sel = well_conditioned(ref, bounding)
    eb = max(RC.err(o[k][sel], ref[k][sel]) for k in ("near", "far"))
    print(bounding, "miss %.2f" % miss, "rays err %.3g bounds err %.3g" % (e, eb))
    check("fp32 oracle vs float64: bounds (%s)" % bounding, eb, BARS["bounds"])


def well_conditioned(ref, bounding):
    """The rays whose near / far are compared: for the sphere the bounds are -ctv -+ sqrt(disc), and
    an error e of the discriminant becomes e / (2 sqrt(disc)): rays with disc >= 0.01 keep that
    factor <= 5 (grazing rays and misses are left to the ``outside`` comparison)."""
    return ref["margin"] >= 0.01 if bounding == "sphere" else ~ref["outside"]
