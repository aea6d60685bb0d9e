"""The per-ray kernels of csrc/rays.hip, each called alone through the C ABI, against
tests/rays_ref.py (float64): mli_rays, mli_sample_coarse, mli_sample_fine, mli_composite_fwd,
mli_composite_bwd, mli_composite_bwd_geo.  No Trainer, no Model: the inputs are the seeded recipes
of tests/rays_cases.py, at the shapes where wave-level code goes wrong -- one ray, tail waves
(R % 4, R % 8 != 0), N % 4 != 0, every register slot of the 256-wide merge, and both sides of the
N = 128 switch between two rays and one ray per wave.

Bars.  A merge only moves values: bit for bit.  Everything else is compared with float64 at
8 x the error the fp32 oracle (oracle/render.py, sequential torch ops) has against float64 ON THE
SAME CASE, computed here on the CPU and never from a GPU output, with a floor of a few ulps
(2^-20 for a distance in [2, 4), 1e-6 relative for the composite's tensors).  The factor covers
what two correct fp32 evaluations do differently: the tree-shaped wave scans against sequential
cumprod / cumsum, expf against torch's sigmoid, the adjugate against an LU inverse.
tests/test_rays_ref.py pins the float64 restatement to the oracle and records the oracle's errors.
Composite tensors use max |gpu - ref| / max |ref| per tensor.  d s_var is one number per case, so
one case's oracle error can be small by accident: its bar is 8 x the LARGEST oracle error over the
case list.  Every bar goes through ``margins.check`` with the oracle's error in the note."""
import ctypes as C

import numpy as np
import pytest
import torch

import rays_cases as RC
import rays_ref as RR
from margins import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64                    # elements behind every output buffer that no kernel may touch
FILL = -7.25
FACTOR = 8.0
DIST_FLOOR = 2.0 ** -20        # four ulps of a distance in [2, 4)
REL_FLOOR = 1e-6
KNOT, WSUM = 1e-5, 0.5         # as tests/test_rays_ref.py
SCALE = 2.0 ** 10              # grad_scale: a power of two, exact
RS = [1, 5, 37]                # one ray; a tail wave; R % 4 != 0 and R % 8 != 0 over several workgroups


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mli_nerf_amd import _lib
    return _lib


class Bufs:
    """Output buffers exactly as wide as the kernel's contract says, each followed by a canary."""

    def __init__(self):
        self.items = []

    def new(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        fill = FILL if dtype.is_floating_point else 173
        full = torch.full((n + CANARY,), fill, dtype=dtype, device=DEV)
        self.items.append((full, n, fill))
        return full[:n].view(*shape)

    def canaries_intact(self):
        return all(bool((full[n:] == fill).all()) for full, n, fill in self.items)

    def untouched(self):
        return all(bool((full == fill).all()) for full, n, fill in self.items)


class Checks:
    """margins.check for every quantity of a test before the first failure ends it."""

    def __init__(self):
        self.fails = []

    def __call__(self, quantity, measured, bar, op="<=", note=None):
        try:
            check(quantity, measured, bar, op, note)
        except AssertionError as e:
            self.fails.append(str(e))

    def true(self, what, cond):
        if not bool(cond):
            self.fails.append(what)

    def against(self, label, gpu, ref, oracle, floor=REL_FLOOR):
        """err(gpu, float64) <= max(8 err(fp32 oracle, float64), floor) on one tensor."""
        eo = RC.err(oracle, ref)
        eg = RC.err(gpu, ref)
        print("%-44s gpu %.3g  oracle %.3g" % (label, eg, eo))
        self(label, eg, max(FACTOR * eo, floor), note="fp32 oracle err %.3g" % eo)

    def done(self):
        assert not self.fails, "\n".join(self.fails)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


# =========================================================================== sampler
def run_fine(L, c, Nf, inv_s, with_sdf=True):
    """One mli_sample_fine call; the outputs on the CPU, and whether every canary survived."""
    R, Na, Nb = c["R"], c["Na"], c["Nb"]
    da, db = dev(c["da"]), dev(c["db"]) if Nb else None
    sa = dev(c["sa"]) if with_sdf else None
    sb = dev(c["sb"]) if with_sdf and Nb else None
    B = Bufs()
    dout = B.new(Na + Nb, R)
    sout = B.new(Na + Nb, R) if with_sdf else None
    fine = B.new(Nf, R) if Nf else None
    u = (C.c_float * 64)(*(RC.u_fine(Nf).tolist() + [2.0] * (64 - Nf))) if Nf else None
    L.call("mli_sample_fine", L.SampleFineArgs(R, L.ptr(da), L.ptr(sa), Na, L.ptr(db), L.ptr(sb), Nb, L.ptr(dout),
                                               L.ptr(sout), Nf, float(inv_s), C.cast(u, C.c_void_p) if Nf else None,
                                               L.ptr(fine)))
    sync()
    cpu = lambda t: None if t is None else t.cpu()   # noqa: E731
    return dict(dists=cpu(dout), sdf=cpu(sout), fine=cpu(fine), canaries=B.canaries_intact())


def _pairs(d, s):
    """Per ray, the (distance, sdf) pairs in lexicographic order."""
    d, s = d.double().numpy(), s.double().numpy()
    out = np.empty((2,) + d.shape)
    for r in range(d.shape[1]):
        o = np.lexsort((s[:, r], d[:, r]))
        out[0, :, r], out[1, :, r] = d[o, r], s[o, r]
    return out


MERGE_SHAPES = [(5, 64, 16), (37, 192, 64), (1, 1, 4)]


@pytest.mark.parametrize("with_sdf", [True, False], ids=["sdf", "nosdf"])
@pytest.mark.parametrize("R,Na,Nb", MERGE_SHAPES)
@pytest.mark.parametrize("kind", ["tie_free", "no_b", "repeat_a", "repeat_b", "all_last", "unsorted_b"])
def test_merge(L, kind, R, Na, Nb, with_sdf):
    """The merge of mli_sample_fine as the final call of engine.sample uses it (Nf = 0): the sorted
    distances bit for bit, the sdf carried along (within a group of equal distances: the same
    multiset), nothing behind the buffers.  A list b slightly out of order still comes out as a
    permutation of the input."""
    if kind in ("tie_free", "no_b"):
        c = RC.sampler_case(R, Na, Nb if kind == "tie_free" else 0, 7 + Na)
    else:
        c = RC.tie_lists(R, Na, Nb, kind, 9 + Na)
    got = run_fine(L, c, 0, 0.0, with_sdf)
    K = Checks()
    cat_d = torch.cat([c["da"], c["db"]], 0) if c["Nb"] else c["da"]
    cat_s = torch.cat([c["sa"], c["sb"]], 0) if c["Nb"] else c["sa"]
    ref_d = torch.sort(cat_d.double(), dim=0).values
    if kind == "unsorted_b":
        K.true("output multiset != input multiset", torch.equal(torch.sort(got["dists"].double(), dim=0).values, ref_d))
    else:
        K.true("dists_out != float64 sort", torch.equal(got["dists"].double(), ref_d))
    if with_sdf:
        K.true("(dist, sdf) pairs moved apart", np.array_equal(_pairs(got["dists"], got["sdf"]), _pairs(cat_d, cat_s)))
    K.true("canary overwritten", got["canaries"])
    K.done()


_FINE = {}


def fine_case(R, Na, Nb, Nf, inv_s):
    """Inputs, float64 reference and the fp32 oracle's error of a sampler case, built once."""
    key = (R, Na, Nb, Nf, inv_s)
    if key not in _FINE:
        c = RC.sampler_case(R, Na, Nb, 100 + Na + (0 if R == 37 else 1000 * R))
        ref = RR.sample_fine(c["da"], c["sa"], c["db"] if Nb else None, c["sb"] if Nb else None, inv_s, RC.u_fine(Nf))
        o = RC.oracle_fine(ref["dists"].float(), ref["sdf"].float(), inv_s, Nf)
        rays = ref["wsum"] >= WSUM
        near = ref["knot"] < KNOT
        mask = rays[None] & ~near
        n = int(rays.sum()) * Nf
        share = float((near & rays[None]).sum()) / n if n else 0.0
        eo = float((o.double() - ref["fine"])[mask].abs().max()) if bool(mask.any()) else 0.0
        _FINE[key] = dict(c=c, ref=ref, mask=mask, share=share, oracle_err=eo)
    return _FINE[key]


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("Na,Nb,Nf,inv_s", RC.SAMPLER_CASES)
def test_fine_samples(L, Na, Nb, Nf, inv_s, R):
    f = fine_case(R, Na, Nb, Nf, inv_s)
    c, ref, mask = f["c"], f["ref"], f["mask"]
    got = run_fine(L, c, Nf, inv_s)
    K = Checks()
    K.true("dists_out != float64 sort", torch.equal(got["dists"].double(), ref["dists"]))
    K.true("sdf_out != the sorted lists' sdf", torch.equal(got["sdf"].double(), ref["sdf"]))
    # the recipe alone leaves out 0 - 0.2 % (tests/test_rays_ref.py)
    K("share of fine samples within %g of a cdf knot" % KNOT, f["share"], 0.01)
    fine = got["fine"].double()
    if bool(mask.any()):
        eg = float((fine - ref["fine"])[mask].abs().max())
        print("fine R %d %s: compared %d of %d, gpu err %.3g, oracle err %.3g" % (
            R, (Na, Nb, Nf, inv_s), int(mask.sum()), mask.numel(), eg, f["oracle_err"]))
        K("fine dists vs float64", eg, max(FACTOR * f["oracle_err"], DIST_FLOOR),
          note="fp32 oracle err %.3g" % f["oracle_err"])
    if R == 37:
        K.true("no ray compared elementwise", int(mask.sum()) >= Nf)
    out = c["kinds"] == 1
    # outside rays: every alpha is 0, the cdf is flat, every quantile lands on the last distance
    K.true("outside rays: fine != last merged distance", torch.equal(fine[:, out], ref["dists"][-1:, out].expand(Nf, -1)))
    # never-crossing (and weak) rays: the pdf is rounding noise in fp32; finite and inside the list
    K.true("fine sample not finite", torch.isfinite(fine).all())
    K.true("fine sample outside [d_first, d_last]", ((fine >= ref["dists"][:1]) & (fine <= ref["dists"][-1:])).all())
    K.true("canary overwritten", got["canaries"])
    K.done()


@pytest.mark.parametrize("Nc", [1, 16, 64])
@pytest.mark.parametrize("inject", [True, False], ids=["u", "u_null"])
def test_sample_coarse(L, Nc, inject):
    R = 37
    g = torch.Generator().manual_seed(Nc)
    near = torch.rand(R, generator=g) + 0.2
    far = near + torch.rand(R, generator=g) * 2 + 0.1
    u = torch.rand(R, Nc, generator=g) if inject else None
    ref = RR.coarse(near, far, Nc, u)
    from oracle import render as o_render
    o = o_render.stratified_dists(near[None, :, None], far[None, :, None], Nc, None if u is None else u[None])
    eo = float((o[0, :, :, 0].t().double() - ref).abs().max())
    B = Bufs()
    out = B.new(Nc, R)
    dn, df, du = dev(near), dev(far), dev(u)
    L.call("mli_sample_coarse", L.SampleCoarseArgs(L.ptr(dn), L.ptr(df), L.ptr(du), R, Nc, L.ptr(out)))
    sync()
    K = Checks()
    K("coarse dists vs float64", float((out.cpu().double() - ref).abs().max()), max(FACTOR * eo, DIST_FLOOR),
      note="fp32 oracle err %.3g" % eo)
    K.true("canary overwritten", B.canaries_intact())
    K.done()


# =========================================================================== rays
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("mode", ["ray_idx", "first_pixel"])
@pytest.mark.parametrize("bounding", ["sphere", "box"])
def test_rays(L, bounding, mode, R):
    cam = RC.camera(11, bounding)
    W, H = cam["W"], cam["H"]
    if mode == "ray_idx":
        pix = torch.randperm(W * H, generator=torch.Generator().manual_seed(R))[:R].contiguous()
        pix[0] = 0                                                      # an image corner: a miss
    else:
        first = 5 * W + 17                                              # the run wraps over image rows
        pix = torch.arange(first, first + R)
    ref = RR.rays(cam["intr"], cam["pose"], cam["pose_light"], pix, W, bounding, cam["aabb"])
    o = RC.oracle_rays(cam, pix, bounding)
    B = Bufs()
    out = dict(center=B.new(R, 3), ray_unit=B.new(R, 3), ray_norm=B.new(R), pts_light=B.new(R, 3), near=B.new(R),
               far=B.new(R), outside=B.new(R, dtype=torch.uint8))
    K_, P_, PL_ = dev(cam["intr"]), dev(cam["pose"]), dev(cam["pose_light"])
    idx = dev(pix.to(torch.int64)) if mode == "ray_idx" else None
    L.call("mli_rays", L.RaysArgs(L.ptr(K_), L.ptr(P_), L.ptr(PL_), L.ptr(idx), 0 if idx is not None else int(pix[0]),
                                  R, W, 1 if bounding == "box" else 0, (C.c_float * 6)(*cam["aabb"]),
                                  L.ptr(out["center"]), L.ptr(out["ray_unit"]), L.ptr(out["ray_norm"]),
                                  L.ptr(out["pts_light"]), L.ptr(out["near"]), L.ptr(out["far"]),
                                  L.ptr(out["outside"])))
    sync()
    got = {k: v.cpu() for k, v in out.items()}
    K = Checks()
    for k in ("center", "ray_unit", "ray_norm", "pts_light"):
        K.against("rays %s %s R %d: %s" % (bounding, mode, R, k), got[k], ref[k], o[k])
    clear = ref["margin"].abs() > 1e-6
    # with the reference alone no ray of these poses lies that close to the edge
    K("share of rays within 1e-6 of the bound's edge", 1.0 - float(clear.double().mean()), 0.01)
    K.true("outside flags differ", torch.equal(got["outside"].bool()[clear], ref["outside"][clear]))
    if R == 37:
        K.true("no ray misses the volume", ref["outside"].any())
        K.true("no ray hits the volume", (~ref["outside"]).any())
    miss = clear & ref["outside"]
    K.true("a miss is not (near, far) = (1, 1.2)",
           bool((got["near"][miss] == 1.0).all()) and bool((got["far"][miss] == np.float32(1.2)).all()))
    # near / far where they are well conditioned (tests/test_rays_ref.well_conditioned)
    sel = (ref["margin"] >= 0.01) if bounding == "sphere" else ~ref["outside"] & clear
    if bool(sel.any()):
        for k in ("near", "far"):
            K.against("rays %s %s R %d: %s" % (bounding, mode, R, k), got[k][sel], ref[k][sel], o[k][sel])
    K.true("canary overwritten", B.canaries_intact())
    K.done()


# =========================================================================== composite
def composite_bufs(B, R, N):
    return dict(weights=B.new(N, R), rgb=B.new(R, 3), o_r=B.new(R, 3), o_s=B.new(R), o_re=B.new(R, 3),
                opacity=B.new(R), gradient=B.new(R, 3), depth=B.new(R), blend_dist=B.new(R))


def padded_dists(c):
    """The distances with one more row behind them that no kernel may read (NaN): the last
    section ends at ``far``, not at the next row."""
    N, R = c["N"], c["R"]
    full = torch.full((N + 1, R), float("nan"))
    full[:N] = c["dists"]
    full = full.to(DEV)
    return full, full[:N]


def run_fwd(L, c, s_var, anneal, white, with_y=True):
    R, N = c["R"], c["N"]
    keep = [padded_dists(c)] + [dev(c[k]) for k in ("far", "ray_unit", "ray_norm", "sdf", "grad", "y")]
    keep.append(torch.tensor([s_var], dtype=torch.float32, device=DEV))
    (_, dists), far, v, nrm, sdf, grad, y, sv = keep
    B = Bufs()
    o = composite_bufs(B, R, N)
    L.call("mli_composite_fwd", L.CompositeArgs(
        R, N, L.ptr(dists), L.ptr(far), L.ptr(v), L.ptr(nrm), L.ptr(sdf), L.ptr(grad), L.ptr(y) if with_y else None,
        L.ptr(sv), float(anneal), int(white), L.ptr(o["weights"]), L.ptr(o["rgb"]), L.ptr(o["o_r"]), L.ptr(o["o_s"]),
        L.ptr(o["o_re"]), L.ptr(o["opacity"]), L.ptr(o["gradient"]), L.ptr(o["depth"]), L.ptr(o["blend_dist"])))
    sync()
    got = {k: t.cpu() for k, t in o.items()}
    got["canaries"] = B.canaries_intact()
    got["dev"] = o
    return got


_REF = {}


def composite_ref(p):
    """float64 reference and fp32 oracle of a COMPOSITE_CASES entry, built once: forward, the
    geometry backward and the heads' backward with the float64-derived loss gradients."""
    if p not in _REF:
        R, N, anneal, white, s_var = p
        c = RC.composite_inputs(p)
        sv = torch.tensor([s_var])
        args = (c["dists"], c["far"], c["ray_unit"])
        ref = RR.composite(*args, c["ray_norm"], c["sdf"], c["grad"], c["y"], sv, anneal, white)
        d = RC.loss_grads(c, ref)
        geo = RR.composite_bwd_geo(*args, c["sdf"], c["grad"], c["y"], sv, anneal, white, c["d_rgb"], SCALE)
        o = RC.oracle_composite(c, s_var, anneal, white, grads=True)
        _REF[p] = dict(c=c, ref=ref, d=d, geo=geo, o=o)
    return _REF[p]


svar_oracle_err = RC.d_s_var_oracle_err


FWD_TENSORS = ("weights", "rgb", "o_r", "o_s", "o_re", "opacity", "gradient", "depth", "blend_dist")


@pytest.mark.parametrize("p", RC.COMPOSITE_CASES, ids=RC.composite_case_id)
def test_composite_fwd(L, p):
    R, N, anneal, white, s_var = p
    z = composite_ref(p)
    c, ref, o = z["c"], z["ref"], z["o"]
    got = run_fwd(L, c, s_var, anneal, white)
    K = Checks()
    for k in FWD_TENSORS:
        K.against("composite fwd %s: %s" % (RC.composite_case_id(p), k), got[k], ref[k], o[k])
    out = c["kinds"] == 1
    K.true("outside rays: weights not exactly 0", (got["weights"][:, out] == 0).all())
    K.true("canary overwritten", got["canaries"])
    # weights only (y = NULL, the PQ heads' path): the same bits, and no other output written
    alone = run_fwd(L, c, s_var, anneal, white, with_y=False)
    K.true("weights with y = NULL differ", torch.equal(alone["weights"], got["weights"]))
    K.true("y = NULL wrote an output", all(bool((alone[k] == FILL).all()) for k in FWD_TENSORS[1:]))
    K.done()


def test_composite_fwd_across_the_dispatch_switch(L):
    """The same rays cut at N = 128 (two rays per wave, 32-lane scans) and N = 129 (one ray per
    wave, 64-lane scans): the first 128 weights differ only through sample 127's section end
    (far against the next distance), so samples 0..126 are the same bits."""
    p128, p129 = [q for q in RC.COMPOSITE_CASES if q[:2] in ((37, 128), (37, 129))]
    a = run_fwd(L, RC.composite_inputs(p128), p128[4], p128[2], p128[3])
    b = run_fwd(L, RC.composite_inputs(p129), p129[4], p129[2], p129[3])
    assert torch.equal(RC.composite_inputs(p128)["dists"], RC.composite_inputs(p129)["dists"][:128])
    assert torch.equal(a["weights"][:127], b["weights"][:127])
    assert float(a["weights"][:127].max()) > 0.1                        # not a comparison of empty rays


GEO_EXTRA = {"steep": (RC.steep_case, 6.0, RC.ANNEAL_MID, 1), "zero_alpha": (RC.zero_alpha_case, 3.0, 0.0, 1)}


def run_geo(L, c, s_var, anneal, white):
    R, N = c["R"], c["N"]
    keep = [padded_dists(c)] + [dev(c[k]) for k in ("far", "ray_unit", "sdf", "grad", "y", "d_rgb")]
    keep.append(torch.tensor([s_var], dtype=torch.float32, device=DEV))
    (_, dists), far, v, sdf, grad, y, d_rgb, sv = keep
    B = Bufs()
    o = dict(dz4=B.new(N, R, 8), d_sdf=B.new(N, R), d_grad=B.new(N, R, 3), d_inv_s_part=B.new(R), d_s_var=B.new(1))
    args = L.CompositeBwdGeoArgs(R, N, L.ptr(dists), L.ptr(far), L.ptr(v), L.ptr(sdf), L.ptr(grad), L.ptr(y), L.ptr(sv),
                                 float(anneal), int(white), L.ptr(d_rgb), SCALE, L.ptr(o["dz4"]), L.ptr(o["d_sdf"]),
                                 L.ptr(o["d_grad"]), L.ptr(o["d_inv_s_part"]), L.ptr(o["d_s_var"]))
    assert L.workspace("mli_composite_bwd_geo", args) == [N * R * 32, N * R * 4, N * R * 12, R * 4]
    L.call("mli_composite_bwd_geo", args)
    sync()
    got = {k: t.cpu() for k, t in o.items()}
    got["canaries"] = B.canaries_intact()
    return got


def check_geo(K, label, got, c, geo, o, s_var):
    """mli_composite_bwd_geo's outputs against float64 autograd (``geo``, dz4 scaled by SCALE) at
    8 x the fp32 oracle's (``o``, unscaled) error."""
    K.against(label + ": d_sdf", got["d_sdf"], geo["d_sdf"], o["d_sdf"])
    K.against(label + ": d_grad", got["d_grad"], geo["d_grad"], o["d_grad"])
    K.against(label + ": dz4", got["dz4"], geo["dz4"], o["dz4_geo"] * SCALE)
    K.true("dz4 channels 3..7 not exactly 0", (got["dz4"][..., 3:] == 0).all())
    for k in ("d_sdf", "d_grad", "dz4", "d_inv_s_part", "d_s_var"):
        K.true(k + " not finite", torch.isfinite(got[k]).all())
    out = c["kinds"] == 1
    K.true("outside rays: a gradient is not exactly 0",
           all(bool((got[k][:, out] == 0).all()) for k in ("d_sdf", "d_grad", "dz4")) and
           bool((got["d_inv_s_part"][out] == 0).all()))
    K.true("canary overwritten", got["canaries"])
    # d s_var = exp(s_var) sum_r part_r, summed in fp32 by a 256-wide tree (8 levels: a partial
    # takes part in <= 8 additions, each rounding by <= 2^-24 of a partial sum <= sum |part|),
    # times expf (<= 2 ulps = 4 x 2^-24) and one product (2^-24): <= 13 x 2^-24, asserted at 16
    part = got["d_inv_s_part"].double()
    inv_s = float(torch.tensor(s_var, dtype=torch.float64).exp())
    total = float(got["d_s_var"][0])
    K(label + ": |exp(s_var) sum(d_inv_s_part) - d_s_var|", abs(float(part.sum()) * inv_s - total),
      16 * 2.0 ** -24 * max(float(part.abs().sum()) * inv_s, 1e-30))


@pytest.mark.parametrize("p", RC.COMPOSITE_CASES, ids=RC.composite_case_id)
def test_composite_bwd_geo(L, p):
    R, N, anneal, white, s_var = p
    z = composite_ref(p)
    label = "bwd_geo " + RC.composite_case_id(p)
    got = run_geo(L, z["c"], s_var, anneal, white)
    K = Checks()
    check_geo(K, label, got, z["c"], z["geo"], z["o"], s_var)
    eo, worst = RC.err(z["o"]["d_s_var"], z["geo"]["d_s_var"]), svar_oracle_err()
    eg = RC.err(got["d_s_var"], z["geo"]["d_s_var"])
    print("%-44s gpu %.3g  oracle %.3g (worst case %.3g)" % (label + ": d_s_var", eg, eo, worst))
    K(label + ": d_s_var", eg, max(FACTOR * worst, REL_FLOOR),
      note="fp32 oracle err %.3g on this case, %.3g the largest over the cases" % (eo, worst))
    K.done()


@pytest.mark.parametrize("name", list(GEO_EXTRA))
def test_composite_bwd_geo_at_the_clamp_bounds(L, name):
    """steep: a sample at the largest alpha the formula gives (1 - alpha = 1e-5; the suffix
    recurrence divides by nothing).  zero_alpha: x = 0 exactly on every sample, where the clamp's
    inclusive bound passes the gradient into grad (tests/rays_cases.py)."""
    make, s_var, anneal, white = GEO_EXTRA[name]
    c = make()
    geo = RR.composite_bwd_geo(c["dists"], c["far"], c["ray_unit"], c["sdf"], c["grad"], c["y"], torch.tensor([s_var]),
                               anneal, white, c["d_rgb"], SCALE)
    o = RC.oracle_composite(c, s_var, anneal, white, grads=True)
    got = run_geo(L, c, s_var, anneal, white)
    K = Checks()
    check_geo(K, "bwd_geo " + name, got, c, geo, o, s_var)
    fwd = run_fwd(L, c, s_var, anneal, white)
    K.against("composite fwd %s: weights" % name, fwd["weights"], geo["weights"], o["weights"])
    if name == "zero_alpha":
        K.true("zero_alpha: a weight is not exactly 0", (fwd["weights"] == 0).all())
        K.true("zero_alpha: a sample's d_grad is 0", (got["d_grad"].abs().amax(-1) > 0).all())
    else:
        # alpha_k = w_k / T_k on the rays that still see sample k (float64 T_k > 1e-3).  The GPU's
        # w_k carries the roundings of T_k, a product of k factors 1 - alpha (each factor and each
        # product <= 2^-24 relative), and of alpha_k itself: 4 (k + 1) 2^-24 bounds them twice over
        k = c["N"] // 2
        t = (1 - geo["alpha"][:k]).prod(0)
        live = t > 1e-3
        K.true("steep: no ray reaches sample k", int(live.sum()) >= 2)
        K("steep: |w_k / T_k - 1 / (1 + 1e-5)|", float((fwd["weights"][k].double() / t)[live].sub(RC.ALPHA_MAX).abs().max()),
          4 * (k + 1) * 2.0 ** -24)
        # d s_var of these five rays against float64 (one number: 8 x the case list's largest error)
        K("bwd_geo steep: d_s_var", RC.err(got["d_s_var"], geo["d_s_var"]),
          max(FACTOR * max(svar_oracle_err(), RC.err(o["d_s_var"], geo["d_s_var"])), REL_FLOOR))
    K.done()


NULLED = [None, 0, 1, 2, 3]     # which of d_rgb, d_o_r, d_o_s, d_o_re is passed as NULL


@pytest.mark.parametrize("p", RC.COMPOSITE_CASES, ids=RC.composite_case_id)
def test_composite_bwd(L, p):
    """mli_composite_bwd on the forward kernel's own weights, o_r, o_s, fed the loss gradients of
    the float64 outputs: dz4 and dray against float64 autograd, with all four gradients and with
    each passed as NULL in turn."""
    R, N, anneal, white, s_var = p
    z = composite_ref(p)
    c = z["c"]
    fwd = run_fwd(L, c, s_var, anneal, white)["dev"]
    y = dev(c["y"])
    dd = [dev(t) for t in z["d"]]
    sv = torch.tensor([s_var])
    K = Checks()
    for nulled in NULLED:
        d = [None if i == nulled else t for i, t in enumerate(z["d"])]
        ref = RR.composite_bwd(c["dists"], c["far"], c["ray_unit"], c["sdf"], c["grad"], c["y"], sv, anneal, white, *d,
                               SCALE)
        o = RC.oracle_composite(c, s_var, anneal, white, d=d)
        B = Bufs()
        dz4, dray = B.new(N, R, 8), B.new(R, 8)
        ptrs = [None if i == nulled else L.ptr(t) for i, t in enumerate(dd)]
        L.call("mli_composite_bwd", L.CompositeBwdArgs(R, N, L.ptr(fwd["weights"]), L.ptr(y), L.ptr(fwd["o_r"]),
                                                       L.ptr(fwd["o_s"]), *ptrs, SCALE, L.ptr(dz4), L.ptr(dray)))
        sync()
        label = "composite bwd %s null %s" % (RC.composite_case_id(p), nulled)
        K.against(label + ": dz4", dz4.cpu(), ref["dz4"], o["dz4"] * SCALE)
        K.against(label + ": dray", dray.cpu(), ref["dray"], o["dray"])
        K.true("dz4 / dray channel 7 not exactly 0", bool((dz4[..., 7] == 0).all()) and bool((dray[:, 7] == 0).all()))
        K.true("canary overwritten", B.canaries_intact())
    K.done()


# =========================================================================== error convention
def test_error_convention(L):
    """Invalid sizes return hipErrorInvalidValue on the host, before any launch; R = 0 returns
    success and writes nothing."""
    R = 4
    big = torch.zeros(260 * R, device=DEV)
    B = Bufs()
    out = [B.new(260, R) for _ in range(3)]
    u = (C.c_float * 64)(*([0.5] * 64))
    up = C.cast(u, C.c_void_p)
    p = L.ptr

    def fine(R_, Na, Nb, Nf, sdf_out=True):
        return L.SampleFineArgs(R_, p(big), p(big), Na, p(big), p(big), Nb, p(out[0]), p(out[1]) if sdf_out else None,
                                Nf, 64.0, up, p(out[2]))

    for bad in (fine(R, 16, 4, 65), fine(R, 16, 65, 4), fine(R, 0, 4, 4), fine(R, 200, 57, 4),
                fine(R, 16, 4, 4, sdf_out=False)):
        with pytest.raises(RuntimeError, match="mli_sample_fine"):
            L.call("mli_sample_fine", bad)
    sv = torch.tensor([3.0], device=DEV)

    def fwd(R_, N):
        return L.CompositeArgs(R_, N, p(big), p(big), p(big), p(big), p(big), p(big), p(big), p(sv), 0.3, 1, p(out[0]),
                               p(out[1]), p(out[1]), p(out[1]), p(out[1]), None, None, None, None)

    def geo(R_, N, part=True):
        return L.CompositeBwdGeoArgs(R_, N, p(big), p(big), p(big), p(big), p(big), p(big), p(sv), 0.3, 1, p(big), SCALE,
                                     p(out[0]), p(out[1]), p(out[2]), p(out[1]) if part else None, p(out[1]))

    with pytest.raises(RuntimeError, match="mli_composite_fwd"):
        L.call("mli_composite_fwd", fwd(R, 257))
    with pytest.raises(RuntimeError, match="mli_composite_bwd_geo"):
        L.call("mli_composite_bwd_geo", geo(R, 257))
    with pytest.raises(RuntimeError, match="mli_composite_bwd_geo"):
        L.call("mli_composite_bwd_geo", geo(R, 16, part=False))
    L.call("mli_sample_fine", fine(0, 16, 4, 4))
    L.call("mli_composite_fwd", fwd(0, 16))
    L.call("mli_composite_bwd_geo", geo(0, 16))
    L.call("mli_composite_bwd", L.CompositeBwdArgs(0, 16, p(big), p(big), p(big), p(big), p(big), p(big), p(big), p(big),
                                                   SCALE, p(out[0]), p(out[1])))
    L.call("mli_sample_coarse", L.SampleCoarseArgs(p(big), p(big), None, 0, 16, p(out[0])))
    L.call("mli_rays", L.RaysArgs(p(big), p(big), p(big), None, 0, 0, 8, 0, (C.c_float * 6)(*([0.0] * 6)), p(out[0]),
                                  p(out[0]), p(out[0]), p(out[0]), p(out[0]), p(out[0]), p(out[0])))
    sync()
    assert B.untouched()
