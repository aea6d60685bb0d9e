"""Seeded input recipes of the per-ray kernel tests, and the fp32 oracle's evaluation of the same
inputs (oracle/render.py, [B][R][N] layout).  Shared by tests/test_rays_ref.py (CPU) and
tests/test_gpu_rays.py, so that the error of the fp32 oracle against the float64 restatement --
the yardstick of every GPU bar -- is measured on exactly the inputs the kernels see.

All tensors are CPU float32 in the kernels' layout: per-sample arrays [N][R]."""
import numpy as np
import torch
import torch.nn.functional as F

import rays_ref
from oracle import render as o_render

ANNEAL_MID = float(np.float32(0.3))      # the anneal blend as the kernel's float argument holds it


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit(g, R):
    return F.normalize(torch.rand(R, 3, generator=g) - 0.5, dim=-1)


def sorted_dists(g, N, R):
    return torch.sort(torch.rand(N, R, generator=g) * 2.0 + 0.5, dim=0).values.contiguous()


def ray_kinds(R):
    """0 = a surface crossing, 1 = outside (sdf 1000), 2 = never crosses (|sdf| + 0.05); every
    R >= 5 holds all three, a single ray is a crossing."""
    kinds = torch.zeros(R, dtype=torch.int64)
    if R >= 5:
        kinds[3::7] = 1
        kinds[4::7] = 2
    return kinds


def sdf_model(g, d, d0, c, kinds):
    """sdf = (d0 - d) c + 0.01 noise along each ray, then the two further kinds."""
    sdf = (d0[None] - d) * c[None] + 0.01 * torch.randn(d.shape, generator=g)
    sdf = torch.where(kinds[None] == 2, sdf.abs() + 0.05, sdf)
    return torch.where(kinds[None] == 1, torch.full_like(sdf, 1000.0), sdf).contiguous()


# --------------------------------------------------------------------------- composite
def composite_case(R, N, seed, backward=True):
    """Rays for the composite kernels.  The crossing depth d0 is uniform over the whole range, so
    crossings land in late lanes too.  ``backward``: samples whose cos = v . grad lies within
    1e-3 of 0 or 1, where the relu gates of _get_iter_cos are discontinuous, are drawn again."""
    g = _gen(seed)
    dists = sorted_dists(g, N, R)
    far = dists[-1] + 0.1
    v = _unit(g, R)
    kinds = ray_kinds(R)
    d0 = torch.rand(R, generator=g) * 2.0 + 0.5
    c = torch.rand(R, generator=g) * 0.7 + 0.3
    sdf = sdf_model(g, dists, d0, c, kinds)
    grad = -c[None, :, None] * v[None] + 0.3 * torch.randn(N, R, 3, generator=g)
    for _ in range(64 if backward else 0):
        cos = (v[None].double() * grad.double()).sum(-1)
        bad = (cos.abs() < 1e-3) | ((cos - 1.0).abs() < 1e-3)
        if not bool(bad.any()):
            break
        fresh = -c[None, :, None] * v[None] + 0.3 * torch.randn(N, R, 3, generator=g)
        grad = torch.where(bad[..., None], fresh, grad)
    y = (torch.rand(N, R, 8, generator=g) * 0.98 + 0.01).contiguous()
    return dict(R=R, N=N, dists=dists, far=far.contiguous(), ray_unit=v.contiguous(),
                ray_norm=(torch.rand(R, generator=g) + 0.5).contiguous(), sdf=sdf, grad=grad.contiguous(), y=y,
                kinds=kinds, d_rgb=torch.randn(R, 3, generator=g).contiguous(),
                d_o_r=torch.randn(R, 3, generator=g).contiguous(), d_o_s=torch.randn(R, 1, generator=g).contiguous(),
                d_o_re=torch.randn(R, 3, generator=g).contiguous())


def cut(case, N):
    """The same rays cut at N samples (far unchanged: the last section then ends at far)."""
    out = dict(case)
    out.update(N=N, dists=case["dists"][:N].contiguous(), sdf=case["sdf"][:N].contiguous(),
               grad=case["grad"][:N].contiguous(), y=case["y"][:N].contiguous())
    return out


ALPHA_MAX = float(np.float32(1.0) / (np.float32(1.0) + np.float32(1e-5)))


def steep_case(R=5, N=37, seed=77):
    """Rays whose sample N // 2 owns a section that falls from a large positive to a large
    negative sdf: a gap of 1.0 in the distances at sdf 0 and cos -2, so the section ends are
    sdf +-(0.75 .. 1) and at s_var = 6 cdf_prev = 1, cdf_next = 0 exactly in fp32.  That is the
    largest alpha the formula can give, 1 / (1 + 1e-5) = ALPHA_MAX (the 1e-5 in the denominator
    keeps x below 1), and the transmittance behind it drops by 1e-5: where a backward that
    divided by 1 - alpha would lose its digits."""
    case = composite_case(R, N, seed)
    k = N // 2
    d = case["dists"].clone()
    # a gap of 1.0 after sample k: shift the rest of the ray outwards
    d[k + 1:] += 1.0
    case["dists"] = d.contiguous()
    case["far"] = (d[-1] + 0.1).contiguous()
    v = case["ray_unit"]
    case["sdf"][k] = 0.0
    case["grad"][k] = -v * 2.0          # cos = -2: the section spans sdf +-(0.5 .. 1) around 0
    case["kinds"] = torch.zeros(R, dtype=torch.int64)
    case["sdf"] = torch.where(case["sdf"] == 1000.0, torch.full_like(case["sdf"], 0.3), case["sdf"])
    return case


def zero_alpha_case(R=5, N=37, seed=78):
    """Rays whose every section is so short (1-2 ulps of a distance in [1, 2)) and so nearly
    parallel to the gradient (cos in [0.99, 0.998], anneal 0: |iter_cos| <= 0.005) that
    sdf -+ iter_cos step / 2 rounds back to sdf in fp32 (|sdf| in [0.05, 0.12], half an ulp
    >= 1.8e-9 against a shift <= 6e-10): x = 0 exactly, on the clamp's inclusive bound, while the
    derivative of x w.r.t. iter_cos is not 0.  The gradient w.r.t. grad there is what torch's
    clamp passes at the bound."""
    g = _gen(seed)
    ulp = 2.0 ** -23
    steps = torch.randint(1, 3, (N, R), generator=g).float() * ulp
    dists = (1.0 + torch.rand(R, generator=g) * 0.5)[None] + torch.cumsum(steps, 0) - steps[:1]
    far = dists[-1] + ulp
    v = _unit(g, R)
    sdf = (torch.rand(N, R, generator=g) * 0.07 + 0.05) * torch.where(torch.rand(N, R, generator=g) < 0.5, -1.0, 1.0)
    cos = torch.rand(N, R, generator=g) * 0.008 + 0.99
    perp = torch.randn(N, R, 3, generator=g)
    perp = F.normalize(perp - (perp * v[None]).sum(-1, keepdim=True) * v[None], dim=-1)
    grad = cos[..., None] * v[None] + 0.2 * perp
    y = (torch.rand(N, R, 8, generator=g) * 0.98 + 0.01).contiguous()
    return dict(R=R, N=N, dists=dists.contiguous(), far=far.contiguous(), ray_unit=v.contiguous(),
                ray_norm=torch.ones(R), sdf=sdf.contiguous(), grad=grad.contiguous(), y=y,
                kinds=torch.zeros(R, dtype=torch.int64), d_rgb=torch.randn(R, 3, generator=g).contiguous())


# (R, N, anneal, white_bg, s_var): every N of {1, 3, 37, 128, 129, 255, 256} (the dispatch switches
# at 128), every R of {1, 5, 37}, every anneal, both backgrounds, both s_var.  The two
# (37, 128 / 129) cases are the same rays cut at both lengths.
COMPOSITE_CASES = [
    (37, 1, 0.0, 1, 3.0), (5, 3, ANNEAL_MID, 0, 3.0), (37, 37, 1.0, 1, 6.0), (1, 37, ANNEAL_MID, 1, 6.0),
    (5, 128, 0.0, 0, 3.0), (37, 128, ANNEAL_MID, 1, 6.0), (37, 129, ANNEAL_MID, 1, 6.0), (5, 129, 0.0, 1, 3.0),
    (5, 255, 1.0, 0, 3.0), (37, 255, ANNEAL_MID, 0, 3.0), (37, 256, 0.0, 1, 6.0), (1, 256, 1.0, 0, 6.0),
]
_COMPOSITE = {}


def composite_case_id(p):
    return "R%d_N%d_an%.1f_bg%d_s%d" % p


def composite_inputs(p):
    """The seeded inputs of a COMPOSITE_CASES entry, built once."""
    if p not in _COMPOSITE:
        R, N = p[:2]
        if (R, N) in ((37, 128), (37, 129)):
            if "pair" not in _COMPOSITE:
                _COMPOSITE["pair"] = composite_case(37, 129, 4000)
            _COMPOSITE[p] = cut(_COMPOSITE["pair"], N)
        else:
            _COMPOSITE[p] = composite_case(R, N, 4001 + COMPOSITE_CASES.index(p))
    return _COMPOSITE[p]


def err(a, ref):
    """max |a - ref| over max |ref| of a tensor (max |a| where the reference is all 0)."""
    a, ref = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    scale = float(ref.abs().max())
    return float((a - ref).abs().max()) / (scale if scale > 0 else 1.0)


def d_s_var_oracle_err():
    """The largest error of the fp32 oracle's d s_var against float64 over COMPOSITE_CASES."""
    if "svar" not in _COMPOSITE:
        worst = 0.0
        for p in COMPOSITE_CASES:
            c = composite_inputs(p)
            geo = rays_ref.composite_bwd_geo(c["dists"], c["far"], c["ray_unit"], c["sdf"], c["grad"], c["y"],
                                             torch.tensor([p[4]]), p[2], p[3], c["d_rgb"], 1.0)
            o = oracle_composite(c, p[4], p[2], p[3], grads=True)
            worst = max(worst, err(o["d_s_var"], geo["d_s_var"]))
        _COMPOSITE["svar"] = worst
    return _COMPOSITE["svar"]


def loss_grads(case, ref):
    """d total / d (rgb, o_r, o_s, o_re) of a squared-error loss on the float64 outputs against
    seeded targets (the outputs plus the case's noise), as fp32 tensors."""
    return tuple((ref[k].reshape(case[n].shape) + case[n].double()).float().contiguous()
                 for k, n in (("rgb", "d_rgb"), ("o_r", "d_o_r"), ("o_s", "d_o_s"), ("o_re", "d_o_re")))


def _brn(t, c):
    """[N][R](c) -> the oracle's [1][R][N][c]."""
    N, R = t.shape[:2]
    return t.reshape(N, R, c).permute(1, 0, 2)[None].contiguous()


def _nr(t):
    """The oracle's [1][R][N][c] -> [N][R](c)."""
    t = t[0].permute(1, 0, 2)
    return t[..., 0] if t.shape[-1] == 1 else t


def oracle_composite(case, s_var, anneal, white_bg, grads=False, d=None):
    """The fp32 oracle on a composite case: neus_alphas + exclusive_transmittance_weights and the
    composited sums as render_rays forms them.  ``grads``: also torch autograd of
    sum(rgb d_rgb) (the stage-a backward) into sdf, grad, s_var; ``d`` = (d_rgb, d_o_r, d_o_s,
    d_o_re), each a tensor or None: autograd of their sum into y -> dz4 / grad_scale and dray."""
    N, R = case["N"], case["R"]
    sv = torch.tensor([float(s_var)], requires_grad=True)
    sdfs = _brn(case["sdf"], 1).requires_grad_(True)
    gr = _brn(case["grad"], 3).requires_grad_(True)
    ys = _brn(case["y"], 8).requires_grad_(True)
    v = case["ray_unit"][None]
    alphas = o_render.neus_alphas(sv[0], v, sdfs, gr, _brn(case["dists"], 1), case["far"].reshape(1, R, 1),
                                  anneal, 1.0)
    w = o_render.exclusive_transmittance_weights(alphas)                  # [1][R][N][1]
    opacity = w.sum(2)
    acc = (ys[..., :7] * w).sum(2)
    if white_bg:
        acc = acc + (1 - opacity)
    acc.retain_grad()
    rgb, o_r, o_s = acc[..., :3], acc[..., 3:6], acc[..., 6:7]
    o_re = rgb - o_r * o_s
    blend = (_brn(case["dists"], 1) * w).sum(2)
    out = dict(weights=_nr(w), rgb=rgb[0], o_r=o_r[0], o_s=o_s[0, :, 0], o_re=o_re[0], opacity=opacity[0, :, 0],
               gradient=(gr * w).sum(2)[0], blend_dist=blend[0, :, 0],
               depth=blend[0, :, 0] / case["ray_norm"])
    out = {k: t.detach() for k, t in out.items()}
    if grads:
        (rgb[0] * case["d_rgb"]).sum().backward(retain_graph=d is not None)
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # noqa: E731
        yd = case["y"]
        dz = torch.zeros(N, R, 8)
        dz[..., :3] = out["weights"][..., None] * case["d_rgb"][None] * (yd[..., :3] * (1 - yd[..., :3]))
        out.update(d_sdf=_nr(zero(sdfs)), d_grad=_nr(zero(gr)), d_s_var=zero(sv).clone(), dz4_geo=dz)
    if d is not None:
        for t in (sdfs, gr, ys, sv, acc):
            t.grad = None
        loss = 0.0
        for val, g in zip((rgb[0], o_r[0], o_s[0], o_re[0]), d):
            if g is not None:
                loss = loss + (val * g.reshape(val.shape)).sum()
        dz, dray = torch.zeros(N, R, 8), torch.zeros(R, 8)
        if torch.is_tensor(loss):
            loss.backward()
            yd = case["y"]
            dz[..., :7] = _nr(ys.grad)[..., :7] * (yd[..., :7] * (1 - yd[..., :7]))
            dray[:, :7] = acc.grad[0]
        out.update(dz4=dz, dray=dray)
    return out


# --------------------------------------------------------------------------- sampler
SAMPLER_CASES = [(16, 0, 4, 64.0), (2, 0, 1, 64.0), (64, 16, 16, 128.0), (115, 16, 16, 256.0),
                 (192, 64, 64, 512.0), (191, 64, 63, 512.0), (1, 4, 3, 512.0)]


def u_fine(n_fine):
    """The midpoint quantiles as nerf_util.sample_dists_from_pdf builds them (fp32)."""
    grid = torch.linspace(0, 1, n_fine + 1)
    return (0.5 * (grid[:-1] + grid[1:])).contiguous()


def sampler_case(R, Na, Nb, seed):
    """Two tie-free sorted lists a [Na][R], b [Nb][R] over [0.5, 2.5] with the sdf of one linear
    crossing per ray (or of the two further kinds)."""
    g = _gen(seed)
    while True:
        d = torch.rand(Na + Nb, R, generator=g) * 2.0 + 0.5
        if all(torch.unique(d[:, r]).numel() == Na + Nb for r in range(R)):
            break
    da = torch.sort(d[:Na], dim=0).values.contiguous()
    db = torch.sort(d[Na:], dim=0).values.contiguous()
    kinds = ray_kinds(R)
    d0 = torch.rand(R, generator=g) * 2.0 + 0.5
    c = torch.rand(R, generator=g) * 0.7 + 0.3
    s = sdf_model(g, torch.cat([da, db], 0), d0, c, kinds)
    return dict(R=R, Na=Na, Nb=Nb, da=da, db=db, sa=s[:Na].contiguous(), sb=s[Na:].contiguous(), kinds=kinds)


def oracle_fine(dists, sdf, inv_s, n_fine):
    """The fp32 oracle's fine samples [Nf][R] of merged lists [Nh][R]."""
    return _nr(o_render.section_pdf_samples(_brn(dists, 1), _brn(sdf, 1), inv_s, n_fine))


def tie_lists(R, Na, Nb, kind, seed):
    """Merge inputs with ties (distances from a coarse grid, so equal values are frequent):
    'repeat_a'   b repeats values of a;
    'repeat_b'   b repeats its own values (and some of a's);
    'all_last'   every b equals a's last element (what outside rays produce);
    'unsorted_b' b slightly out of order (neighbours swapped).  The sdf values are distinct."""
    g = _gen(seed)
    da = torch.sort(torch.randint(0, 4 * Na, (Na, R), generator=g).float() / 64.0 + 0.5, dim=0).values
    if kind == "repeat_a":
        db = da.gather(0, torch.randint(0, Na, (Nb, R), generator=g))
    elif kind == "repeat_b":
        few = da.gather(0, torch.randint(0, Na, (max(Nb // 4, 1), R), generator=g)) + \
            torch.randint(0, 2, (max(Nb // 4, 1), R), generator=g).float() / 128.0
        db = few.gather(0, torch.randint(0, few.shape[0], (Nb, R), generator=g))
    elif kind == "all_last":
        db = da[-1:].expand(Nb, R)
    else:
        db = torch.sort(torch.rand(Nb, R, generator=g) * 2.0 + 0.5, dim=0).values.clone()
        for j in range(0, Nb - 1, 3):
            db[[j, j + 1]] = db[[j + 1, j]]
    if kind != "unsorted_b":
        db = torch.sort(db, dim=0).values
    n = Na + Nb
    s = (torch.randperm(n * R, generator=g).float().reshape(n, R) + 1.0) / 8.0
    return dict(R=R, Na=Na, Nb=Nb, da=da.contiguous(), db=db.contiguous(), sa=s[:Na].contiguous(),
                sb=s[Na:].contiguous())


# --------------------------------------------------------------------------- rays
def camera(seed, bounding):
    """A pinhole camera looking at the unit volume from a distance at which about a third of
    the image misses it; the image is 24 x 17 pixels (a width that divides no tested R)."""
    g = _gen(seed)
    W, H = 24, 17
    eye = F.normalize(torch.rand(3, generator=g) - 0.5, dim=0) * 2.6
    fwd = F.normalize(-eye + 0.1 * (torch.rand(3, generator=g) - 0.5), dim=0)
    up = torch.tensor([0.13, 0.95, 0.2])
    right = F.normalize(torch.linalg.cross(fwd, up), dim=0)
    down = torch.linalg.cross(fwd, right)
    rot = torch.stack([right, down, fwd], 0)                           # w2c rotation
    pose = torch.cat([rot, -(rot @ eye)[:, None]], 1).contiguous()
    f = 20.0 if bounding == "sphere" else 16.0
    intr = torch.tensor([[f, 0.0, W / 2 + 0.3], [0.0, f * 1.05, H / 2 - 0.2], [0.0, 0.0, 1.0]])
    leye = F.normalize(torch.rand(3, generator=g) - 0.5, dim=0) * 3.0
    lrot = rot[[1, 2, 0]]
    pose_light = torch.cat([lrot, -(lrot @ leye)[:, None]], 1).contiguous()
    return dict(W=W, H=H, intr=intr.contiguous(), pose=pose, pose_light=pose_light,
                aabb=(-0.8, -0.7, -0.9, 0.9, 0.8, 0.7))


def oracle_rays(cam, pix, bounding):
    """The fp32 oracle's rays of flat pixels ``pix``: pixel_rays, F.normalize, the bounds."""
    pix = pix.reshape(1, -1)
    center, ray = o_render.pixel_rays(cam["pose"][None], cam["intr"][None], pix, cam["W"], cam["H"])
    v = F.normalize(ray, dim=-1)
    if bounding == "box":
        near, far, outside = o_render.aabb_bounds(center, v, cam["aabb"])
    else:
        near, far, outside = o_render.sphere_bounds(center, v)
    light = o_render.light_points(cam["pose_light"][None], cam["W"] * cam["H"])[0, pix[0]]
    return dict(center=center[0], ray_unit=v[0], ray_norm=ray[0].norm(dim=-1), pts_light=light, near=near[0, :, 0],
                far=far[0, :, 0], outside=outside[0, :, 0])
