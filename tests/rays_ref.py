"""Float64 restatement of the per-ray kernels of csrc/rays.hip, per-sample arrays [N][R].

Written from the reference's formulas (the line references are the ones rays.hip cites), not by
calling oracle/render.py: tests/test_rays_ref.py pins it to the oracle's fp32 functions, and
tests/test_gpu_rays.py compares every kernel with it.  Plain torch in float64; no GPU, no
library, no oracle.  Inputs are taken as given (fp32 values are upcast exactly), so the only
difference to an fp32 evaluation of the same formulas is that evaluation's own rounding."""
import torch
import torch.nn.functional as F

F64 = torch.float64


def _d(t):
    return None if t is None else torch.as_tensor(t).to(F64)


# --------------------------------------------------------------------------- sampling
def coarse(near, far, n, u=None):
    """nerf_util.py:20-38 sample_dists: ((u + k) / n) (far - near) + near -> [n][R]; u [R][n]
    injected uniforms (None -> 0.5)."""
    near, far = _d(near).reshape(-1), _d(far).reshape(-1)
    uu = torch.full((near.numel(), n), 0.5, dtype=F64) if u is None else _d(u).reshape(-1, n)
    t = (uu.t() + torch.arange(n, dtype=F64)[:, None]) / n
    return t * (far - near)[None] + near[None]


def merge(da, sa, db, sb):
    """torch.sort(cat(a, b)) (neuralangelo/model.py:461) as a stable sort by distance, the sdf
    carried along: (dists [Na + Nb][R], sdf or None, order).  Among equal distances list a comes
    first, then list b, each in index order."""
    d = da if db is None or db.shape[0] == 0 else torch.cat([da, db], 0)
    out, order = torch.sort(d, dim=0, stable=True)
    s = None
    if sa is not None:
        s = sa if sb is None or sb.shape[0] == 0 else torch.cat([sa, sb], 0)
        s = s.gather(0, order)
    return out, s, order


def section_cdf(d, s, inv_s):
    """neuralangelo/model.py:467-482 (robust cos) + render.py:87-99 + nerf_util.py:41-57 on merged
    lists d, s [Nh][R]: the section alphas [Nh - 1][R], their exclusive-transmittance weights,
    the L1-normalised pdf (denominator clamped at 1e-12), the cdf with the leading 0 [Nh][R] and
    the unnormalised weight sum per ray."""
    d, s = _d(d), _d(s)
    ds = d[1:] - d[:-1]
    mid = (s[:-1] + s[1:]) * 0.5
    cos = (s[1:] - s[:-1]) / (ds + 1e-5)
    prev = torch.cat([torch.zeros_like(cos[:1]), cos[:-1]], 0)
    cos = torch.minimum(prev, cos)
    cdf_prev = torch.sigmoid((mid - cos * ds * 0.5) * inv_s)
    cdf_next = torch.sigmoid((mid + cos * ds * 0.5) * inv_s)
    alpha = ((cdf_prev - cdf_next) / (cdf_prev + 1e-5)).clamp(0.0, 1.0)
    trans = torch.cat([torch.ones_like(alpha[:1]), (1.0 - alpha[:-1]).cumprod(0)], 0)
    w = alpha * trans
    wsum = w.abs().sum(0)
    pdf = w / wsum.clamp_min(1e-12)[None]
    cdf = torch.cat([torch.zeros_like(pdf[:1]), pdf.cumsum(0)], 0)
    return dict(alpha=alpha, w=w, pdf=pdf, cdf=cdf, wsum=wsum)


def inverse_cdf(d, cdf, u):
    """nerf_util.py:58-68: idx = searchsorted(cdf, u, right) = #{k : cdf_k <= u}, the sample
    interpolated between knots idx - 1 and idx (both clamped to the list) with the 1e-8 in the
    denominator -> (fine [Nf][R], the distance of each u to the nearest cdf knot [Nf][R])."""
    d, cdf, u = _d(d), _d(cdf), _d(u).reshape(-1)
    n = cdf.shape[0]
    idx = (cdf[None] <= u[:, None, None]).sum(1)                       # [Nf][R]
    lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=n - 1)
    d0, d1 = d.gather(0, lo), d.gather(0, hi)
    c0, c1 = cdf.gather(0, lo), cdf.gather(0, hi)
    t = (u[:, None] - c0) / (c1 - c0 + 1e-8)
    knot = (cdf[None] - u[:, None, None]).abs().amin(1)
    return d0 + t * (d1 - d0), knot


def sample_fine(da, sa, db, sb, inv_s, u):
    """One round of sample_dists_hierarchical: merge, section cdf, inverse cdf."""
    d, s, order = merge(_d(da), _d(sa), _d(db), _d(sb))
    sec = section_cdf(d, s, inv_s)
    fine, knot = inverse_cdf(d, sec["cdf"], u)
    return dict(dists=d, sdf=s, order=order, fine=fine, knot=knot, wsum=sec["wsum"], cdf=sec["cdf"])


# --------------------------------------------------------------------------- composite
def composite(dists, far, ray_unit, ray_norm, sdf, grad, y, s_var, anneal, white_bg, inv_s=None):
    """NeuS alphas (neuralangelo/model.py:492-515: _get_iter_cos with the anneal blend, `far` the
    end of the last section), weights (render.py:87-99) and the composited outputs
    (NeuralLumen/model.py:266-305).  dists, sdf [N][R], grad [N][R][3], y [N][R][8] (rgb 0-2,
    o_r 3-5, o_s 6; None -> alphas and weights only), far / ray_norm [R], ray_unit [R][3], s_var
    a one-element tensor.  ``inv_s`` [R] replaces exp(s_var) (the backward's per-ray partials)."""
    dists, far, v, sdf, grad = _d(dists), _d(far).reshape(-1), _d(ray_unit), _d(sdf), _d(grad)
    if inv_s is None:
        inv_s = _d(s_var).reshape(-1)[:1].exp()
    cos = (v[None] * grad).sum(-1)
    iter_cos = -(torch.relu(-cos * 0.5 + 0.5) * (1.0 - anneal) + torch.relu(-cos) * anneal)
    step = torch.cat([dists[1:], far[None]], 0) - dists
    cdf_prev = torch.sigmoid((sdf - iter_cos * step * 0.5) * inv_s)
    cdf_next = torch.sigmoid((sdf + iter_cos * step * 0.5) * inv_s)
    x = (cdf_prev - cdf_next) / (cdf_prev + 1e-5)
    alpha = x.clamp(0.0, 1.0)
    trans = torch.cat([torch.ones_like(alpha[:1]), (1.0 - alpha[:-1]).cumprod(0)], 0)
    w = alpha * trans
    out = dict(cos=cos, x=x, alpha=alpha, weights=w)
    if y is None:
        return out
    y = _d(y)
    opacity = w.sum(0)
    acc = (y[..., :7] * w[..., None]).sum(0)                           # [R][7]
    if white_bg:
        acc = acc + (1.0 - opacity)[:, None]
    rgb, o_r, o_s = acc[:, :3], acc[:, 3:6], acc[:, 6:7]
    blend = (dists * w).sum(0)
    out.update(acc=acc, rgb=rgb, o_r=o_r, o_s=o_s, o_re=rgb - o_r * o_s, opacity=opacity,
               gradient=(grad * w[..., None]).sum(0), blend_dist=blend, depth=blend / _d(ray_norm).reshape(-1))
    return out


def composite_bwd_geo(dists, far, ray_unit, sdf, grad, y, s_var, anneal, white_bg, d_rgb, grad_scale):
    """mli_composite_bwd_geo by float64 autograd through ``composite`` of sum(rgb * d_rgb):
    d_sdf [N][R], d_grad [N][R][3], d_s_var (one element), the per-ray d / d inv_s [R] (they sum
    to d_s_var / exp(s_var)), and dz4 [N][R][8] = grad_scale w d_rgb y (1 - y) in the rgb
    channels, 0 in the other five."""
    sdf = _d(sdf).clone().requires_grad_(True)
    grad = _d(grad).clone().requires_grad_(True)
    s_var = _d(s_var).reshape(-1)[:1].clone().requires_grad_(True)
    y, d_rgb = _d(y), _d(d_rgb)
    R = sdf.shape[1]
    inv_s = s_var.exp() * torch.ones(R, dtype=F64)
    inv_s.retain_grad()
    out = composite(dists, far, ray_unit, torch.ones(R), sdf, grad, y, None, anneal, white_bg, inv_s=inv_s)
    (out["rgb"] * d_rgb).sum().backward()
    w = out["weights"].detach()
    dz4 = torch.zeros(*y.shape[:2], 8, dtype=F64)
    dz4[..., :3] = grad_scale * w[..., None] * d_rgb[None] * (y[..., :3] * (1.0 - y[..., :3]))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # noqa: E731
    return dict(d_sdf=zero(sdf), d_grad=zero(grad), d_s_var=zero(s_var), d_inv_s=zero(inv_s), dz4=dz4,
                weights=w, alpha=out["alpha"].detach(), x=out["x"].detach(), cos=out["cos"].detach())


def composite_bwd(dists, far, ray_unit, sdf, grad, y, s_var, anneal, white_bg, d_rgb, d_o_r, d_o_s, d_o_re,
                  grad_scale):
    """mli_composite_bwd by float64 autograd through ``composite`` of
    sum(rgb d_rgb) + sum(o_r d_o_r) + sum(o_s d_o_s) + sum(o_re d_o_re) (None = that term is
    absent): dz4 [N][R][8] = grad_scale dL/dy y (1 - y) (the heads' sigmoids; channel 7 is 0) and
    dray [R][8], the gradient w.r.t. the composited (rgb, o_r, o_s) with the o_re chain folded
    in (channel 7 is 0)."""
    y = _d(y).clone().requires_grad_(True)
    R = y.shape[1]
    out = composite(dists, far, ray_unit, torch.ones(R), sdf, grad, y, s_var, anneal, white_bg)
    out["acc"].retain_grad()
    loss = torch.zeros((), dtype=F64)
    for key, g in (("rgb", d_rgb), ("o_r", d_o_r), ("o_s", d_o_s), ("o_re", d_o_re)):
        if g is not None:
            loss = loss + (out[key] * _d(g).reshape(out[key].shape)).sum()
    dz4 = torch.zeros(*y.shape[:2], 8, dtype=F64)
    dray = torch.zeros(R, 8, dtype=F64)
    if loss.requires_grad:
        loss.backward()
        yd = y.detach()
        dz4[..., :7] = grad_scale * y.grad[..., :7] * (yd[..., :7] * (1.0 - yd[..., :7]))
        dray[:, :7] = out["acc"].grad
    return dict(dz4=dz4, dray=dray)


# --------------------------------------------------------------------------- rays
def rays(intr, pose, pose_light, pix, width, bounding, aabb=None, radius=1.0):
    """camera.py:259-311 + nerf_util.py:199-205 / NeuralLumen/utils/utils.py:86-123: the pixel
    centre (x + 0.5, y + 0.5) of flat pixel y W + x through K^-1 and the inverted w2c pose
    [R^T | -R^T t], F.normalize, and the sphere (``bounding`` 'sphere') or slab ('box') bounds.
    ``margin`` is the quantity whose sign decides ``outside``: the sphere discriminant, or
    tmax - tmin of the box."""
    intr, pose, pose_light = _d(intr).reshape(3, 3), _d(pose).reshape(3, 4), _d(pose_light).reshape(3, 4)
    pix = torch.as_tensor(pix).to(torch.int64).reshape(-1)
    px = (pix % width).to(F64) + 0.5
    py = torch.div(pix, width, rounding_mode="floor").to(F64) + 0.5
    hom = torch.stack([px, py, torch.ones_like(px)], -1)
    cam = hom @ torch.linalg.inv(intr).t()
    rot_t, t = pose[:, :3].t(), pose[:, 3]
    c = -(rot_t @ t)
    ray = cam @ rot_t.t()                                              # world - center
    center = c[None].expand_as(ray)
    nrm = ray.norm(dim=-1)
    v = F.normalize(ray, dim=-1)
    light = (-(pose_light[:, :3].t() @ pose_light[:, 3]))[None].expand_as(ray)
    if bounding == "box":
        box = _d(aabb)
        t0, t1 = (box[:3] - center) / v, (box[3:] - center) / v
        tmin = torch.minimum(t0, t1).amax(-1).clamp(0, 1e10)
        tmax = torch.maximum(t0, t1).amin(-1).clamp(0, 1e10)
        margin = tmax - tmin
        outside = tmax <= tmin
        near, far = tmin, tmax
    else:
        ctc, ctv = (center * center).sum(-1), (center * v).sum(-1)
        margin = ctv ** 2 - (ctc - radius ** 2)
        outside = margin < 0
        sq = margin.clamp_min(0).sqrt()
        near, far = torch.relu(-ctv - sq), -ctv + sq
    near = torch.where(outside, torch.ones_like(near), near)
    far = torch.where(outside, torch.full_like(far, 1.2), far)
    return dict(center=center, ray_unit=v, ray_norm=nrm, pts_light=light, near=near, far=far, outside=outside,
                margin=margin)
