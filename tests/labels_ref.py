"""The pseudo-label definitions of DESIGN.md §15 / include/mli_labels.h restated in numpy: the
test reference of the GPU kernels (not a test, and never imported by the product).  fp32 op by op
in the stated order; only the fill's distance D is taken in float64 from the fp32 features."""
import numpy as np

F = np.float32
SQRT2, SQRT6 = F(np.sqrt(2.0)), F(np.sqrt(6.0))


# ---------------------------------------------------------------------------- morphology
def _window_has_both(v, r):
    """[H,W] bool: the (2r+1)^2 window with clamped indices holds a 0 and a 1."""
    H, W = v.shape
    ys = np.clip(np.arange(H)[:, None] + np.arange(-r, r + 1)[None, :], 0, H - 1)   # [H, 2r+1]
    xs = np.clip(np.arange(W)[:, None] + np.arange(-r, r + 1)[None, :], 0, W - 1)
    win = v[ys[:, None, :, None], xs[None, :, None, :]]                             # [H,W,2r+1,2r+1]
    return win.min(axis=(2, 3)) != win.max(axis=(2, 3))


def nearest_other(v, radius):
    """d(p): the smallest r in 1..radius whose clamped window holds both values, radius + 1 if none."""
    v = np.asarray(v) != 0
    d = np.full(v.shape, radius + 1, dtype=np.int32)
    for r in range(radius, 0, -1):
        d[_window_has_both(v, r)] = r
    return d


def erode(v, kernel_size):
    """[..., H, W] binary -> fp32 0/1: all of the kernel_size^2 clamped window is 1."""
    v = np.asarray(v)
    out = np.empty(v.shape, dtype=F)
    flat, oflat = v.reshape((-1,) + v.shape[-2:]), out.reshape((-1,) + v.shape[-2:])
    for i in range(flat.shape[0]):
        oflat[i] = ((flat[i] != 0) & (nearest_other(flat[i], kernel_size // 2) > kernel_size // 2)).astype(F)
    return out


def edge_count(v, step):
    d = nearest_other(v, step)
    return np.maximum(0, step - d + 1).astype(np.int32)


def certainty(v, step):
    v = np.asarray(v)
    out = np.empty(v.shape, dtype=F)
    flat, oflat = v.reshape((-1,) + v.shape[-2:]), out.reshape((-1,) + v.shape[-2:])
    for i in range(flat.shape[0]):
        c = edge_count(flat[i], step).astype(F)
        m = c.max()
        oflat[i] = F(1) - c / m if m > 0 else F(1)
    return out


def shading(normal_x_light, eroded, inter_mask=None, gamma=2.2):
    ps = np.asarray(normal_x_light, dtype=F) * np.asarray(eroded, dtype=F)
    if inter_mask is not None:
        ps = ps * np.asarray(inter_mask, dtype=F)
    return ps, np.power(ps, F(1.0 / gamma)).astype(F)


# ---------------------------------------------------------------------------- k-means along pixels
def opponent(image):
    """[L,3,N] fp32 -> [L,2,N]."""
    r, g, b = image[:, 0], image[:, 1], image[:, 2]
    return np.stack([(r - g) / SQRT2, ((r + g) - F(2) * b) / SQRT6], axis=1).astype(F)


def _d2(x, c):
    """x [L,2,N], c [2,N] -> [L,N], dx*dx + dy*dy from direct differences."""
    dx, dy = x[:, 0] - c[None, 0], x[:, 1] - c[None, 1]
    return dx * dx + dy * dy


def _assign(x, cen):
    d = np.stack([_d2(x, c) for c in cen])      # [K,L,N]
    return np.argmin(d, axis=0).astype(np.uint8)  # first minimum: lowest cluster on ties


def kmeans_init(x, K):
    cen = [x[0].copy()]
    n = np.arange(x.shape[2])
    for j in range(1, K):
        m = _d2(x, cen[0])
        for c in cen[1:]:
            m = np.minimum(m, _d2(x, c))
        pick = np.argmax(m, axis=0)             # first maximum: lowest l on ties
        cen.append(x[pick, :, n].T.copy())
    return np.stack(cen)                        # [K,2,N]


def kmeans(image, K, max_iter=100):
    """image [L,3,N] fp32 -> labels [L,N] uint8, centres [K,2,N] fp32, passes [N] int32,
    initial labels [L,N] (the first assignment, for the inertia property)."""
    image = np.asarray(image, dtype=F)
    x = opponent(image)
    Ln, _, N = x.shape
    cen = kmeans_init(x, K)
    labels = np.zeros((Ln, N), dtype=np.uint8)
    passes = np.zeros(N, dtype=np.int32)
    active = np.ones(N, dtype=bool)
    first = None
    for it in range(max_iter):
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        xa = x[:, :, idx]
        new = _assign(xa, cen[:, :, idx])
        changed = np.ones(idx.size, dtype=bool) if it == 0 else (new != labels[:, idx]).any(axis=0)
        labels[:, idx] = new
        if it == 0:
            first = labels.copy()
        passes[idx] += 1
        active[idx[~changed]] = False
        upd = idx[changed]
        xu, lu = x[:, :, upd], labels[:, upd]
        for j in range(K):
            sx = np.zeros(upd.size, dtype=F)
            sy = np.zeros(upd.size, dtype=F)
            cnt = np.zeros(upd.size, dtype=np.int32)
            for l in range(Ln):                 # ascending l
                m = lu[l] == j
                sx = np.where(m, sx + xu[l, 0], sx)
                sy = np.where(m, sy + xu[l, 1], sy)
                cnt += m
            has = cnt > 0
            den = np.maximum(cnt, 1).astype(F)
            cen[j, 0, upd] = np.where(has, sx / den, cen[j, 0, upd])
            cen[j, 1, upd] = np.where(has, sy / den, cen[j, 1, upd])
    return labels, cen, passes, first


# ---------------------------------------------------------------------------- best reflectance
def best_ref(image, ps, psg, labels, K, threshold=0.0, wrt_max=0.6):
    """image [L,3,N], ps / psg [L,N], labels [L,N] -> average_ref [3,N] fp32, keep [N] int32,
    any_mask [N] bool, keep mask [L,N]."""
    image, ps, psg = (np.asarray(t, dtype=F) for t in (image, ps, psg))
    Ln, N = ps.shape
    mask = ps > F(threshold)
    lab = np.where(mask, labels, K)
    counts = np.stack([(lab == j).sum(axis=0) for j in range(K)])          # [K,N]
    winners = counts == counts.max(axis=0, keepdims=True)
    winners = np.concatenate([winners, np.zeros((1, N), dtype=bool)])
    g = np.take_along_axis(winners, lab.astype(np.int64), axis=0)          # [L,N]
    smax = (ps * g.astype(F)).max(axis=0)
    keep = g & (ps > F(wrt_max) * smax[None])
    out = np.zeros((3, N), dtype=F)
    for l in range(Ln):                                                    # ascending l
        k = keep[l]
        for c in range(3):
            q = np.divide(image[l, c], psg[l], out=np.zeros(N, dtype=F), where=k)
            out[c] = np.where(k, out[c] + q, out[c])
    n_keep = keep.sum(axis=0).astype(np.int32)
    out = out / np.maximum(n_keep, 1).astype(F)[None]
    return out.astype(F), n_keep, mask.any(axis=0), keep


# ---------------------------------------------------------------------------- nearest-donor fill
def features(normal, centers, H, W):
    """normal [3,N], centers [K,2,N] -> base [5,N] fp32, colour [K,2,N] fp32."""
    normal = np.asarray(normal, dtype=F)
    p = np.arange(H * W)
    den = F(max(H - 1, W - 1, 1))
    y, x = (p // W).astype(F), (p % W).astype(F)
    norm = np.sqrt((normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2]) + F(1e-10)
    base = np.stack([y / den * F(4), x / den * F(4), normal[0] / norm, normal[1] / norm, normal[2] / norm])
    return base.astype(F), np.asarray(centers, dtype=F)


def distances(base, colour, holes, donors):
    """D in float64 from the fp32 features: [n_holes, n_donors]."""
    b, c = base.astype(np.float64), colour.astype(np.float64)
    D = ((b[:, holes, None] - b[:, None, donors]) ** 2).sum(axis=0)
    K = c.shape[0]
    cmin = None
    for i in range(K):
        for j in range(K):
            e = ((c[i][:, holes, None] - c[j][:, None, donors]) ** 2).sum(axis=0)
            cmin = e if cmin is None else np.minimum(cmin, e)
    return D + cmin


def fill(ref, normal, centers, donor_mask):
    """ref [3,H,W] -> filled copy, plus (holes, donors, D) for the tolerance checks."""
    ref = np.asarray(ref, dtype=F)
    _, H, W = ref.shape
    donor = np.asarray(donor_mask).reshape(-1) != 0
    holes, donors = np.nonzero(~donor)[0], np.nonzero(donor)[0]
    out = ref.reshape(3, -1).copy()
    if holes.size == 0 or donors.size == 0:
        return out.reshape(ref.shape), holes, donors, None
    base, colour = features(np.asarray(normal, dtype=F).reshape(3, -1), np.asarray(centers, dtype=F).reshape(
        centers.shape[0], 2, -1), H, W)
    D = distances(base, colour, holes, donors)
    out[:, holes] = out[:, donors[np.argmin(D, axis=1)]]
    return out.reshape(ref.shape), holes, donors, D
