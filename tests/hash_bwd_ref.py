"""mli_hash_bwd (include/mli_hip.h) restated for the tests: the 5 points of a sample as
field_points5 builds them, the table gradient as a float64 scatter with its per-element error
budget, the d enc fragment image, and the ray builders of tests/test_gpu_hash_bwd.py.

The cell of a point is oracle/hashgrid.py's (``_encode_fwd``: pos = fmaf(scale, x, 0.5) rounded
once to fp32, g = floor(pos), frac = pos - g) and the rows are its ``_corner_index``;
tests/test_hash_bwd_ref.py ties both to ``_encode_fwd``'s own cache bit for bit.  No GPU, no
library."""
import numpy as np
import torch

from mli_nerf_amd import layout
from oracle import hashgrid as o_hash

TAPS = torch.tensor([[0, 0, 0], [1, -1, -1], [-1, -1, 1], [-1, 1, -1], [1, 1, 1]], dtype=torch.float32)


# ---------------------------------------------------------------------------- points and cells
def points5(center, ray_unit, dists, eps):
    """The 5 points of every sample in tile order (sample m = r N + k reads dists[k][r]), fp32 as
    field_points5: p0 = center + ray_unit * d with the product and the sum rounded separately,
    taps p0 + k_i eps.  center, ray_unit [R][3], dists [N][R] -> [5][S][3]."""
    N, R = dists.shape
    d = dists.to(torch.float32).t().reshape(-1)
    r_of = torch.arange(R * N) // N
    prod = ray_unit.to(torch.float32)[r_of] * d[:, None]
    p0 = center.to(torch.float32)[r_of] + prod
    e = torch.tensor(float(eps), dtype=torch.float32)
    return torch.stack([p0 if i == 0 else p0 + TAPS[i] * e for i in range(5)])


def x01_of(pts):
    """The encoder's input (p + 2) / 4 as the kernels compute it (fp32: an add, then a product)."""
    return (pts + 2.0) * 0.25


def cell_frac(x01, scale):
    """oracle/hashgrid.py's cell rule: integer cell (int64, negative below 0) and the fp32 frac."""
    pos = (x01.to(torch.float64) * float(scale) + 0.5).to(torch.float32)
    g = torch.floor(pos)
    return g.to(torch.int64), pos - g


def center_runs(cells, tile=32):
    """Runs of equal consecutive cells inside every ``tile`` samples (the lane half of a wave):
    cells [S][3] -> (tile, start lane, length) int64 arrays, one entry per run."""
    c = cells.reshape(-1, tile, 3)
    head = torch.ones(c.shape[:2], dtype=torch.bool)
    head[:, 1:] = (c[:, 1:] != c[:, :-1]).any(-1)
    t, s = torch.nonzero(head, as_tuple=True)
    nxt = torch.cat([s[1:], s.new_tensor([0])])
    last = torch.cat([t[1:] != t[:-1], t.new_tensor([True], dtype=torch.bool)])
    length = torch.where(last, tile - s, nxt - s)
    return t, s, length


# ---------------------------------------------------------------------------- the reference
def reference(pts, d_enc_pts, table, active_levels):
    """The table gradient of levels < active_levels in float64, over the touched rows only.

    pts [P][S][3] fp32 points, d_enc_pts [P][S][128] (level-major, 8 features per level).  Every
    corner of every point adds w * d enc, the 8 corner weights recomputed in float64 from the
    oracle's fp32 frac.  Returns rows [U] (table entries, sorted), and per element of those rows
    ([U][8]): g = sum w d, A = sum |w d|, n = how many of its contributions are nonzero."""
    bits = o_hash._CORNER_BITS
    rows_all, g_all, a_all, n_all = [], [], [], []
    for lvl, (scale, res, size, offset) in enumerate(table[:active_levels]):
        rows, vals = [], []
        for p in range(pts.shape[0]):
            gi, frac = cell_frac(x01_of(pts[p]), scale)
            gc = ((gi & o_hash.MASK32)[:, None, :] + bits[None]) & o_hash.MASK32
            rows.append(offset + o_hash._corner_index(gc[..., 0], gc[..., 1], gc[..., 2], res, size))
            fd = frac.to(torch.float64)
            w = torch.ones(fd.shape[0], 8, dtype=torch.float64)
            for d in range(3):
                w = w * torch.where(bits[None, :, d] == 1, fd[:, None, d], 1.0 - fd[:, None, d])
            vals.append(w[:, :, None] * d_enc_pts[p][:, None, lvl * 8:(lvl + 1) * 8].to(torch.float64))
        rows, vals = torch.cat(rows).reshape(-1), torch.cat(vals).reshape(-1, 8)
        # segment sums over the sorted rows (index_add_ crawls when thousands of contributions
        # share an element, as in crafted_runs)
        rows, order = torch.sort(rows)
        uniq, counts = torch.unique_consecutive(rows, return_counts=True)
        stacked = torch.cat([vals, vals.abs(), (vals != 0).to(torch.float64)], 1)[order]
        sums = torch.segment_reduce(stacked, "sum", lengths=counts, axis=0)
        rows_all.append(uniq)
        g_all.append(sums[:, :8])
        a_all.append(sums[:, 8:16])
        n_all.append(sums[:, 16:])
    return dict(rows=torch.cat(rows_all), g=torch.cat(g_all), A=torch.cat(a_all), n=torch.cat(n_all))


def tolerance(ref, deterministic=False):
    """The per-element bar.  A sum of n fp32 terms in any order is within (n - 1) 2^-24 A of the
    exact sum to first order, and each term carries at most 5 roundings (1 - frac, three weight
    products, the product with d enc): (n + 8) 2^-23 A is that bound with a factor of 2.  The fixed point of deterministic mode rounds each run total to 2^-40: n 2^-41
    more (include/mli_hip.h)."""
    tol = (ref["n"] + 8.0) * 2.0 ** -23 * ref["A"]
    return tol + ref["n"] * 2.0 ** -41 if deterministic else tol


# ---------------------------------------------------------------------------- the d enc image
def d_enc_col(S, p):
    """Column of point p of every sample in the [128][5 S] matrix whose NAT fragment image is
    mli_sdf_bwd's d enc ([S/32][5][8][64][8] fp32): tile 5 t + p of the 5 S columns."""
    m = torch.arange(S)
    return (m // 32 * 5 + p) * 32 + m % 32


def d_enc_image(mat):
    """[128][5 S] fp32 -> the d enc image mli_hash_bwd reads."""
    return layout.to_frag(mat, 8, "nat")


def d_enc_points(mat):
    """[128][5 S] -> [5][S][128], the operand of ``reference``."""
    S = mat.shape[1] // 5
    return torch.stack([mat[:, d_enc_col(S, p)].t() for p in range(5)])


# ---------------------------------------------------------------------------- ray builders
def _level0_x(j, u):
    """x of the point u cells above the centre of level-0 cell j (scale 31: the cell spans
    p in [4 (j - 0.5) / 31 - 2, 4 (j + 0.5) / 31 - 2))."""
    return 4.0 * (j + u) / 31.0 - 2.0


CRAFTED_R, CRAFTED_N = 528, 32


def crafted_pairs():
    """(start lane s, length n) of the crafted run of ray r: every 0 <= s < 32, 1 <= n <= 32 - s."""
    return [(s, n) for s in range(32) for n in range(1, 33 - s)]


def crafted_runs(variant, eps=float(np.float32(1.4e-4)), seed=0, spread=False):
    """528 rays x 32 samples, one tile per ray: ray (s, n) has lanes s .. s + n - 1 in level-0 cell
    16 and every other lane in cell 18 (odd lanes) or 20 (even lanes) -- singleton runs that share
    cells without being adjacent.  All rays start at (0, 0.013, -0.021) along +x, so a sample's
    depth is its x.  ``variant`` places x inside the cell: "center" mid-cell, "face" eps / 2 below
    the upper face (taps 1 and 4 leave the cell, 2 and 3 stay), "jitter" uniform over the middle
    96 % (seeded: finer levels split the same lanes into short runs).

    With all rays on one line every table element collects the contributions of all 528 (n up to
    30 000), and the bar, which grows with n, is then as wide as the sum of a few thousand of
    them.  ``spread`` moves ray r by whole level-0 cells to the (y, z) cell (4 + r % 24,
    4 + r // 24), the same place inside it: the runs are unchanged, an element collects a few
    rays at the most, and a single lost lane shows."""
    pairs = crafted_pairs()
    R, N = len(pairs), CRAFTED_N
    assert R == CRAFTED_R
    lane = torch.arange(N)
    cell = torch.where(lane % 2 == 1, 18, 20)[None].repeat(R, 1)
    for r, (s, n) in enumerate(pairs):
        cell[r, s:s + n] = 16
    cell = cell.to(torch.float64)
    if variant == "center":
        x = _level0_x(cell, 0.0)
    elif variant == "face":
        x = _level0_x(cell, 0.5) - 0.5 * float(eps)
    elif variant == "jitter":
        gen = torch.Generator().manual_seed(seed)
        x = _level0_x(cell, (torch.rand(R, N, generator=gen, dtype=torch.float64) - 0.5) * 0.96)
    else:
        raise ValueError(variant)
    center = torch.tensor([0.0, 0.013, -0.021], dtype=torch.float64).repeat(R, 1)
    if spread:
        r = torch.arange(R)
        center[:, 1] += 4.0 * (4 + r % 24 - 16) / 31.0
        center[:, 2] += 4.0 * (4 + r // 24 - 15) / 31.0
    center = center.to(torch.float32)
    ray_unit = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float32).repeat(R, 1)
    return dict(R=R, N=N, center=center, ray_unit=ray_unit, dists=x.t().contiguous().to(torch.float32))


IDLE_NEIGHBOUR_LANES = (5, 20)


def idle_neighbour_rays(eps=float(np.float32(1.4e-4))):
    """2 rays x 32 samples along +x, just outside the grid at y ~ -2 and z < -2.  In ray r, with
    l = IDLE_NEIGHBOUR_LANES[r], every sample sits mid-cell in level-0 cell (16, l, -1) except
    lane l - 1, which lies eps / 2 below the face between the x cells -2 and -1: its taps 1 and 4
    land in cell (-1, l, -1), and lane l, whose taps stay with its centre, has nothing to add to
    that tap's scatter.  A kernel that marks such idle lanes with a cell no point can have must
    not pick (-1, lane, -1) for it: that is this neighbour's cell."""
    R, N = len(IDLE_NEIGHBOUR_LANES), 32
    x = torch.full((R, N), _level0_x(16, 0.0), dtype=torch.float64)
    center = torch.zeros(R, 3, dtype=torch.float64)
    for r, l in enumerate(IDLE_NEIGHBOUR_LANES):
        x[r, l - 1] = _level0_x(-2, 0.5) - 0.5 * float(eps)
        center[r, 1], center[r, 2] = _level0_x(l, 0.0), _level0_x(-1, 0.0)
    ray_unit = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float32).repeat(R, 1)
    return dict(R=R, N=N, center=center.to(torch.float32), ray_unit=ray_unit,
                dists=x.t().contiguous().to(torch.float32))


OUT_OF_RANGE_SCALE = 5.0


def random_rays(R, N, seed, spread="in_range"):
    """Centres N(0, 0.3), random unit directions, depths uniform in [0, 2] sorted along each ray.
    spread="out_of_range" multiplies the centres by 5 (N(0, 1.5)): at least 5 % of the points
    then have some |p| coordinate in (2, 2.6), at least 5 % an x01 coordinate below 0 and at least
    5 % one above 1 (tests/test_hash_bwd_ref.py asserts the three shares; about 30 % each)."""
    gen = torch.Generator().manual_seed(seed)
    center = torch.randn(R, 3, generator=gen) * 0.3
    if spread == "out_of_range":
        center = center * OUT_OF_RANGE_SCALE
    elif spread != "in_range":
        raise ValueError(spread)
    v = torch.randn(R, 3, generator=gen)
    ray_unit = v / v.norm(dim=1, keepdim=True)
    dists = torch.sort(torch.rand(N, R, generator=gen) * 2.0, dim=0).values
    return dict(R=R, N=N, center=center, ray_unit=ray_unit, dists=dists.contiguous())


def random_d_enc(S, seed):
    """Seeded randn [128][5 S] fp32."""
    return torch.randn(128, 5 * S, generator=torch.Generator().manual_seed(seed))
