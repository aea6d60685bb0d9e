"""tests/hash_bwd_ref.py: the reference of mli_hash_bwd against oracle/hashgrid.py, and the
properties of the crafted and random inputs that tests/test_gpu_hash_bwd.py relies on (dense and
hashed levels at log2T = 18, every run length and every cross-row start, off-cell taps,
out-of-range points).  None of these measures the kernel.  No GPU, no library."""
import numpy as np
import pytest
import torch

import hash_bwd_ref as H
from oracle import hashgrid as o_hash

EPS_FINE = float(np.float32(1.4e-4))
EPS_COARSE = 0.02


@pytest.fixture(scope="module")
def table18():
    return o_hash.level_table(log2T=18)


def _cells(pts, table, lvl):
    """[P][S][3] cells of every point at one level."""
    return torch.stack([H.cell_frac(H.x01_of(p), table[lvl][0])[0] for p in pts])


def test_level_table_log2T18_is_dense_then_hashed(table18):
    table, total = table18
    dense = [res ** 3 <= size for _, res, size, _ in table]
    assert dense == [True] * 3 + [False] * 13
    # dense levels 1 and 2 are no powers of two (fastmod indexing), the hashed ones are 2^18 (mask)
    assert all(size & (size - 1) for _, _, size, _ in table[1:3])
    assert all(size == 1 << 18 for _, _, size, _ in table[3:])
    # the kernel's table (engine._grid_levels) is the oracle's
    from mli_nerf_amd import engine
    g, g_total = engine._grid_levels(engine.PathConfig(log2T=18))
    assert g_total == total
    for i, (scale, res, size, off) in enumerate(table):
        assert (g.scale[i], g.res[i], g.size[i], g.offset[i]) == (np.float32(scale), res, size, off)
        assert all((n * g.modmagic[i] & (2 ** 64 - 1)) * size >> 64 == n % size
                   for n in (0, 1, size - 1, size, size + 1, 2 ** 32 - 1, 2 ** 32 - res))
    # all hashed at 2^14 (the configuration of the Trainer-level decomposition test)
    assert not any(res ** 3 <= size for _, res, size, _ in o_hash.level_table(log2T=14)[0])


def test_cells_and_rows_are_the_oracles(table18):
    """cell_frac / reference restate two lines of _encode_fwd: its cached rows and fp32 weights
    come out bit for bit (out-of-range points included)."""
    table, total = table18
    rays = H.random_rays(6, 32, seed=3, spread="out_of_range")
    pts = H.points5(rays["center"], rays["ray_unit"], rays["dists"], EPS_COARSE)
    x01 = H.x01_of(pts[1])
    _, cache = o_hash._encode_fwd(x01, torch.zeros(total * 8), table, 8)
    bits = o_hash._CORNER_BITS
    for (scale, res, size, offset), (rows, ws) in zip(table, cache):
        gi, frac = H.cell_frac(x01, scale)
        gc = ((gi & o_hash.MASK32)[:, None, :] + bits[None]) & o_hash.MASK32
        assert torch.equal(rows, offset + o_hash._corner_index(gc[..., 0], gc[..., 1], gc[..., 2], res, size))
        for c in range(8):
            w = torch.ones(frac.shape[0])
            for d in range(3):
                w = w * (frac[:, d] if (c >> d) & 1 else (1.0 - frac[:, d]))
            assert torch.equal(w, ws[c])


def test_reference_equals_the_oracle_backward(table18):
    table, total = table18
    rays = H.random_rays(6, 32, seed=1)
    S = 6 * 32
    pts = H.points5(rays["center"], rays["ray_unit"], rays["dists"], EPS_FINE)[:1]
    d = torch.randn(S, 128, generator=torch.Generator().manual_seed(2))
    params = torch.zeros(total * 8, requires_grad=True)
    o_hash.encode(H.x01_of(pts[0]), params, table).backward(d)
    dense = params.grad.view(-1, 8)
    ref = H.reference(pts, d[None], table, 16)
    err = (dense[ref["rows"]].double() - ref["g"]).abs()
    assert (err <= H.tolerance(ref)).all(), float((err / H.tolerance(ref).clamp_min(1e-300)).max())
    assert (ref["A"] > 0).any(1).all() and int((ref["n"] > 1).sum()) > 0
    # support: nothing outside the touched rows
    assert int(torch.count_nonzero(dense)) == int(torch.count_nonzero(dense[ref["rows"]]))
    # fewer active levels: the same rows and sums, cut at the level's offset
    ref1 = H.reference(pts, d[None], table, 1)
    k = ref1["rows"].numel()
    assert k < ref["rows"].numel() and int(ref1["rows"].max()) < table[1][3]
    assert torch.equal(ref1["rows"], ref["rows"][:k]) and torch.equal(ref1["g"], ref["g"][:k])


def test_d_enc_image_layout():
    """Element j of lane c + 32 h of k-step q of tile 5 t + p is feature 16 q + 8 h + j (level
    2 q + h, feature j) of point p of sample 32 t + c."""
    S = 64
    mat = H.random_d_enc(S, 0)
    img = H.d_enc_image(mat).view(S // 32, 5, 8, 2, 32, 8)
    pts = H.d_enc_points(mat)
    assert pts.shape == (5, S, 128)
    for t, p, q, h, c, j in [(0, 0, 0, 0, 0, 0), (1, 4, 7, 1, 31, 7), (1, 2, 3, 0, 17, 5), (0, 3, 6, 1, 2, 1)]:
        assert img[t, p, q, h, c, j] == pts[p, 32 * t + c, 16 * q + 8 * h + j]


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("variant", ["center", "face", "jitter"])
def test_crafted_runs(table18, variant, spread):
    table, _ = table18
    rays = H.crafted_runs(variant, EPS_FINE, spread=spread)
    assert (rays["R"], rays["N"]) == (528, 32)
    pts = H.points5(rays["center"], rays["ray_unit"], rays["dists"], EPS_FINE)
    cells = _cells(pts, table, 0)
    # one (y, z) cell per ray: (16, 15) for all of them, or every ray its own
    yz = cells[0].reshape(528, 32, 3)[:, :, 1:]
    assert (yz == yz[:, :1]).all()
    assert len(set(map(tuple, yz[:, 0].tolist()))) == (528 if spread else 1)
    assert yz[0, 0].tolist() == ([4, 4] if spread else [16, 15])
    assert int(yz.min()) >= 4 and int(yz.max()) <= 27
    t, s, n = H.center_runs(cells[0])
    # the crafted run of ray (s, n) is there, in cell j = 16 along x
    runs = set(zip(t.tolist(), s.tolist(), n.tolist()))
    for r, (s0, n0) in enumerate(H.crafted_pairs()):
        assert (r, s0, n0) in runs
        assert (cells[0][r * 32 + s0:r * 32 + s0 + n0, 0] == 16).all()
    assert set(n.tolist()) == set(range(1, 33))
    crossing = (s <= 15) & (s + n - 1 >= 16)
    assert set(s[crossing].tolist()) == set(range(16))
    # the other lanes: cells 18 / 20, shared between lanes that are never adjacent
    other = cells[0][:, 0] != 16
    assert set(cells[0][other, 0].tolist()) == {18, 20}
    off = (cells[1:] != cells[:1]).any(-1).double().mean(1)   # per tap: share outside the centre's cell
    if variant == "face":
        assert off.tolist() == [1.0, 0.0, 0.0, 1.0]
    if variant == "center":
        assert off.tolist() == [0.0] * 4
    if variant == "jitter":
        longest = int(H.center_runs(_cells(pts[:1], table, 15)[0])[2].max())
        print("longest level-15 run", longest)
        assert longest <= 4


def test_random_rays_leave_the_centre_cell(table18):
    table, _ = table18
    rays = H.random_rays(16, 32, seed=0)
    assert (rays["dists"][1:] >= rays["dists"][:-1]).all()
    assert torch.allclose(rays["ray_unit"].norm(dim=1), torch.ones(16))

    def share(eps, lvl):
        cells = _cells(H.points5(rays["center"], rays["ray_unit"], rays["dists"], eps), table, lvl)
        return float((cells[1:] != cells[:1]).any(-1).double().mean())

    s0, s5, s15 = share(EPS_COARSE, 0), share(EPS_COARSE, 5), share(EPS_FINE, 15)
    print("off-cell share: level 0 %.3f, level 5 %.3f at eps 0.02; level 15 %.3f at eps 1.4e-4" % (s0, s5, s15))
    assert s0 >= 0.3 and s5 >= 0.9 and s15 > 0.0


def test_idle_neighbour_rays(table18):
    table, _ = table18
    rays = H.idle_neighbour_rays(EPS_FINE)
    cells = _cells(H.points5(rays["center"], rays["ray_unit"], rays["dists"], EPS_FINE), table, 0)
    for r, l in enumerate(H.IDLE_NEIGHBOUR_LANES):
        m = 32 * r + l
        assert cells[0][m - 1].tolist() == [-2, l, -1]
        for tap in (1, 4):       # leaves for the cell that reads (-1, lane l, -1)
            assert cells[tap][m - 1].tolist() == [-1, l, -1]
        for tap in (2, 3):
            assert cells[tap][m - 1].tolist() == [-2, l, -1]
        assert (cells[:, m] == cells[0, m]).all() and cells[0, m].tolist() == [16, l, -1]


def test_out_of_range_rays():
    rays = H.random_rays(6, 32, seed=0, spread="out_of_range")
    x01 = H.x01_of(H.points5(rays["center"], rays["ray_unit"], rays["dists"], EPS_COARSE)[0])
    neg, above = float((x01 < 0).any(1).double().mean()), float((x01 > 1).any(1).double().mean())
    p = (x01 * 4 - 2).abs()
    near = float(((p > 2) & (p < 2.6)).any(1).double().mean())
    print("out_of_range: x01 < 0 %.3f, x01 > 1 %.3f, some |p| in (2, 2.6) %.3f" % (neg, above, near))
    assert neg >= 0.05 and above >= 0.05 and near >= 0.05
