"""The marching-cubes kernels (csrc/mesh.hip) through mesh.marching_cubes on synthetic lattices.

Every check is computed in numpy from the input lattice and does not read the case table (but for
the per-case triangle count): the vertex set is the set of sign-changing lattice edges, the
positions are the linear-interpolation formula of include/mli_mesh.h in fp32, and the triangles
form a closed, consistently oriented 2-manifold."""
import numpy as np
import pytest
import torch

from margins import check
from mli_nerf_amd import mc_tables
from mli_nerf_amd.mesh import marching_cubes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ragged: points no multiple of the wave (64) or the workgroup (256), each axis the shortest in
# turn; 96 x 96 x 64 = 2304 chunks: more than the grid cap (2048 workgroups, the grid-stride
# loop) and than the scan's 1024 threads (several chunks per thread)
SHAPES = [(9, 7, 5), (65, 17, 3), (33, 33, 33), (2, 64, 2), (96, 96, 64)]


def _lattice(shape, seed):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def _layouts(lat):
    """The same lattice as a contiguous [nx,ny,nz] tensor and in mli_sdf's output order
    [k][i*ny + j] (strides (ny, 1, nx*ny))."""
    t = torch.from_numpy(lat).to(DEV)
    return {"contiguous": t, "sdf_order": t.permute(2, 0, 1).contiguous().permute(1, 2, 0)}


def ref_vertices(lat, iso=0.0, origin=(0.0, 0.0, 0.0), spacing=1.0, offset=(0, 0, 0), gdims=None):
    """keys [V] int64 (ascending) and positions [V,3] fp32 of the sign-changing lattice edges."""
    gdims = lat.shape if gdims is None else gdims
    inside = lat < np.float32(iso)
    keys, pos = [], []
    o32, s32 = np.asarray(origin, np.float32), np.float32(spacing)
    for axis in range(3):
        lo = tuple(slice(0, -1) if d == axis else slice(None) for d in range(3))
        hi = tuple(slice(1, None) if d == axis else slice(None) for d in range(3))
        cross = inside[lo] != inside[hi]
        g = np.argwhere(cross).astype(np.int64) + np.asarray(offset, np.int64)
        s0, s1 = lat[lo][cross], lat[hi][cross]
        with np.errstate(all="ignore"):   # (NaN / inf lattices: the position is then NaN too)
            t = (np.float32(iso) - s0) / (s1 - s0)
        f = g.astype(np.float32)
        f[:, axis] = f[:, axis] + t
        keys.append(((g[:, 0] * gdims[1] + g[:, 1]) * gdims[2] + g[:, 2]) * 3 + axis)
        pos.append(o32 + f * s32)
    keys, pos = np.concatenate(keys), np.concatenate(pos)
    order = np.argsort(keys)
    return keys[order], pos[order]


def canonical(out):
    """(sorted vertex keys, positions in that order, per-face vertex KEYS sorted by face key, face keys)."""
    verts, faces, vkeys, fkeys = out
    vo, fo = torch.argsort(vkeys), torch.argsort(fkeys)
    return vkeys[vo], verts[vo], vkeys[faces[fo]], fkeys[fo]


def assert_closed_oriented(faces, n_verts):
    """Every undirected edge in exactly two faces, once in each direction."""
    f = faces.cpu().numpy()
    code = np.concatenate([f[:, a] * n_verts + f[:, b] for a, b in ((0, 1), (1, 2), (2, 0))])
    rev = np.concatenate([f[:, b] * n_verts + f[:, a] for a, b in ((0, 1), (1, 2), (2, 0))])
    uniq, counts = np.unique(code, return_counts=True)
    assert counts.max() == 1, "a directed edge is used %d times" % counts.max()
    assert np.array_equal(uniq, np.unique(rev)), "an edge without its opposite"
    return uniq.size // 2


def test_all_256_cases():
    rng = np.random.RandomState(7)
    for case in range(256):
        mag = rng.uniform(0.1, 1.0, 8).astype(np.float32)
        lat = np.empty((2, 2, 2), np.float32)
        for c in range(8):
            lat[c & 1, c >> 1 & 1, c >> 2 & 1] = -mag[c] if case >> c & 1 else mag[c]
        verts, faces, vkeys, fkeys = marching_cubes(torch.from_numpy(lat).to(DEV))
        keys, _ = ref_vertices(lat)
        assert verts.shape == (len(keys), 3) and np.array_equal(np.sort(vkeys.cpu().numpy()), keys), case
        assert faces.shape == (mc_tables.TRI_COUNT[case], 3), case
        assert fkeys.tolist() == list(range(faces.shape[0])), case   # cell 0, triangles 0..F-1
        if faces.numel():
            assert int(faces.min()) >= 0 and int(faces.max()) < verts.shape[0], case


@pytest.mark.parametrize("shape", SHAPES)
def test_vertex_set_positions_and_layouts(shape):
    lat = _lattice(shape, 11)
    origin, spacing, iso = (-1.0, 0.25, 3.0), 0.0625, 0.125
    outs = {name: marching_cubes(t, iso, origin, spacing) for name, t in _layouts(lat).items()}
    keys, pos = ref_vertices(lat, iso, origin, spacing)
    a, b = canonical(outs["contiguous"]), canonical(outs["sdf_order"])
    for x, y in zip(a, b):   # the two layouts: the same mesh, bit for bit, once sorted by key
        assert torch.equal(x, y)
    assert np.array_equal(a[0].cpu().numpy(), keys)          # exactly the sign-changing edges
    got = a[1].cpu().numpy()
    bound = 2.0 ** -20 * np.maximum(np.abs(pos), np.float32(spacing))
    ratio = float((np.abs(got - pos) / bound).max())
    check("marching cubes %s: max position error / (2^-20 max(|coord|, spacing))" % (shape,), ratio, 1.0)
    faces = outs["contiguous"][1]
    assert faces.dtype == torch.int64 and int(faces.min()) >= 0 and int(faces.max()) < len(keys)
    assert torch.unique(a[3]).numel() == a[3].numel()        # face keys are unique


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_closed_oriented_manifold_on_noise(seed):
    lat = _lattice((17, 13, 9), seed)
    lat[0] = lat[-1] = 1.0
    lat[:, 0] = lat[:, -1] = 1.0
    lat[:, :, 0] = lat[:, :, -1] = 1.0
    for t in _layouts(lat).values():
        verts, faces, vkeys, _ = marching_cubes(t)
        assert np.array_equal(np.sort(vkeys.cpu().numpy()), ref_vertices(lat)[0])
        assert_closed_oriented(faces, verts.shape[0])


def _analytic(kind, n=25):
    g = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    if kind == "sphere":
        lat = np.sqrt(x * x + y * y + z * z) - 0.6
    else:
        lat = np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z) - 0.25
    lat = lat.astype(np.float32)
    assert (lat != 0).all()   # no lattice point on the surface (radii chosen so)
    return lat, (-1.0, -1.0, -1.0), 2.0 / (n - 1)


@pytest.mark.parametrize("kind,euler", [("sphere", 2), ("torus", 0)])
def test_topology_and_orientation(kind, euler):
    lat, origin, spacing = _analytic(kind)
    verts, faces, _, _ = marching_cubes(torch.from_numpy(lat).to(DEV), 0.0, origin, spacing)
    n_edges = assert_closed_oriented(faces, verts.shape[0])
    assert verts.shape[0] - n_edges + faces.shape[0] == euler
    p = verts[faces].double()
    normal = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1)
    if kind == "sphere":   # outward: along the centroid
        assert float((normal * p.mean(1)).sum(-1).min()) > 0
    else:                  # outward: along the analytic SDF gradient at the centroid
        c = p.mean(1)
        ring = torch.nn.functional.normalize(c[:, :2], dim=-1) * 0.55
        grad = c - torch.cat([ring, torch.zeros_like(c[:, :1])], -1)
        assert float((normal * grad).sum(-1).min()) > 0


def test_blocks_share_keys_and_positions():
    """A lattice cut into two blocks that share a plane (offset / gdims): the union of the block
    meshes has the whole lattice's vertices (shared-plane copies bit-identical) and triangles."""
    lat = _lattice((21, 10, 12), 5)
    origin, spacing = (0.5, -2.0, 1.0), 0.03125
    t = torch.from_numpy(lat).to(DEV)
    whole = canonical(marching_cubes(t, 0.0, origin, spacing))
    parts = [marching_cubes(t[i0:i1 + 1], 0.0, origin, spacing, offset=(i0, 0, 0), gdims=lat.shape)
             for i0, i1 in ((0, 8), (8, 20))]
    vkeys = torch.cat([p[2] for p in parts])
    verts = torch.cat([p[0] for p in parts])
    order = torch.argsort(vkeys, stable=True)
    vkeys, verts = vkeys[order], verts[order]
    first = torch.ones_like(vkeys, dtype=torch.bool)
    first[1:] = vkeys[1:] != vkeys[:-1]
    assert (~first).any()                                          # the shared plane has edges
    assert torch.equal(verts[1:][~first[1:]], verts[:-1][~first[1:]])   # ... with identical copies
    assert torch.equal(vkeys[first], whole[0]) and torch.equal(verts[first], whole[1])
    fkeys = torch.cat([p[3] for p in parts])
    fverts = torch.cat([p[2][p[1]] for p in parts])
    fo = torch.argsort(fkeys)
    assert torch.equal(fkeys[fo], whole[3]) and torch.equal(fverts[fo], whole[2])


def test_bit_reproducible():
    t = torch.from_numpy(_lattice((33, 33, 33), 3)).to(DEV)
    a, b = marching_cubes(t), marching_cubes(t)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("value", [1.0, -1.0, float("nan")])
def test_no_surface(value):
    t = torch.full((9, 7, 5), value, device=DEV)
    verts, faces, vkeys, fkeys = marching_cubes(t)
    assert verts.shape == (0, 3) and verts.dtype == torch.float32
    assert faces.shape == (0, 3) and faces.dtype == torch.int64
    assert vkeys.shape == (0,) and vkeys.dtype == torch.int64 and fkeys.shape == (0,) and fkeys.dtype == torch.int64


def test_nan_inf_and_iso_values_count_as_outside():
    """Only s < iso classifies: NaN, +inf and s == iso are outside; the counts stay consistent
    (every face index < V) whatever the values."""
    lat = _lattice((12, 11, 10), 9)
    flat = lat.reshape(-1)
    flat[::7], flat[3::11], flat[5::13], flat[1::17] = np.nan, 0.0, np.inf, -np.inf
    verts, faces, vkeys, _ = marching_cubes(torch.from_numpy(lat).to(DEV))
    assert np.array_equal(np.sort(vkeys.cpu().numpy()), ref_vertices(lat)[0])
    assert faces.shape[0] > 0 and int(faces.min()) >= 0 and int(faces.max()) < verts.shape[0]
