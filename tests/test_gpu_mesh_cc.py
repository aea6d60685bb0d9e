"""Connected components on the GPU (include/mli_mesh_cc.h, mesh.connected_components /
filter_components / extract_mesh(keep_lcc=True)) against the numpy / scipy restatement
tests/mesh_cc_ref.py: labels bit-equal, face counts equal, fixed-point areas within one unit per
face, the choice and tie rules, bit-reproducibility, the filter's subset and order, and the whole
path from a model to a PLY.

Measured on an MI355X (profiles/mesh/cc_margins.json): max per-face |q_gpu - q_numpy| = 0 units on
both numberings of the analytic lattice (bar 1); the 4099-vertex strip took 9 rounds (random
numbering) and 7 (sequential), against the stalest-read model's 13 and a cap of 34."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_cc_ref as R
from margins import check
from mli_nerf_amd import synthetic
from mli_nerf_amd.configs import preset
from mli_nerf_amd.mesh import (Mesh, cc_max_rounds, connected_components, extract_mesh, filter_components,
                               marching_cubes, vertex_attributes)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- case 1: the analytic lattice
# 33 x 29 x 31 points, spacing 1: a torus and five spheres of distinct radii, every pair >= 3
# cells apart (the closest: the torus and the r = 3.1 sphere, 3.26), all >= 1.2 inside the boundary
SHAPE = (33, 29, 31)
TORUS = ((9.3, 9.2, 5.1), 6.0, 2.0)
SPHERES = (((26.0, 7.0, 7.0), 4.7), ((26.5, 22.0, 6.5), 3.9), ((8.0, 23.5, 5.5), 3.1), ((8.5, 9.5, 21.5), 5.5),
           ((24.3, 20.4, 22.1), 3.3))   # 2290 vertices, 4560 faces


def _analytic_sdf():
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SHAPE], indexing="ij")
    (cx, cy, cz), big, small = TORUS
    s = np.sqrt((np.sqrt((x - cx) ** 2 + (y - cy) ** 2) - big) ** 2 + (z - cz) ** 2) - small
    for (cx, cy, cz), rad in SPHERES:
        s = np.minimum(s, np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - rad)
    return s.astype(np.float32)


class Case:
    """A mesh on the device with the restatement's answers next to it (computed once)."""

    def __init__(self, verts, faces, keys=None, face_keys=None):
        self.verts, self.faces, self.keys, self.face_keys = verts, faces, keys, face_keys
        self.v, self.f = verts.cpu().numpy(), faces.cpu().numpy()
        self.V = self.v.shape[0]
        self.label = R.labels(self.f, self.V)
        _, self.unit, self.inv_unit = R.area_unit(self.v)
        self.q = R.face_q(self.v, self.f, self.inv_unit)
        self.ids, self.n_faces, self.area_q = R.component_stats(self.label, self.f, self.q)


@pytest.fixture(scope="module")
def lattice():
    sdf = torch.from_numpy(_analytic_sdf()).to(DEV)
    verts, faces, keys, fkeys = marching_cubes(sdf)
    order_v, order_f = torch.argsort(keys), torch.argsort(fkeys)    # the canonical order extract_mesh gives
    inverse = torch.empty_like(order_v)
    inverse[order_v] = torch.arange(order_v.numel(), device=DEV)
    return Case(verts[order_v], inverse[faces[order_f]], keys[order_v], fkeys[order_f])


@pytest.fixture(scope="module")
def renumbered(lattice):
    g = torch.Generator().manual_seed(5)
    new_of_old = torch.randperm(lattice.V, generator=g).to(DEV)
    verts = torch.empty_like(lattice.verts)
    verts[new_of_old] = lattice.verts
    return Case(verts, new_of_old[lattice.faces])


def _per_face_q(case):
    """The GPU's q of every face: the faces pulled apart (three vertices of its own each, the same
    vertex set and so the same unit), every face a component."""
    F = case.f.shape[0]
    cc = connected_components(torch.arange(3 * F, device=DEV).view(F, 3), 3 * F, case.verts[case.faces].reshape(-1, 3))
    assert torch.equal(cc.ids, 3 * torch.arange(F, device=DEV)) and int(cc.n_faces.min()) == int(cc.n_faces.max()) == 1
    return cc.area_q.cpu().numpy()


def _against_restatement(case, what):
    cc = connected_components(case.faces, case.V, case.verts)
    assert cc.label.dtype == torch.int32 and torch.equal(cc.label.cpu(), torch.from_numpy(case.label))
    assert torch.equal(cc.ids.cpu(), torch.from_numpy(case.ids))
    assert torch.equal(cc.n_faces.cpu().long(), torch.from_numpy(case.n_faces))
    assert cc.rounds <= cc_max_rounds(case.V)
    dq = np.abs(_per_face_q(case) - case.q)
    # the bar is derived: q <= 2^43 carries 9 spare bits of the fp64 significand, so a sqrt within
    # 1 ulp moves it by far less than half a unit; only a rounding tie can flip it, by one
    check("mesh cc, %s: max per-face |q_gpu - q_numpy| [units]" % what, dq.max(), 1,
          note="expected 0 when the device's fp64 sqrt is correctly rounded")
    d_area = np.abs(cc.area_q.cpu().numpy() - case.area_q)
    assert (d_area <= case.n_faces).all()
    assert torch.equal(cc.area.cpu(), cc.area_q.cpu().double() * case.unit)
    return cc


def test_analytic_lattice(lattice):
    V, F = lattice.V, lattice.f.shape[0]
    assert V % 64 and F % 64 and F > 256
    assert lattice.ids.size == 6 and np.unique(lattice.label).size == 6    # preconditions (scipy)
    first, second = np.sort(lattice.area_q)[::-1][:2]
    assert first >= 1.01 * second
    _against_restatement(lattice, "analytic lattice")


def test_analytic_lattice_renumbered(lattice, renumbered):
    assert renumbered.ids.size == 6 and sorted(renumbered.n_faces) == sorted(lattice.n_faces)
    assert not np.array_equal(renumbered.label, lattice.label)
    _against_restatement(renumbered, "analytic lattice, random numbering")


# ---------------------------------------------------------------- case 2: the strip
@pytest.mark.parametrize("numbering", ["random", "sequential"])
def test_strip(numbering):
    n = 4099
    p = R.numberings(n, seed=1)[numbering]
    faces = torch.from_numpy(np.stack([p[:-2], p[1:-1], p[2:]], 1)).to(DEV)
    cc = connected_components(faces, n)
    assert cc.area is None and int(cc.area_q.sum()) == 0
    assert int(cc.label.max()) == 0 and cc.ids.tolist() == [0] and cc.n_faces.tolist() == [n - 2]
    model = R.stalest_rounds(faces.cpu().numpy(), n)[1]
    check("mesh cc, strip of 4099 vertices (%s): rounds" % numbering, cc.rounds, cc_max_rounds(n),
          note="the stalest-read model takes %d; the cap is 2*ceil(log2 V) + 8" % model)


# ---------------------------------------------------------------- case 3: ragged and degenerate
def _ragged_cases():
    rng = np.random.default_rng(11)
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 3, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]], dtype=np.float32)
    return {
        "F=1": (np.array([[2, 0, 1]]), rng.random((4, 3)).astype(np.float32)),
        "F=65, V=257": (rng.integers(0, 257, (65, 3)), rng.random((257, 3)).astype(np.float32)),
        "duplicate faces": (np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 4, 5]]), rng.random((6, 3)).astype(np.float32)),
        # (u, u, v), three points in a line, and a proper triangle apart from them
        "degenerate": (np.array([[3, 3, 0], [0, 1, 2], [4, 5, 6]]), line),
    }


@pytest.mark.parametrize("name", ["F=1", "F=65, V=257", "duplicate faces", "degenerate"])
def test_ragged_and_degenerate_inputs(name):
    f, v = _ragged_cases()[name]
    case = Case(torch.from_numpy(v).to(DEV), torch.from_numpy(f.astype(np.int64)).to(DEV))
    cc = connected_components(case.faces, case.V, case.verts)
    assert torch.equal(cc.label.cpu(), torch.from_numpy(case.label))
    assert torch.equal(cc.ids.cpu(), torch.from_numpy(case.ids))
    assert torch.equal(cc.n_faces.cpu().long(), torch.from_numpy(case.n_faces))
    assert (np.abs(cc.area_q.cpu().numpy() - case.area_q) <= case.n_faces).all()
    if name == "degenerate":
        assert case.q[:2].tolist() == [0, 0] and case.q[2] > 0
        assert cc.ids.tolist() == [0, 4] and cc.n_faces.tolist() == [2, 1]
        assert cc.area_q[0].item() == 0 and cc.area_q[1].item() > 0
        assert _per_face_q(case)[:2].tolist() == [0, 0]


def test_no_faces_launches_nothing():
    from mli_nerf_amd import _lib as L
    L.PROFILE, L.PROFILE_NAMES = [], None
    try:
        cc = connected_components(torch.empty(0, 3, dtype=torch.int64, device=DEV), 5, torch.rand(5, 3, device=DEV))
        assert L.PROFILE == []
    finally:
        L.PROFILE = L.PROFILE_NAMES = None
    assert cc.label.tolist() == [0, 1, 2, 3, 4] and cc.label.dtype == torch.int32
    assert cc.ids.numel() == cc.n_faces.numel() == cc.area.numel() == cc.area_q.numel() == 0 and cc.rounds == 0
    empty = filter_components(Mesh(torch.rand(5, 3, device=DEV), torch.empty(0, 3, dtype=torch.int64, device=DEV)))
    assert empty.verts.shape == (0, 3) and empty.faces.shape == (0, 3)


@pytest.mark.parametrize("bad", [8, -1, 2 ** 31])
def test_an_index_out_of_range_is_refused_before_any_launch(bad):
    from mli_nerf_amd import _lib as L
    faces = torch.tensor([[0, 1, 2], [3, bad, 4]], device=DEV)
    L.PROFILE, L.PROFILE_NAMES = [], None
    try:
        with pytest.raises(ValueError, match="outside"):
            connected_components(faces, 8, torch.rand(8, 3, device=DEV))
        assert L.PROFILE == []
    finally:
        L.PROFILE = L.PROFILE_NAMES = None
    with pytest.raises(ValueError):
        connected_components(faces[:1].to(torch.int32), 8)
    with pytest.raises(ValueError):
        connected_components(faces[:1], 0)


def test_round_cap_raises():
    n = 4099
    p = R.numberings(n, seed=1)["random"]
    faces = torch.from_numpy(np.stack([p[:-2], p[1:-1], p[2:]], 1)).to(DEV)
    with pytest.raises(RuntimeError, match="no fixpoint after 2 rounds"):
        connected_components(faces, n, max_rounds=2)


# ---------------------------------------------------------------- case 4: ties
def _two_octahedra():
    """Two copies of an octahedron with integer coordinates, the second moved by (10, 0, 0); the
    moved copy has the even vertex numbers (so label 0) and its faces come last."""
    corners = np.array([[2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2]], dtype=np.float32)
    tri = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    verts = np.zeros((12, 3), dtype=np.float32)
    verts[1::2] = corners
    verts[0::2] = corners + np.array([10, 0, 0], dtype=np.float32)
    faces = np.concatenate([2 * tri + 1, 2 * tri])
    return torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)


def test_ties_keep_the_lower_label():
    verts, faces = _two_octahedra()
    cc = connected_components(faces, 12, verts)
    assert cc.ids.tolist() == [0, 1] and cc.n_faces.tolist() == [8, 8]
    assert cc.area_q[0].item() == cc.area_q[1].item() > 0
    attr = torch.arange(12, device=DEV, dtype=torch.float32)[:, None].expand(12, 3)
    for by in ("area", "faces"):
        kept = filter_components(Mesh(verts, faces, normals=attr), keep="largest", by=by)
        assert torch.equal(kept.verts, verts[0::2]) and torch.equal(kept.normals, attr[0::2])
        assert torch.equal(kept.faces, faces[8:] // 2)
    # one more face on the odd copy's side (a duplicate): by area it wins, by faces too
    more = torch.cat([faces, faces[:1]])
    for by in ("area", "faces"):
        assert torch.equal(filter_components(Mesh(verts, more), by=by).verts, verts[1::2])
    with pytest.raises(ValueError):
        filter_components(Mesh(verts, faces), by="volume")
    with pytest.raises(ValueError):
        filter_components(Mesh(verts, faces), keep="smallest")


# ---------------------------------------------------------------- case 5: determinism
def test_runs_and_face_orders_give_the_same_bits(lattice):
    a = connected_components(lattice.faces, lattice.V, lattice.verts)
    b = connected_components(lattice.faces, lattice.V, lattice.verts)
    g = torch.Generator().manual_seed(9)
    shuffled = lattice.faces[torch.randperm(lattice.faces.shape[0], generator=g).to(DEV)]
    c = connected_components(shuffled, lattice.V, lattice.verts)
    for other in (b, c):
        assert torch.equal(a.label, other.label) and torch.equal(a.n_faces, other.n_faces)
        assert torch.equal(a.area_q, other.area_q) and torch.equal(a.ids, other.ids)


# ---------------------------------------------------------------- case 6: the filter
def _with_attributes(case):
    g = torch.Generator().manual_seed(2)
    return Mesh(case.verts, case.faces, normals=torch.rand(case.V, 3, generator=g).to(DEV),
                colors={"reflectance": torch.rand(case.V, 3, generator=g).to(DEV)}, keys=case.keys,
                face_keys=case.face_keys)


def _check_subset(case, full, kept, ids):
    vkeep, fkeep = R.keep_subset(case.label, case.f, ids)
    vk, fk = torch.from_numpy(vkeep).to(DEV), torch.from_numpy(fkeep).to(DEV)
    assert 0 < vkeep.sum() < case.V
    assert torch.equal(kept.verts, full.verts[vk]) and torch.equal(kept.keys, full.keys[vk])
    assert torch.equal(kept.face_keys, full.face_keys[fk])
    assert torch.equal(kept.keys[kept.faces], full.keys[full.faces[fk]])     # the same faces, re-indexed
    assert torch.equal(kept.normals, full.normals[vk])
    assert torch.equal(kept.colors["reflectance"], full.colors["reflectance"][vk])
    assert torch.equal(kept.keys, kept.keys.sort()[0]) and torch.equal(kept.face_keys, kept.face_keys.sort()[0])
    assert int(kept.faces.min()) >= 0 and int(kept.faces.max()) < kept.verts.shape[0]
    assert torch.unique(kept.faces).numel() == kept.verts.shape[0]             # no unreferenced vertex


def test_filter_keeps_the_restatements_subset(lattice):
    full = _with_attributes(lattice)
    best = lattice.ids[R.largest(lattice.ids, lattice.n_faces, lattice.area_q, "area")]
    _check_subset(lattice, full, filter_components(full, keep="largest"), [best])
    counts = np.sort(lattice.n_faces)
    assert counts[0] < counts[1]
    kept = filter_components(full, keep="all", min_faces=int(counts[0]) + 1)
    _check_subset(lattice, full, kept, lattice.ids[lattice.n_faces > counts[0]])
    assert kept.faces.shape[0] == lattice.f.shape[0] - counts[0]
    areas = np.sort(lattice.area_q * lattice.unit)
    kept = filter_components(full, keep="all", min_area=float(areas[-2] + areas[-1]) / 2)
    _check_subset(lattice, full, kept, [best])
    # the input is left as it was
    assert full.verts.shape[0] == lattice.V and torch.equal(full.faces, lattice.faces)


# ---------------------------------------------------------------- case 7: end to end
LOG2T = 14
RES = 32
LIGHT = (1.5, -2.0, 2.5)


@pytest.fixture(scope="module")
def model():
    from mli_nerf_amd.model import Model
    cfg = preset("syn_hotdog_b", log2T=LOG2T)
    m = Model(cfg.model, cfg.data)
    m.load_state_dict(synthetic.make_state_dict(log2T=LOG2T, heads="rgb_r_s", out_bias=0.5, enc_std=0.05))
    return m.to(DEV)


@pytest.fixture(scope="module")
def plain(model):
    return extract_mesh(model, resolution=RES, block_res=16, attributes=("normal",))


def test_extract_mesh_keep_lcc(model, plain):
    f = plain.faces.cpu().numpy()
    label = R.labels(f, plain.verts.shape[0])
    ids, n_faces, _ = R.component_stats(label, f)
    assert ids.size >= 2 and n_faces.max() >= 0.9 * f.shape[0]                 # preconditions (scipy)
    want = filter_components(plain, keep="largest")
    assert want.faces.shape[0] == n_faces.max() and want.verts.shape[0] < plain.verts.shape[0]
    want_normals = vertex_attributes(model, want.verts, ("normal",))["normal"]
    for block_res in (16, 8, 32):
        timings = {}
        got = extract_mesh(model, resolution=RES, block_res=block_res, attributes=("normal",), keep_lcc=True,
                           timings=timings)
        assert torch.equal(got.verts, want.verts) and torch.equal(got.faces, want.faces)
        assert torch.equal(got.keys, want.keys) and torch.equal(got.face_keys, want.face_keys)
        assert torch.equal(got.normals, want_normals)
        assert timings["components"] > 0
    # the size threshold alone: the single-cell blobs (8 faces each) go, the body stays
    small = extract_mesh(model, resolution=RES, block_res=16, attributes=(), min_component_faces=int(n_faces.max()))
    assert torch.equal(small.faces, want.faces) and torch.equal(small.keys, want.keys)


def test_defaults_do_what_they_did(model, plain):
    """No option given: the mesh before the filter, as the parent commit's extract_mesh built it
    (welded by key, faces by face key, the sphere filter) -- rebuilt here from the unwelded pieces."""
    timings = {}
    again = extract_mesh(model, resolution=RES, block_res=16, attributes=("normal",), keep_lcc=False,
                         min_component_faces=0, timings=timings)
    assert "components" not in timings
    for name in ("verts", "faces", "keys", "face_keys", "normals"):
        assert torch.equal(getattr(again, name), getattr(plain, name)), name
    loose = extract_mesh(model, resolution=RES, block_res=16, attributes=(), weld=False, sphere_filter=False)
    keys, inverse = torch.unique(loose.keys, sorted=True, return_inverse=True)
    verts = torch.empty(keys.numel(), 3, device=DEV)
    verts[inverse] = loose.verts                      # the copies of a vertex are bit-identical
    faces = inverse[loose.faces][torch.argsort(loose.face_keys)]
    assert float(verts.norm(dim=-1).max()) < 1.0      # nothing for the sphere filter to drop
    assert torch.equal(plain.keys, keys) and torch.equal(plain.verts, verts) and torch.equal(plain.faces, faces)


def test_unwelded_meshes_are_refused(model):
    for kw in (dict(keep_lcc=True), dict(min_component_faces=10)):
        with pytest.raises(ValueError, match="weld"):
            extract_mesh(model, resolution=RES, weld=False, **kw)


def _ply_counts(path):
    data = open(path, "rb").read()
    head = data[:data.index(b"end_header\n")].decode("ascii").split("\n")
    return {l.split()[1]: int(l.split()[2]) for l in head if l.startswith("element")}


def test_command_line_keep_lcc(model, plain, tmp_path):
    from mli_nerf_amd.trainer import Trainer
    cfg = preset("syn_hotdog_b", log2T=LOG2T)
    tr = Trainer(cfg, is_inference=True, model=model)
    tr.current_epoch, tr.current_iteration = 0, 1000
    ckpt = tr.save_checkpoint(str(tmp_path), latest=True)
    out = str(tmp_path / "lcc.ply")
    cmd = [sys.executable, "-m", "mli_nerf_amd.mesh", "--config", "syn_hotdog_b", "--checkpoint", str(ckpt),
           "--resolution", str(RES), "--block_res", "16", "--output_file", out, "--keep_lcc",
           "--model.object.sdf.encoding.hashgrid.dict_size=%d" % LOG2T]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    want = filter_components(plain, keep="largest")
    n = _ply_counts(out)
    assert (n["vertex"], n["face"]) == (want.verts.shape[0], want.faces.shape[0])
    assert n["face"] < plain.faces.shape[0] and "faces: %d" % n["face"] in res.stdout
