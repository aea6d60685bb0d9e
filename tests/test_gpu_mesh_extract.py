"""extract_mesh (mli_nerf_amd/mesh.py) on a synthetic stage-b model (log2T = 14, preset
syn_hotdog_b) against the CPU oracle: lattice SDF and sign-changing edges (oracle.render.sdf_net),
4-tap normals (sdf_taps) and the heads (rgb_heads), plus the properties of the stitched mesh:
independent of the block size, welded, closed, filtered, written by the command line.

The geometric init is a sphere of radius ~0.5 with hash-grid bumps: the 33^3 lattice over
[-1,1]^3 has ~1100 sign-changing edges and a positive boundary (checked on the CPU oracle), so the
surface is closed inside the lattice."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from margins import check
from mli_nerf_amd import synthetic
from mli_nerf_amd.configs import preset
from mli_nerf_amd.mesh import extract_mesh, lattice_axis
from oracle import render as o_render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG2T = 14
RES = 32          # 33^3 lattice, spacing 1/16
SDF_BAR = 2e-3    # tests/test_gpu_parity.py: sdf max abs
LIGHT = (1.5, -2.0, 2.5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _state_dict(heads="rgb_r_s", out_bias=0.5):
    return synthetic.make_state_dict(log2T=LOG2T, heads=heads, out_bias=out_bias)


def _model(config="syn_hotdog_b", **kw):
    from mli_nerf_amd.model import Model
    cfg = preset(config, log2T=LOG2T)
    model = Model(cfg.model, cfg.data)
    model.load_state_dict(_state_dict("rgb" if config.endswith("_a") else "rgb_r_s", **kw))
    return model.to(DEV)


@pytest.fixture(scope="module")
def model():
    return _model()


def _oracle_weights(**kw):
    sd = _state_dict(**kw)
    key = "neural_sdf.tcnn_encoding.params"
    sd[key] = sd[key].half().float()   # the kernels gather from the fp16 shadow of the table
    return sd


def _oracle_sdf(weights, pts, active=None):
    cfg = o_render.PathCfg(log2T=LOG2T, active_levels=active)
    with torch.no_grad():
        return o_render.sdf_net(weights, cfg, pts, False)[0][..., 0]


def _oracle_lattice(weights, active=None, lo=-1.0, hi=1.0):
    """The oracle's SDF on the lattice extract_mesh uses, its sign-changing edges {key: (|s0|, |s1|)}
    and the linear-interpolation vertex of each."""
    g = torch.from_numpy(lattice_axis(lo, hi, 2.0 / RES)).float()
    n = g.numel()
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1)
    s = _oracle_sdf(weights, pts, active).numpy()
    inside = s < 0
    edges, verts = {}, []
    for axis in range(3):
        lo_s = tuple(slice(0, -1) if d == axis else slice(None) for d in range(3))
        hi_s = tuple(slice(1, None) if d == axis else slice(None) for d in range(3))
        idx = np.argwhere(inside[lo_s] != inside[hi_s])
        for i, j, k in idx:
            q = [i, j, k]
            q[axis] += 1
            s0, s1 = float(s[i, j, k]), float(s[tuple(q)])
            edges[((i * n + j) * n + k) * 3 + axis] = (abs(s0), abs(s1))
            p = pts[i, j, k].clone()
            p[axis] += (0.0 - s0) / (s1 - s0) * (2.0 / RES)
            verts.append(p)
    return s, edges, torch.stack(verts)


@pytest.fixture(scope="module")
def oracle16():
    w = _oracle_weights()
    return (w,) + _oracle_lattice(w)


def _edge_rule(mesh, s, edges, what):
    """Every oracle edge with both end values above the SDF bar is in the GPU mesh; every GPU edge
    the oracle lacks has an end point with |oracle sdf| <= the bar."""
    got = set(mesh.keys.tolist())
    n = s.shape[0]
    missing = [k for k, (a, b) in edges.items() if min(a, b) > SDF_BAR and k not in got]
    assert not missing, (what, len(missing))
    extra = 0
    for k in got - set(edges):
        p, axis = divmod(k, 3)
        q = list(np.unravel_index(p, (n, n, n)))
        a = abs(float(s[tuple(q)]))
        q[axis] += 1
        assert min(a, abs(float(s[tuple(q)]))) <= SDF_BAR, (what, k)
        extra += 1
    return extra


def _closed_oriented(faces, n_verts):
    f = faces.cpu().numpy()
    pairs = ((0, 1), (1, 2), (2, 0))
    code = np.concatenate([f[:, a] * n_verts + f[:, b] for a, b in pairs])
    rev = np.concatenate([f[:, b] * n_verts + f[:, a] for a, b in pairs])
    uniq, counts = np.unique(code, return_counts=True)
    return counts.max() == 1 and np.array_equal(uniq, np.unique(rev))


@pytest.fixture(scope="module")
def mesh16(model):
    return extract_mesh(model, resolution=RES, block_res=16, attributes=("normal", "reflectance"), light=LIGHT,
                        sphere_filter=False)


def test_edge_set_and_surface_residual_against_oracle(mesh16, oracle16):
    weights, s, edges, v_oracle = oracle16
    assert len(edges) > 500
    extra = _edge_rule(mesh16, s, edges, "16 levels")
    print("oracle edges %d, GPU vertices %d, GPU-only edges %d" % (len(edges), mesh16.keys.numel(), extra))
    # surface residual: |oracle sdf| at the GPU vertices against the oracle's own interpolation
    # residual (the same linear interpolation on the oracle's lattice) + the SDF bar
    own = float(_oracle_sdf(weights, v_oracle).abs().max())
    got = float(_oracle_sdf(weights, mesh16.verts.cpu()).abs().max())
    # (the oracle's own residual has no bar of its own: a |grad| ~ 1 field cannot miss by a cell)
    check("mesh: oracle's own interpolation residual max |sdf(v_oracle)|", own, 2.0 / RES)
    check("mesh: surface residual max |oracle sdf(v_gpu)|", got, own + SDF_BAR,
          note="bar = oracle's own interpolation residual + the sdf bar %g" % SDF_BAR)


def test_block_size_does_not_change_the_mesh(model, mesh16):
    for block_res in (8, 32):
        m = extract_mesh(model, resolution=RES, block_res=block_res, attributes=(), sphere_filter=False)
        assert torch.equal(m.keys, mesh16.keys) and torch.equal(m.faces, mesh16.faces)
        assert torch.equal(m.face_keys, mesh16.face_keys)
        assert torch.equal(m.verts, mesh16.verts)


def test_welding(model, mesh16):
    loose = extract_mesh(model, resolution=RES, block_res=8, attributes=(), weld=False, sphere_filter=False)
    assert torch.unique(loose.keys).numel() < loose.keys.numel()       # block planes carry copies
    assert torch.unique(mesh16.keys).numel() == mesh16.keys.numel() == mesh16.verts.shape[0]
    assert torch.equal(torch.unique(loose.keys), mesh16.keys)
    assert int(mesh16.faces.min()) >= 0 and int(mesh16.faces.max()) < mesh16.verts.shape[0]
    assert loose.faces.shape == mesh16.faces.shape
    assert torch.equal(mesh16.keys, mesh16.keys.sort()[0]) and torch.equal(mesh16.face_keys, mesh16.face_keys.sort()[0])
    assert _closed_oriented(mesh16.faces, mesh16.verts.shape[0])       # closed, consistently oriented
    assert not _closed_oriented(loose.faces, loose.verts.shape[0])     # unwelded: open along the block planes


def test_sphere_filter():
    """Bounds widened to [-1.25, 1.25]^3.  The default field's surface stays inside the unit
    sphere; with the SDF bias at 1.0 it straddles it, so the filter has vertices to drop."""
    bounds = [[-1.25, 1.25]] * 3
    for out_bias, straddles in ((0.5, False), (1.0, True)):
        m = _model(out_bias=out_bias)
        full = extract_mesh(m, resolution=RES, block_res=16, bounds=bounds, attributes=(), sphere_filter=False)
        cut = extract_mesh(m, resolution=RES, block_res=16, bounds=bounds, attributes=("normal",))
        assert bool((full.verts.norm(dim=-1) >= 1).any()) == straddles
        assert cut.verts.shape[0] > 0 and float(cut.verts.norm(dim=-1).max()) < 1.0
        assert cut.faces.shape[0] > 0 and int(cut.faces.min()) >= 0 and int(cut.faces.max()) < cut.verts.shape[0]
        assert cut.normals.shape == cut.verts.shape
        # exactly the vertices inside the sphere and the faces that touch no dropped vertex
        keep = full.verts.norm(dim=-1) < 1
        assert torch.equal(cut.keys, full.keys[keep]) and torch.equal(cut.verts, full.verts[keep])
        fkeep = keep[full.faces].all(-1)
        assert torch.equal(cut.face_keys, full.face_keys[fkeep])
        assert torch.equal(cut.keys[cut.faces], full.keys[full.faces[fkeep]])


def test_normals_and_reflectance_against_oracle(mesh16, oracle16):
    weights = oracle16[0]
    cfg = o_render.PathCfg(log2T=LOG2T)
    v = mesh16.verts.cpu()
    with torch.no_grad():
        sdf, feat = o_render.sdf_net(weights, cfg, v, True)
        grad, _ = o_render.sdf_taps(weights, cfg, v, sdf, False)
        normal = torch.nn.functional.normalize(grad, dim=-1)
        light = torch.tensor(LIGHT).expand_as(v)
        _, o_r, _ = o_render.rgb_heads(weights, v, normal, -normal, feat, light)
    got = mesh16.normals.cpu()
    assert torch.allclose(got.norm(dim=-1), torch.ones(len(v)), atol=1e-5)
    angle = torch.rad2deg(torch.acos((got * normal).sum(-1).clamp(-1, 1)))
    check("mesh normals vs oracle 4-tap normals: p99 angle [deg]", float(torch.quantile(angle, 0.99)), 1.0, "<")
    refl = mesh16.colors["reflectance"].cpu()
    assert refl.shape == v.shape and mesh16.color is mesh16.colors["reflectance"]
    check("mesh reflectance vs oracle rgb_heads: max abs", float((refl - o_r).abs().max()), 5e-3, "<")


def test_colours_need_a_light_and_the_heads(model):
    with pytest.raises(ValueError, match="light"):
        extract_mesh(model, resolution=RES, attributes=("reflectance",))
    stage_a = _model("syn_hotdog_a")
    with pytest.raises(ValueError, match="stage a"):
        extract_mesh(stage_a, resolution=RES, attributes=("reflectance",), light=LIGHT)
    m = extract_mesh(stage_a, resolution=RES, block_res=32, attributes=("rgb",), light=LIGHT)
    assert m.colors["rgb"].shape == m.verts.shape and m.normals is None
    assert float(m.colors["rgb"].min()) >= 0 and float(m.colors["rgb"].max()) <= 1


def test_coarse_to_fine_levels(mesh16):
    """8 active levels (a stage-a checkpoint in mid coarse-to-fine): another surface, the oracle's
    with the same level mask."""
    m = _model()
    m.neural_sdf.active_levels = 8
    coarse = extract_mesh(m, resolution=RES, block_res=16, attributes=(), sphere_filter=False)
    assert m.engine.active_levels == 8
    assert not (coarse.verts.shape == mesh16.verts.shape and torch.equal(coarse.verts, mesh16.verts))
    s, edges, _ = _oracle_lattice(_oracle_weights(), active=8)
    _edge_rule(coarse, s, edges, "8 levels")


def _read_ply_counts(path):
    data = open(path, "rb").read()
    head = data[:data.index(b"end_header\n")].decode("ascii").split("\n")
    n = {l.split()[1]: int(l.split()[2]) for l in head if l.startswith("element")}
    props = [l.split()[2] for l in head if l.startswith("property") and "list" not in l]
    v = np.frombuffer(data, dtype=[(p, "u1" if p in ("red", "green", "blue") else "<f4") for p in props],
                      count=n["vertex"], offset=data.index(b"end_header\n") + 11)
    return n["vertex"], n["face"], props, v


def test_command_line_round_trip(model, tmp_path):
    from mli_nerf_amd.trainer import Trainer
    cfg = preset("syn_hotdog_b", log2T=LOG2T)
    tr = Trainer(cfg, is_inference=True, model=model)
    tr.current_epoch, tr.current_iteration = 0, 1000
    ckpt = tr.save_checkpoint(str(tmp_path), latest=True)
    out = str(tmp_path / "out" / "mesh.ply")
    cmd = [sys.executable, "-m", "mli_nerf_amd.mesh", "--config", "syn_hotdog_b", "--checkpoint", str(ckpt),
           "--resolution", str(RES), "--block_res", "16", "--output_file", out,
           "--attributes", "normal,reflectance", "--light", ",".join(str(x) for x in LIGHT),
           "--model.object.sdf.encoding.hashgrid.dict_size=%d" % LOG2T]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    want = extract_mesh(model, resolution=RES, block_res=16, attributes=("normal", "reflectance"), light=LIGHT)
    n_v, n_f, props, v = _read_ply_counts(out)
    assert (n_v, n_f) == (want.verts.shape[0], want.faces.shape[0])
    assert "vertices: %d" % n_v in res.stdout and "faces: %d" % n_f in res.stdout
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], -1), want.verts.cpu().numpy())
