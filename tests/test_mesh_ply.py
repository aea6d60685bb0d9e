"""write_ply (mli_nerf_amd/mesh.py) against a small test-local PLY reader, no GPU."""
import numpy as np
import torch

from mli_nerf_amd.mesh import Mesh, write_ply


def read_ply(path):
    """Binary little-endian PLY with float / uchar vertex properties and uchar-int face lists."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    n_v = n_f = 0
    props, element = [], None
    for line in head[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            element = w[1]
            n_v, n_f = (int(w[2]), n_f) if element == "vertex" else (n_v, int(w[2]))
        elif w[:1] == ["property"] and element == "vertex":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        elif w[:1] == ["property"]:
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"]
    v = np.frombuffer(data, dtype=props, count=n_v, offset=end)
    f = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=n_f, offset=end + v.nbytes)
    assert end + v.nbytes + f.nbytes == len(data) and (f["n"] == 3).all()
    return v, f["i"]


def _mesh():
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.5, 0.125]])
    faces = torch.tensor([[0, 1, 2], [1, 3, 2]])
    normals = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.6, 0.0, 0.8]])
    colors = torch.tensor([[0.0, 0.5, 1.0], [1.2, -0.1, 0.25], [0.1, 0.2, 0.4], [0.999, 0.001, 0.498]])
    return verts, faces, normals, colors


def test_round_trip_with_normals_and_colours(tmp_path):
    verts, faces, normals, colors = _mesh()
    path = str(tmp_path / "m.ply")
    assert write_ply(path, Mesh(verts, faces, normals, {"reflectance": colors})) == (4, 2)
    v, f = read_ply(path)
    assert v.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], -1), verts.numpy())
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], -1), normals.numpy())
    want = np.array([[0, 128, 255], [255, 0, 64], [26, 51, 102], [255, 0, 127]], dtype=np.uint8)
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], -1), want)
    assert np.array_equal(f, faces.numpy())


def test_positions_only(tmp_path):
    verts, faces, _, _ = _mesh()
    path = str(tmp_path / "m.ply")
    write_ply(path, Mesh(verts, faces))
    v, f = read_ply(path)
    assert v.dtype.names == ("x", "y", "z") and len(v) == 4 and np.array_equal(f, faces.numpy())


def test_degenerate_face_is_dropped(tmp_path):
    verts, faces, normals, _ = _mesh()
    verts = torch.cat([verts, verts[1:2]])              # vertex 4 sits on vertex 1
    normals = torch.cat([normals, normals[1:2]])
    faces = torch.cat([faces, torch.tensor([[1, 4, 2], [0, 0, 3]])])   # equal positions; equal indices
    path = str(tmp_path / "m.ply")
    assert write_ply(path, Mesh(verts, faces, normals)) == (5, 2)
    v, f = read_ply(path)
    assert len(v) == 5 and np.array_equal(f, faces[:2].numpy())


def test_empty_mesh(tmp_path):
    path = str(tmp_path / "m.ply")
    assert write_ply(path, Mesh(torch.empty(0, 3), torch.empty(0, 3, dtype=torch.int64))) == (0, 0)
    v, f = read_ply(path)
    assert len(v) == 0 and f.shape == (0, 3)
