"""The numpy restatement of the connected-component definitions (tests/mesh_cc_ref.py) checked on
its own, no GPU: the labelling round under the stalest reads converges within log2 V + 4 rounds on
paths (the largest-diameter graphs there are), which is under the product's round cap, and the
labels, areas and choice rules hold on a hand-made mesh."""
import math

import numpy as np
import pytest
import torch

import mesh_cc_ref as R
from mli_nerf_amd import mesh

# two tetrahedra (vertices 1, 3, 4, 6 and 0, 2, 7, 8) and the unreferenced vertex 5
TET_A, TET_B = (1, 3, 4, 6), (0, 2, 7, 8)
VERTS = np.zeros((9, 3), dtype=np.float32)
VERTS[list(TET_A)] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
VERTS[list(TET_B)] = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]], dtype=np.float32) + 5
VERTS[5] = [9, 9, 9]


def _tet(v):
    a, b, c, d = v
    return [[a, c, b], [a, b, d], [a, d, c], [b, c, d]]


FACES = np.array(_tet(TET_A) + _tet(TET_B), dtype=np.int64)


@pytest.mark.parametrize("n", [4099, 65536])
def test_stalest_read_rounds_on_chains(n):
    bound = math.log2(n) + 4
    assert bound < R.default_max_rounds(n) == mesh.cc_max_rounds(n)
    for name, p in R.numberings(n).items():
        label, rounds = R.stalest_rounds(R.chain(p), n)
        assert not label.any(), name
        assert rounds <= bound, (name, rounds)


def test_round_cap_formula():
    for v, want in ((1, 10), (2, 10), (3, 12), (4, 12), (5, 14), (4099, 34), (65536, 40), (2 ** 20, 48),
                    (2 ** 31 - 1, 70)):
        assert mesh.cc_max_rounds(v) == want
        if v < 2 ** 22:
            assert R.default_max_rounds(v) == want


def test_two_tetrahedra_and_a_loose_vertex():
    label = R.labels(FACES, 9)
    assert label.dtype == np.int32 and label.tolist() == [0, 1, 0, 1, 1, 5, 1, 0, 0]
    model, rounds = R.stalest_rounds(FACES, 9)
    assert np.array_equal(model, label) and rounds <= R.default_max_rounds(9)
    e, unit, inv_unit = R.area_unit(VERTS)
    d2 = 3 * 9.0 ** 2   # the box from (0, 0, 0) to (9, 9, 9)
    assert 2.0 ** (e - 1) < d2 <= 2.0 ** e and unit * inv_unit == 1.0 and unit == 2.0 ** (e - 44)
    q = R.face_q(VERTS, FACES, inv_unit)
    assert q.dtype == np.int64 and int(q.max()) <= 2 ** 43
    # three right triangles of area 1/2 and the slanted one of sqrt(3)/2; the second is twice the size
    area = q * unit
    want = np.array([0.5, 0.5, 0.5, math.sqrt(3) / 2] * 2) * np.repeat([1.0, 4.0], 4)
    assert np.abs(area - want).max() <= unit
    ids, n_faces, area_q = R.component_stats(label, FACES, q)
    assert ids.tolist() == [0, 1] and n_faces.tolist() == [4, 4]      # vertex 5 owns no face: not listed
    assert area_q.tolist() == [int(q[4:].sum()), int(q[:4].sum())]
    assert R.largest(ids, n_faces, area_q, "area") == 0               # label 0: the large tetrahedron
    assert R.largest(ids, n_faces, area_q, "faces") == 0              # equal counts: the lower label
    assert R.largest(ids, n_faces, area_q[::-1].copy(), "area") == 1
    vkeep, fkeep = R.keep_subset(label, FACES, [1])
    assert np.flatnonzero(vkeep).tolist() == sorted(TET_A) and fkeep.tolist() == [True] * 4 + [False] * 4
    # the product's host-side choice states the same rule
    for by in ("area", "faces"):
        for aq in (area_q, area_q[::-1].copy(), np.array([7, 7])):
            assert mesh.largest_component(ids, n_faces, aq, by) == R.largest(ids, n_faces, aq, by)
    assert mesh.largest_component([3, 9, 4], [5, 6, 6], [8, 8, 8], "area") == 2
    assert mesh.largest_component([3, 9, 4], [5, 6, 6], [8, 1, 2], "faces") == 2


def test_degenerate_faces_have_no_area():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=np.float32)
    f = np.array([[0, 0, 1], [0, 1, 2], [0, 1, 3]], dtype=np.int64)   # a repeated vertex, three in a line
    q = R.face_q(v, f, R.area_unit(v)[2])
    assert q[0] == 0 and q[1] == 0 and q[2] > 0
    assert R.area_unit(np.ones((3, 3), dtype=np.float32)) == (44, 1.0, 1.0)


def test_area_unit_matches_the_product():
    rng = np.random.default_rng(3)
    for scale in (1e-3, 1.0, 2.0, 37.5, 1e6):
        v = (rng.random((50, 3)) * scale).astype(np.float32)
        _, unit, inv_unit = R.area_unit(v)
        assert mesh.area_unit(torch.from_numpy(v)) == (unit, inv_unit)
    box = np.array([[0, 0, 0], [2, 0, 0]], dtype=np.float32)           # d2 = 4 exactly: e = 2
    assert R.area_unit(box)[0] == 2 and mesh.area_unit(torch.from_numpy(box)) == (2.0 ** -42, 2.0 ** 42)
    assert mesh.area_unit(torch.ones(4, 3)) == (1.0, 1.0)
