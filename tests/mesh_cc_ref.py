"""The connected-component definitions of DESIGN.md §14.6 / include/mli_mesh_cc.h restated in
numpy / scipy (no GPU, nothing imported from the product): labels from
scipy.sparse.csgraph.connected_components mapped to the smallest index of each component, the
fixed-point face area q in float64, the per-component sums, the choice of the largest, and the
labelling round under the stalest reads a launch can give (every read taken from the round's start)."""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as _scipy_cc

PAIRS = ((0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0))   # (u, v): every pair, both directions


def labels(faces, n_verts):
    """[V] int32: the smallest vertex index of each vertex's component."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    cols = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    graph = coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(n_verts, n_verts))
    _, comp = _scipy_cc(graph, directed=False)
    smallest = np.full(comp.max() + 1, n_verts, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n_verts))
    return smallest[comp].astype(np.int32)


def area_unit(verts):
    """(e, unit, 1 / unit): unit = 2^(e-44), e = ceil(log2(d2)), d2 the squared diagonal of the
    bounding box in float64; (44, 1, 1) when d2 = 0."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    ext = v.max(0) - v.min(0)
    d2 = (ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2]
    if d2 == 0.0:
        return 44, 1.0, 1.0
    e = math.ceil(math.log2(d2))
    while 2.0 ** e < d2:        # log2's own rounding, both ways
        e += 1
    while 2.0 ** (e - 1) >= d2:
        e -= 1
    return e, 2.0 ** (e - 44), 2.0 ** (44 - e)


def face_q(verts, faces, inv_unit):
    """[F] int64: llrint(0.5 * sqrt(n2) * inv_unit), float64 from the fp32 coordinates."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    U, W = b - a, c - a
    cx = U[:, 1] * W[:, 2] - U[:, 2] * W[:, 1]
    cy = U[:, 2] * W[:, 0] - U[:, 0] * W[:, 2]
    cz = U[:, 0] * W[:, 1] - U[:, 1] * W[:, 0]
    n2 = (cx * cx + cy * cy) + cz * cz
    return np.rint(0.5 * np.sqrt(n2) * inv_unit).astype(np.int64)   # rint: to nearest even, as llrint


def component_stats(label, faces, q=None):
    """ids (labels owning >= 1 face, ascending), n_faces, area_q; a face counts for the component
    of its first vertex."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    owner = np.asarray(label, dtype=np.int64)[f[:, 0]]
    ids, inverse, counts = np.unique(owner, return_inverse=True, return_counts=True)
    area_q = np.zeros(ids.size, dtype=np.int64)
    if q is not None:
        np.add.at(area_q, inverse, np.asarray(q, dtype=np.int64))
    return ids, counts.astype(np.int64), area_q


def largest(ids, n_faces, area_q, by="area"):
    """Position of the largest component: greatest area_q, then most faces, then lowest label
    (by='faces': most faces, then lowest label)."""
    best = None
    for i in range(len(ids)):
        key = (-int(area_q[i]), -int(n_faces[i]), int(ids[i])) if by == "area" else (-int(n_faces[i]), int(ids[i]))
        if best is None or key < best[0]:
            best = (key, i)
    return best[1]


def keep_subset(label, faces, kept_ids):
    """(vertex mask, face mask) of the components in kept_ids."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vkeep = np.isin(np.asarray(label, dtype=np.int64), np.asarray(kept_ids, dtype=np.int64))
    return vkeep, vkeep[f[:, 0]]


def default_max_rounds(n_verts):
    return 2 * math.ceil(math.log2(max(n_verts, 2))) + 8


def stalest_round(label, faces):
    """One round in which every read sees the labels of the round's start and every write is a
    min into the live array.  Returns True when some word got lower."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    start = label.copy()
    jump = start[start]                       # label[label[.]] at the round's start
    for u, v in PAIRS:
        g = jump[f[:, v]]
        np.minimum.at(label, start[f[:, u]], g)
        np.minimum.at(label, f[:, u], g)
    np.minimum(label, jump, out=label)        # label[x] = min(label[x], label[label[x]])
    return bool((label < start).any())


def stalest_rounds(faces, n_verts, max_rounds=None):
    """(labels, rounds run, the confirming round included) of the stalest-read model."""
    label = np.arange(n_verts, dtype=np.int64)
    cap = default_max_rounds(n_verts) if max_rounds is None else max_rounds
    for r in range(cap):
        if not stalest_round(label, faces):
            return label.astype(np.int32), r + 1
    raise RuntimeError("no fixpoint after %d rounds" % cap)


def chain(numbering):
    """Faces (p_i, p_i+1, p_i+1) of the path p_0 - p_1 - ... under a vertex numbering."""
    p = np.asarray(numbering, dtype=np.int64)
    return np.stack([p[:-1], p[1:], p[1:]], 1)


def numberings(n, seed=0):
    """The four numberings of a path of n vertices: sequential, reversed, random, zigzag
    (0, n-1, 1, n-2, ...)."""
    seq = np.arange(n, dtype=np.int64)
    zig = np.empty(n, dtype=np.int64)
    zig[0::2] = seq[:(n + 1) // 2]
    zig[1::2] = seq[::-1][:n // 2]
    return {"sequential": seq, "reversed": seq[::-1].copy(),
            "random": np.random.default_rng(seed).permutation(n).astype(np.int64), "zigzag": zig}
