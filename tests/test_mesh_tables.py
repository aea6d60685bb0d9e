"""The marching-cubes case table (mli_nerf_amd/mc_tables.py -> csrc/mc_table.h): the committed
header is what the generator writes, and every case is a valid oriented surface patch, checked in
pure Python from the header's own data (no GPU)."""
import itertools

import pytest

from mli_nerf_amd import mc_tables as T

TEXT = open(T.HEADER).read()
EDGE_CORNER, EDGE_AXIS, TRI_COUNT, TRI_EDGES = T.parse_header(TEXT)


def _corner(off):
    return off[0] | off[1] << 1 | off[2] << 2


def _ends(e):
    c = _corner(EDGE_CORNER[e])
    return c, c | 1 << EDGE_AXIS[e]


def _tris(case):
    row = TRI_EDGES[case]
    return [tuple(row[3 * t:3 * t + 3]) for t in range(TRI_COUNT[case])]


def _crossed(case):
    return {e for e in range(12) if (case >> _ends(e)[0] & 1) != (case >> _ends(e)[1] & 1)}


def _faces_of_edge(e):
    """The two cube faces (axis, side) an edge lies on."""
    a, b = _ends(e)
    return {(ax, a >> ax & 1) for ax in range(3) if (a >> ax & 1) == (b >> ax & 1)}


def _boundary(case):
    """Directed mesh edges used once; asserts no edge is used more than twice / twice one way."""
    use = {}
    for t in _tris(case):
        for u, v in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            use[(u, v)] = use.get((u, v), 0) + 1
    out = []
    for (u, v), n in use.items():
        assert n == 1, (case, u, v)
        if (v, u) not in use:
            out.append((u, v))
    return out


def test_header_is_what_the_generator_writes():
    assert T.render_header() == TEXT


def test_header_layout():
    assert len(TRI_COUNT) == 256 and len(TRI_EDGES) == 256 and max(TRI_COUNT) <= 5
    assert sorted(_ends(e) for e in range(12)) == sorted(
        (c, c | 1 << a) for a in range(3) for c in range(8) if not c >> a & 1)
    for case in range(256):
        used = 3 * TRI_COUNT[case]
        assert all(e < 12 for e in TRI_EDGES[case][:used]) and all(e == 255 for e in TRI_EDGES[case][used:])


@pytest.mark.parametrize("case", range(256))
def test_case_is_a_valid_patch(case):
    tris = _tris(case)
    # vertex set = the sign-changing cube edges; three distinct edges per triangle
    assert {e for t in tris for e in t} == _crossed(case)
    assert all(len(set(t)) == 3 for t in tris)
    # the once-used edges form closed loops (one in, one out per vertex) ...
    boundary = _boundary(case)
    nxt = dict(boundary)
    assert len(nxt) == len(boundary) and sorted(nxt) == sorted(nxt.values()) == sorted(_crossed(case))
    loops, seen = [], set()
    for start in nxt:
        if start in seen:
            continue
        n, e = 0, start
        while e not in seen:
            seen.add(e)
            e, n = nxt[e], n + 1
        assert e == start
        loops.append(n)
    # ... each segment on one cube face, and the triangle count is sum(loop length - 2)
    for u, v in boundary:
        assert _faces_of_edge(u) & _faces_of_edge(v), (case, u, v)
    assert TRI_COUNT[case] == sum(n - 2 for n in loops)
    # no interior (twice-used) edge lies in a cube face, where a neighbour could draw it too
    interior = {frozenset(p) for t in tris for p in itertools.combinations(t, 2)} - {frozenset(b) for b in boundary}
    for u, v in interior:
        assert not _faces_of_edge(u) & _faces_of_edge(v), (case, u, v)


def test_orientation_points_out_of_the_inside():
    """Each single-corner case: the triangle's normal (edge midpoints) points away from the inside
    corner; and the complement case has the opposite winding."""
    def mid(e):
        a, b = _ends(e)
        return [((a >> d & 1) + (b >> d & 1)) / 2 for d in range(3)]
    for c in range(8):
        (t,) = _tris(1 << c)
        p = [mid(e) for e in t]
        u = [p[1][d] - p[0][d] for d in range(3)]
        v = [p[2][d] - p[0][d] for d in range(3)]
        nrm = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
        away = [p[0][d] - (c >> d & 1) for d in range(3)]
        assert sum(nrm[d] * away[d] for d in range(3)) > 0, c
        (tc,) = _tris(255 ^ 1 << c)
        i = tc.index(t[0])
        assert (tc[i], tc[(i + 1) % 3], tc[(i + 2) % 3]) == (t[0], t[2], t[1])


def _face_segments(case, axis, side):
    """Undirected boundary segments of a case on one cube face, as pairs of (in-face position of
    the edge's lower corner, edge axis): comparable between the two cells that share the face."""
    segs = set()
    for u, v in _boundary(case):
        if (axis, side) in _faces_of_edge(u) & _faces_of_edge(v):
            def name(e):
                off = list(EDGE_CORNER[e])
                del off[axis]
                return tuple(off), EDGE_AXIS[e]
            segs.add(frozenset((name(u), name(v))))
    return segs


@pytest.mark.parametrize("axis", range(3))
def test_adjacent_cells_agree_on_the_shared_face(axis):
    """Cell A's +axis face is cell B's -axis face: for every pair of cases with the same four
    corner signs there, the segments on the face coincide."""
    lo = [c for c in range(8) if not c >> axis & 1]
    by_face = {}
    for case in range(256):
        for side in (0, 1):
            key = tuple(case >> (c | side << axis) & 1 for c in lo)
            by_face.setdefault((side, key), []).append(case)
    for key in itertools.product((0, 1), repeat=4):
        ref = None
        for side in (0, 1):
            for case in by_face[(side, key)]:
                segs = _face_segments(case, axis, side)
                ref = segs if ref is None else ref
                assert segs == ref, (axis, key, case, side)
