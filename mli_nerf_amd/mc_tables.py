"""Marching-cubes case table: the generator of mli_nerf_amd/csrc/mc_table.h.

``python -m mli_nerf_amd.mc_tables`` rewrites the header; tests/test_mesh_tables.py checks that
the committed header is what this module generates.

Conventions (shared with csrc/mesh.hip and mesh.py):

* corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell origin;
  bit c of the 8-bit case is set when that corner is INSIDE (s < iso);
* edge e = 4 * axis + n joins corner EDGE_CORNER[e] to the corner one step along +axis:
  edges 0-3 run along x from corners 0, 2, 4, 6, edges 4-7 along y from 0, 1, 4, 5, edges 8-11
  along z from 0, 1, 2, 3;
* every face is looked at from outside the cube, its corners in counter-clockwise order.

Construction of a case: on each face the crossed edges are joined into segments that cut off the
maximal runs of inside corners (an ambiguous face, inside / outside alternating, has two runs of
one corner: the segments cut off the INSIDE corners -- a rule of the face's four signs alone, so
the two cells sharing a face agree).  A segment is directed from the edge where the walk round the
face enters the run to the edge where it leaves it; the directed segments of the six faces link
into closed loops whose right-hand normal points from inside to outside (toward increasing SDF).
Each loop is fan-triangulated from its lowest-numbered edge whose fan has no diagonal inside a
cube face (fan_apex; almost always the lowest edge of the loop).  The triangulation is this project's
own: it differs from PyMCubes' on some cases, the vertex set (one vertex per sign-changing lattice
edge) cannot.
"""
import os

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.h")

CORNER_OFFSET = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
# lower corner of each edge, and its axis
EDGE_CORNER = [0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3]
EDGE_AXIS = [e // 4 for e in range(12)]
EDGE_ENDS = [(EDGE_CORNER[e], EDGE_CORNER[e] | (1 << EDGE_AXIS[e])) for e in range(12)]
_EDGE_OF = {frozenset(ends): e for e, ends in enumerate(EDGE_ENDS)}


def _faces():
    """The 6 faces (axis a, side s) as 4 corners, counter-clockwise seen from outside."""
    faces = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3   # e_b x e_c = e_a
        for side in (0, 1):
            cyc = [(0, 0), (1, 0), (1, 1), (0, 1)]   # counter-clockwise about +e_a
            if side == 0:
                cyc = cyc[::-1]
            faces.append([(side << a) | (u << b) | (v << c) for u, v in cyc])
    return faces


FACES = _faces()


def face_segments(corners, inside):
    """Directed segments [(edge_in, edge_out)] on one face: ``corners`` its 4 corner numbers in
    counter-clockwise order, ``inside`` their 4 flags."""
    if all(inside) or not any(inside):
        return []
    segs = []
    for i in range(4):
        # a maximal run of inside corners starts at i (the corner before it is outside)
        if inside[i] and not inside[i - 1]:
            j = i
            while inside[(j + 1) % 4]:
                j += 1
            e_in = _EDGE_OF[frozenset((corners[i - 1], corners[i]))]
            e_out = _EDGE_OF[frozenset((corners[j % 4], corners[(j + 1) % 4]))]
            segs.append((e_in, e_out))
    return segs


def case_segments(case):
    segs = []
    for corners in FACES:
        segs += face_segments(corners, [bool(case >> c & 1) for c in corners])
    return segs


def case_loops(case):
    """Closed loops of edge numbers, each starting at its lowest edge, in case order of that edge."""
    nxt = {}
    for a, b in case_segments(case):
        assert a not in nxt, (case, a)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), case   # every crossed edge: one segment in, one out
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, case
        loops.append(loop)
    return loops


def _edge_faces(e):
    a, b = EDGE_ENDS[e]
    return {i for i, f in enumerate(FACES) if a in f and b in f}


def fan_apex(loop):
    """Position in ``loop`` of the fan's apex: the lowest-numbered edge from which no fan diagonal
    joins two edges of one cube face.  Such a diagonal lies in the face, where the neighbouring
    cell may draw the same one -- four triangles on one mesh edge.  (On an ambiguous face a loop
    can cross the face twice; 18 of the 358 loops need an apex other than their lowest edge, and
    every loop has one.)"""
    n = len(loop)
    for e in sorted(loop):
        s = loop.index(e)
        rot = loop[s:] + loop[:s]
        if all(not (_edge_faces(rot[0]) & _edge_faces(rot[i])) for i in range(2, n - 1)):
            return s
    raise AssertionError(loop)


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        s = fan_apex(loop)
        rot = loop[s:] + loop[:s]
        for i in range(1, len(rot) - 1):
            tris.append((rot[0], rot[i], rot[i + 1]))
    return tris


TRI_TABLE = [case_triangles(k) for k in range(256)]
TRI_COUNT = [len(t) for t in TRI_TABLE]
assert max(TRI_COUNT) <= 5


def render_header():
    out = ["/* mc_table.h -- marching-cubes case table.  GENERATED by mli_nerf_amd/mc_tables.py",
           " * (python -m mli_nerf_amd.mc_tables); do not edit.  Conventions: see that module. */",
           "#ifndef MLI_MC_TABLE_H", "#define MLI_MC_TABLE_H", "",
           "#ifndef MLI_MC_QUAL", "#define MLI_MC_QUAL static const", "#endif", "",
           "/* edge -> lower corner offset (x, y, z) and axis */",
           "MLI_MC_QUAL unsigned char MLI_MC_EDGE_CORNER[12][3] = {"]
    out.append("  " + ", ".join("{%d, %d, %d}" % CORNER_OFFSET[EDGE_CORNER[e]] for e in range(12)))
    out += ["};", "MLI_MC_QUAL unsigned char MLI_MC_EDGE_AXIS[12] = {",
            "  " + ", ".join(str(a) for a in EDGE_AXIS), "};", "",
            "/* triangles per case (bit c of the case: corner c inside, s < iso) */",
            "MLI_MC_QUAL unsigned char MLI_MC_TRI_COUNT[256] = {"]
    for r in range(0, 256, 32):
        out.append("  " + ", ".join(str(n) for n in TRI_COUNT[r:r + 32]) + ",")
    out += ["};", "",
            "/* per case: 3 edge numbers per triangle, up to 5 triangles; 255 = unused (16th byte: pad) */",
            "MLI_MC_QUAL unsigned char MLI_MC_TRI_EDGES[256][16] = {"]
    for k in range(256):
        flat = [e for t in TRI_TABLE[k] for e in t]
        flat += [255] * (16 - len(flat))
        out.append("  {" + ", ".join("%d" % e for e in flat) + "},  /* %d */" % k)
    out += ["};", "", "#endif", ""]
    return "\n".join(out)


def parse_header(text):
    """(edge_corner [12][3], edge_axis [12], tri_count [256], tri_edges [256][16]) of a header."""
    import re

    def ints(name):
        m = re.search(name + r"(?:\[\d+\])+ = \{(.*?)\};", text, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        return [int(x) for x in re.findall(r"\d+", body)]
    ec, tri = ints("MLI_MC_EDGE_CORNER"), ints("MLI_MC_TRI_EDGES")
    return ([ec[3 * e:3 * e + 3] for e in range(12)], ints("MLI_MC_EDGE_AXIS"), ints("MLI_MC_TRI_COUNT"),
            [tri[16 * k:16 * k + 16] for k in range(256)])


if __name__ == "__main__":
    with open(HEADER, "w") as f:
        f.write(render_header())
    print(HEADER)
