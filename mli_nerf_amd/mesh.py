"""Surface extraction: the SDF's iso-surface as a welded triangle mesh, on the GPU.

Replaces projects/neuralangelo/scripts/extract_mesh.py + projects/neuralangelo/utils/mesh.py
(mcubes + trimesh) with the marching-cubes kernels of libmli_hip.so (include/mli_mesh.h):

* ``marching_cubes(sdf, ...)``: one lattice -> vertices, faces and their keys;
* ``extract_mesh(model, ...)``: the model's SDF on a lattice in blocks (the existing mli_sdf SDF
  mode, a lattice column along z as a pseudo-ray), marching cubes per block, the blocks welded by
  vertex key, optional per-vertex normals (FIELD mode) and colours (the heads, under a stated light);
* ``connected_components(faces, n_verts, verts)`` / ``filter_components(mesh, ...)``: the mesh's
  components, their face counts and areas (include/mli_mesh_cc.h) and the mesh cut down to the
  largest one or to those above a size (``extract_mesh(keep_lcc=True)``, ``--keep_lcc``);
* ``write_ply(path, mesh)``; ``python -m mli_nerf_amd.mesh`` is the command-line form.

Differences from the reference, on purpose: the triangulation is this project's own table
(mc_tables.py; the vertex set is any marching cubes'); vertices are welded across blocks; the
sign convention is the project's (negative inside, triangles face outside; the reference negates
the SDF for mcubes); --keep_lcc keeps the largest component of the whole welded mesh, chosen by a
fixed-point area with stated tie rules (the reference applies it to every block's unwelded piece
on its own); blocks are not spread over ranks; vertex colours need an explicit light position
(LumenRGB.forward needs pts_light, which the reference's extract_texture does not pass); the
lattice includes the upper bound's plane (the reference's arange(min, max, intv) stops one step
short of it).
"""
import collections
import math
import sys
import time

import numpy as np
import torch

from . import _lib as L

ATTRIBUTES = ("normal", "reflectance", "shading", "rgb")
_CHUNK = 1 << 20  # vertices per attribute pass


class Mesh:
    """verts [V,3] f32, faces [F,3] int64, normals [V,3] f32 or None, colors {name: [V,3] f32 in
    [0,1]} (``color``: the first one), keys [V] int64 vertex keys, face_keys [F] int64."""

    def __init__(self, verts, faces, normals=None, colors=None, keys=None, face_keys=None):
        self.verts, self.faces, self.normals = verts, faces, normals
        self.colors = colors or {}
        self.keys, self.face_keys = keys, face_keys

    @property
    def color(self):
        return next(iter(self.colors.values()), None)


# ---------------------------------------------------------------------------- one lattice
def _mc_args(sdf, iso, origin, spacing, offset, gdims):
    nx, ny, nz = sdf.shape
    sx, sy, sz = sdf.stride()
    gx, gy, gz = gdims if gdims is not None else (nx, ny, nz)
    a = L.McArgs()
    a.sdf, a.nx, a.ny, a.nz, a.sx, a.sy, a.sz = L.ptr(sdf), nx, ny, nz, sx, sy, sz
    a.iso, a.spacing = float(iso), float(spacing)
    a.origin = (L.F32 * 3)(*[float(x) for x in origin])
    a.off_x, a.off_y, a.off_z = [int(x) for x in offset]
    a.gx, a.gy, a.gz = int(gx), int(gy), int(gz)
    return a


def mc_workspace(shape):
    """Element counts (int32) of the chunk-base, counts and edge-slot scratch marching_cubes
    allocates for a lattice (the library's mli_mc_*_workspace queries give the same, in bytes)."""
    n = int(np.prod(shape))
    if min(shape) < 2 or 3 * n >= 2 ** 31:
        raise ValueError("marching_cubes: lattice %s: every side needs >= 2 points and 3 * points < 2^31"
                         % (tuple(shape),))
    return (n + L.MC_CHUNK - 1) // L.MC_CHUNK * 2, 2, 3 * n


@torch.no_grad()
def marching_cubes(sdf, iso=0.0, origin=(0.0, 0.0, 0.0), spacing=1.0, offset=(0, 0, 0), gdims=None, scratch=None):
    """Iso-surface of one fp32 lattice ``sdf`` [nx,ny,nz] (a CUDA tensor, any non-negative strides).

    Returns ``verts [V,3] f32, faces [F,3] int64, vert_keys [V] int64, face_keys [F] int64``.
    Inside is ``sdf < iso``; triangles face outside.  ``offset`` / ``gdims``: the lattice is a
    block of a larger one (keys and positions from global indices).  Output order is fixed for a
    given input (bit-reproducible) but otherwise unspecified; sort by key for a canonical mesh."""
    if not (torch.is_tensor(sdf) and sdf.is_cuda and sdf.dtype == torch.float32 and sdf.dim() == 3):
        raise ValueError("marching_cubes: a CUDA float32 tensor [nx, ny, nz] is needed")
    dev = sdf.device
    a = _mc_args(sdf, iso, origin, spacing, offset, gdims)
    n_cb, n_cnt, n_es = mc_workspace(sdf.shape)
    buf = scratch if scratch is not None else {}

    def get(name, n):
        t = buf.get(name)
        if t is None or t.numel() < n or t.device != dev:
            t = buf[name] = torch.empty(n, dtype=torch.int32, device=dev)
        return t
    chunk_base, counts, edge_slot = get("chunk_base", n_cb), get("counts", n_cnt), get("edge_slot", n_es)
    a.chunk_base, a.counts, a.edge_slot = L.ptr(chunk_base), L.ptr(counts), L.ptr(edge_slot)
    with torch.cuda.device(dev):
        L.call("mli_mc_count", a)
        n_v, n_f = counts[:2].tolist()   # the one synchronisation: the outputs' sizes
        verts = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
        vkeys = torch.empty(n_v, dtype=torch.int64, device=dev)
        faces = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
        fkeys = torch.empty(n_f, dtype=torch.int64, device=dev)
        a.max_vertices, a.max_triangles = n_v, n_f
        a.verts, a.vert_keys, a.faces, a.face_keys = L.ptr(verts), L.ptr(vkeys), L.ptr(faces), L.ptr(fkeys)
        L.call("mli_mc_emit", a)
    return verts, faces.to(torch.int64), vkeys, fkeys


# ---------------------------------------------------------------------------- the model's surface
def lattice_axis(lo, hi, intv):
    """Lattice coordinates lo + i * intv up to and including hi (float64; cast where used)."""
    n = int(math.floor((hi - lo) / intv + 1e-6)) + 1
    return lo + np.arange(n, dtype=np.float64) * intv


def _blocks(n_points, block_res):
    """[(first point, last point)] of blocks of block_res cells; neighbours share a plane."""
    return [(i0, min(i0 + block_res, n_points - 1)) for i0 in range(0, n_points - 1, block_res)]


def _lattice_sdf(eng, xs, ys, z0, zd, out_buf):
    """The SDF on the lattice points (xs[i], ys[j], z0 + zd[k]) through mli_sdf (SDF mode): one
    pseudo-ray per (i, j) column, direction +z, dists zd.  Returns the [nz][nx*ny] output viewed
    as [nx, ny, nz] (strides (ny, 1, nx*ny))."""
    nx, ny, nz = xs.numel(), ys.numel(), zd.numel()
    R = nx * ny
    dev = xs.device
    center = torch.empty(nx, ny, 3, device=dev)
    center[..., 0] = xs[:, None]
    center[..., 1] = ys[None, :]
    center[..., 2] = z0
    ray_unit = torch.zeros(R, 3, device=dev)
    ray_unit[:, 2] = 1.0
    dists = zd[:, None].expand(nz, R).contiguous()
    n = nz * R
    out = out_buf.get("sdf")
    if out is None or out.numel() < n:
        out = out_buf["sdf"] = torch.empty(n, device=dev)
    out = out[:n].view(nz, R)
    eng._sdf(dict(center=center.view(R, 3), ray_unit=ray_unit, outside=None), dists, nz, out)
    return out.view(nz, nx, ny).permute(1, 2, 0)


def _check_attributes(model, attributes, light):
    attributes = tuple(attributes or ())
    for name in attributes:
        if name not in ATTRIBUTES:
            raise ValueError("extract_mesh: unknown attribute %r (known: %s)" % (name, ", ".join(ATTRIBUTES)))
    colours = [n for n in attributes if n != "normal"]
    if model.stage == "a":
        missing = [n for n in colours if n != "rgb"]
        if missing:
            raise ValueError("extract_mesh: attribute %s needs the intrinsic heads; this model is stage a "
                             "(LumenRGB mode 'rgb') and offers only 'rgb'" % ", ".join(repr(n) for n in missing))
    if colours and light is None:
        raise ValueError("extract_mesh: attribute %s is evaluated under a light; pass light=(x, y, z), the "
                         "world-space light position" % ", ".join(repr(n) for n in colours))
    return attributes


@torch.no_grad()
def vertex_attributes(model, verts, attributes=("normal",), light=None):
    """Per-vertex attributes of points ``verts`` [V,3]: 'normal' = the normalised 4-tap SDF
    gradient (mli_sdf FIELD mode); 'reflectance' / 'shading' / 'rgb' = the heads' outputs
    (mli_rgb_fwd) seen along -normal under the light at ``light``.  Returns {name: [V,3]}."""
    attributes = _check_attributes(model, attributes, light)
    eng = model.engine
    dev = verts.device
    V = verts.shape[0]
    out = {n: torch.empty(V, 3, device=dev) for n in attributes}
    colours = [n for n in attributes if n != "normal"]
    slots = {"rgb": slice(0, 3), "reflectance": slice(3, 6), "shading": slice(6, 7)}
    for v0 in range(0, V, _CHUNK):
        v1 = min(v0 + _CHUNK, V)
        n = v1 - v0
        R = -(-n // 256) * 256   # whole 256-sample workgroups of the heads: pad with vertex 0
        pts = verts[v0:v1] if R == n else torch.cat([verts[v0:v1], verts[:1].expand(R - n, 3)], 0)
        rays = dict(center=pts.contiguous(), ray_unit=torch.zeros(R, 3, device=dev),
                    outside=torch.zeros(R, dtype=torch.uint8, device=dev))
        dists = torch.zeros(1, R, device=dev)
        fld = eng.field(rays, dists, training=False)
        normal = torch.nn.functional.normalize(fld["grad"].view(R, 3), dim=-1)
        if "normal" in out:
            out["normal"][v0:v1] = normal[:n]
        if colours:
            rays["ray_unit"] = (-normal).contiguous()
            rays["pts_light"] = torch.tensor([float(x) for x in light], device=dev).expand(R, 3).contiguous()
            y = eng.heads(rays, dists, fld, training=False)["y"].view(R, 8)
            for name in colours:
                out[name][v0:v1] = y[:n, slots[name]].expand(n, 3)
    return out


# ---------------------------------------------------------------------------- connected components
class Components(collections.namedtuple("Components", "label ids n_faces area area_q rounds")):
    """label [V] int32 (the smallest vertex index of each vertex's component); ids [C] int64 the
    labels that own >= 1 face, ascending; n_faces [C] int32; area [C] float64 (None without
    vertices); area_q [C] int64 fixed-point area; rounds: labelling rounds run."""


def cc_max_rounds(n_verts):
    """The default round cap 2 * ceil(log2(max(V, 2))) + 8."""
    return 2 * (max(int(n_verts), 2) - 1).bit_length() + 8


def cc_workspace(n_verts, n_faces, max_rounds=None):
    """Element counts of label (int32), changed (int32), comp_faces (int32) and comp_area + max_q
    (int64) as connected_components allocates them (mli_cc_init_workspace gives the bytes)."""
    if not (1 <= n_verts < 2 ** 31 and 0 <= n_faces < 2 ** 31):
        raise ValueError("connected_components: 1 <= n_verts < 2^31 and 0 <= faces < 2^31 are needed, got %d and %d"
                         % (n_verts, n_faces))
    max_rounds = cc_max_rounds(n_verts) if max_rounds is None else int(max_rounds)
    if not 1 <= max_rounds <= L.MESH_CC_MAX_ROUNDS:
        raise ValueError("connected_components: max_rounds %d is outside 1 .. %d" % (max_rounds, L.MESH_CC_MAX_ROUNDS))
    return n_verts, max_rounds, n_verts, n_verts + 1


def area_unit(verts):
    """(unit, 2^(44-e)) of the fixed-point face area: unit = 2^(e-44), e = ceil(log2(d2)), d2 the
    squared diagonal of the vertices' bounding box in float64; (1, 1) when d2 = 0."""
    ext = (verts.max(dim=0)[0].double() - verts.min(dim=0)[0].double()).tolist()
    d2 = (ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2]
    if not math.isfinite(d2):
        raise ValueError("connected_components: the vertices are not finite")
    if d2 == 0.0:
        return 1.0, 1.0
    m, e = math.frexp(d2)   # d2 = m * 2^e, 0.5 <= m < 1
    if m == 0.5:
        e -= 1
    return math.ldexp(1.0, e - 44), math.ldexp(1.0, 44 - e)


@torch.no_grad()
def connected_components(faces, n_verts, verts=None, max_rounds=None, timings=None):
    """Connected components of the graph whose vertices are 0 .. n_verts-1 and in which two
    vertices are adjacent when a face names both (``faces`` [F,3] int64, a CUDA tensor).

    Returns ``Components``.  A face belongs to the component of its first vertex.  With ``verts``
    [V,3] f32 the components' areas are summed in fixed point (order-independent, the same bits
    every run); without, area is None and area_q is 0.  Raises ValueError for an index outside
    [0, n_verts) (checked before any launch) and RuntimeError when ``max_rounds`` rounds (default
    cc_max_rounds) did not converge.  ``timings``: receives the seconds of 'labelling' and 'stats'."""
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.dtype == torch.int64 and faces.dim() == 2
            and faces.shape[1] == 3):
        raise ValueError("connected_components: faces must be a CUDA int64 tensor [F, 3]")
    dev = faces.device
    n_verts, F = int(n_verts), int(faces.shape[0])
    n_label, n_changed, n_cf, n_area = cc_workspace(n_verts, F, max_rounds)
    if verts is not None and not (torch.is_tensor(verts) and verts.device == dev and verts.dtype == torch.float32
                                  and tuple(verts.shape) == (n_verts, 3)):
        raise ValueError("connected_components: verts must be a float32 tensor [n_verts, 3] on the faces' device")
    if F and not (int(faces.min()) >= 0 and int(faces.max()) < n_verts):
        raise ValueError("connected_components: a face names a vertex outside 0 .. %d" % (n_verts - 1))
    unit, inv_unit = area_unit(verts) if verts is not None else (1.0, 1.0)
    clock = _Clock(timings, dev)
    if F == 0:   # nothing to launch: every vertex is its own component and owns no face
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        return Components(torch.arange(n_verts, dtype=torch.int32, device=dev), empty, empty.to(torch.int32),
                          None if verts is None else empty.double(), empty, 0)
    faces = faces.contiguous()
    verts = None if verts is None else verts.contiguous()
    label = torch.empty(n_label, dtype=torch.int32, device=dev)
    changed = torch.empty(n_changed, dtype=torch.int32, device=dev)
    comp_faces = torch.empty(n_cf, dtype=torch.int32, device=dev)
    area_buf = torch.empty(n_area, dtype=torch.int64, device=dev)   # comp_area [V], then max_q
    a = L.MeshCcArgs()
    a.faces, a.n_faces, a.n_verts = L.ptr(faces), F, n_verts
    a.verts = L.ptr(verts)
    a.label, a.changed, a.max_rounds = L.ptr(label), L.ptr(changed), n_changed
    a.comp_faces, a.comp_area, a.max_q = L.ptr(comp_faces), L.ptr(area_buf), L.ptr(area_buf[n_verts:])
    a.inv_unit = inv_unit
    with torch.cuda.device(dev):
        L.call("mli_cc_init", a)
        for r in range(n_changed):
            a.round = r
            L.call("mli_cc_round", a)
            if not int(changed[r]):   # the round lowered nothing: the fixpoint
                break
        else:
            raise RuntimeError("connected_components: no fixpoint after %d rounds (%d vertices, %d faces)"
                               % (n_changed, n_verts, F))
        clock.lap("labelling")
        L.call("mli_cc_stats", a)
        max_q, most = int(area_buf[n_verts]), int(comp_faces.max())
    if max_q * most >= 2 ** 63:
        raise ValueError("connected_components: the fixed-point area may overflow (largest face %d units, %d faces "
                         "in one component)" % (max_q, most))
    ids = torch.nonzero(comp_faces > 0).view(-1)
    area_q = area_buf[:n_verts][ids]
    out = Components(label, ids, comp_faces[ids], None if verts is None else area_q.double() * unit, area_q, r + 1)
    clock.lap("stats")
    return out


def largest_component(ids, n_faces, area_q, by="area"):
    """Position in ``ids`` of the largest component: the greatest area_q, then the most faces, then
    the lowest label (``by='faces'``: the most faces, then the lowest label).  Host arrays."""
    if by not in ("area", "faces"):
        raise ValueError("filter_components: by=%r (known: 'area', 'faces')" % (by,))
    ids, n_faces, area_q = (np.asarray(x, dtype=np.int64) for x in (ids, n_faces, area_q))
    keys = (ids, -n_faces, -area_q) if by == "area" else (ids, -n_faces)
    return int(np.lexsort(keys)[0])


@torch.no_grad()
def filter_components(mesh, keep="largest", by="area", min_faces=0, min_area=0.0, timings=None):
    """A new ``Mesh`` with the components of ``mesh`` that have >= ``min_faces`` faces and an area
    >= ``min_area``: all of them (``keep='all'``) or the largest (``keep='largest'``; see
    largest_component for ``by`` and the tie rules).  Vertices no kept face names are dropped; the
    order of vertices and faces is preserved; normals, colours, keys and face keys are carried."""
    if keep not in ("largest", "all"):
        raise ValueError("filter_components: keep=%r (known: 'largest', 'all')" % (keep,))
    if by not in ("area", "faces"):
        raise ValueError("filter_components: by=%r (known: 'area', 'faces')" % (by,))
    verts, faces = mesh.verts, mesh.faces
    dev = verts.device
    V = verts.shape[0]
    vkeep = torch.zeros(V, dtype=torch.bool, device=dev)
    if V and faces.shape[0]:
        cc = connected_components(faces, V, verts, timings=timings)
        ok = (cc.n_faces >= int(min_faces)) & (cc.area >= float(min_area))
        ids, n_f, a_q = (t[ok].cpu().numpy() for t in (cc.ids, cc.n_faces, cc.area_q))
        if keep == "largest" and ids.size:
            ids = ids[largest_component(ids, n_f, a_q, by):][:1]
        kept = torch.zeros(V, dtype=torch.bool, device=dev)
        kept[torch.from_numpy(ids).to(dev)] = True
        vkeep = kept[cc.label.long()]
    clock = _Clock(timings, dev)
    fkeep = vkeep[faces[:, 0]] if faces.shape[0] else torch.zeros(0, dtype=torch.bool, device=dev)
    remap = torch.cumsum(vkeep.to(torch.int64), 0) - 1

    def rows(t, mask):
        return None if t is None else t[mask]
    out = Mesh(verts[vkeep], remap[faces[fkeep]], rows(mesh.normals, vkeep),
               {n: c[vkeep] for n, c in mesh.colors.items()}, rows(mesh.keys, vkeep), rows(mesh.face_keys, fkeep))
    clock.lap("compaction")
    return out


@torch.no_grad()
def extract_mesh(model, resolution=512, block_res=256, bounds=None, attributes=("normal",), light=None,
                 weld=True, sphere_filter=True, scale=1.0, center=(0.0, 0.0, 0.0), timings=None,
                 keep_lcc=False, min_component_faces=0):
    """The model's zero level set as a ``Mesh`` (device tensors).

    ``resolution``: lattice spacing 2 / resolution; ``bounds`` [[x0,x1],[y0,y1],[z0,z1]] (default:
    the config's AABB for a box-bounded scene, else [-1,1]^3); ``block_res``: cells per block side
    (the result does not depend on it); ``weld``: one vertex per lattice edge across blocks,
    vertices sorted by key and faces by face key; ``sphere_filter``: for a sphere-bounded scene drop
    vertices with |v| >= 1 and the faces touching them; ``scale`` / ``center``: v * scale + center,
    applied last.  ``timings``: a dict that receives the seconds spent per phase (synchronises).
    ``keep_lcc``: keep only the largest connected component (filter_components: by area, then
    faces, then lowest label); ``min_component_faces``: drop the components with fewer faces.
    Both act on the welded, sphere-filtered mesh, before the attributes are evaluated."""
    attributes = _check_attributes(model, attributes, light)
    if (keep_lcc or min_component_faces) and not weld:
        raise ValueError("extract_mesh: keep_lcc / min_component_faces need weld=True (the blocks' copies of a "
                         "shared vertex would split every component along the block planes)")
    model.eval()
    model.prepare()   # the engine as trained: active_levels, tap epsilon, weights
    eng = model.engine
    dev = model.flat.device
    pc = model.pcfg
    intv = 2.0 / resolution
    if bounds is None:
        bounds = [[pc.aabb[i], pc.aabb[i + 3]] for i in range(3)] if pc.bounding == "box" else [[-1.0, 1.0]] * 3
    axes = [lattice_axis(float(lo), float(hi), intv) for lo, hi in bounds]
    G = [len(ax) for ax in axes]
    if min(G) < 2:
        raise ValueError("extract_mesh: bounds %r hold fewer than 2 lattice points at spacing %g" % (bounds, intv))
    origin = [float(ax[0]) for ax in axes]
    xs, ys = (torch.from_numpy(ax).to(torch.float32).to(dev) for ax in axes[:2])
    # z = z_min + fp32(gk * intv): the pseudo-ray's distance, from the GLOBAL index, so a lattice
    # point has the same coordinates (and SDF bits) whichever block evaluates it
    zd = torch.from_numpy(np.arange(G[2], dtype=np.float64) * intv).to(torch.float32).to(dev)

    clock = _Clock(timings, dev)
    scratch, sdf_buf = {}, {}
    parts, v_off = [], 0
    for i0, i1 in _blocks(G[0], block_res):
        for j0, j1 in _blocks(G[1], block_res):
            for k0, k1 in _blocks(G[2], block_res):
                lat = _lattice_sdf(eng, xs[i0:i1 + 1], ys[j0:j1 + 1], origin[2], zd[k0:k1 + 1], sdf_buf)
                clock.lap("lattice_sdf")
                v, f, vk, fk = marching_cubes(lat, 0.0, origin, intv, (i0, j0, k0), G, scratch)
                clock.lap("marching_cubes")
                if v.shape[0]:
                    parts.append((v, f + v_off, vk, fk))
                    v_off += v.shape[0]
    if parts:
        verts, faces, keys, fkeys = (torch.cat(p, 0) for p in zip(*parts))
    else:
        verts, faces = torch.empty(0, 3, device=dev), torch.empty(0, 3, dtype=torch.int64, device=dev)
        keys, fkeys = (torch.empty(0, dtype=torch.int64, device=dev) for _ in range(2))
    if weld and keys.numel():
        # one vertex per key (the copies of a shared-plane vertex are bit-identical); ascending
        # key order; faces ascending by face key
        uniq, inverse = torch.unique(keys, sorted=True, return_inverse=True)
        first = torch.full((uniq.numel(),), keys.numel(), dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, inverse, torch.arange(keys.numel(), device=dev), reduce="amin")
        verts, keys = verts[first], uniq
        faces = inverse[faces]
        order = torch.argsort(fkeys)
        faces, fkeys = faces[order], fkeys[order]
    if sphere_filter and pc.bounding != "box" and verts.shape[0]:
        keep = verts.norm(dim=-1) < 1.0   # filter_points_outside_bounding_sphere (mesh.py:136-148)
        remap = torch.cumsum(keep.to(torch.int64), 0) - 1
        fkeep = keep[faces].all(dim=-1)
        verts, keys = verts[keep], keys[keep]
        faces, fkeys = remap[faces[fkeep]], fkeys[fkeep]
    clock.lap("stitch")
    if (keep_lcc or min_component_faces) and verts.shape[0]:
        # filter_largest_cc (mesh.py:151-158), on the whole welded mesh
        kept = filter_components(Mesh(verts, faces, keys=keys, face_keys=fkeys), keep="largest" if keep_lcc else "all",
                                 min_faces=min_component_faces)
        verts, faces, keys, fkeys = kept.verts, kept.faces, kept.keys, kept.face_keys
        clock.lap("components")
    attrs =vertex_attributes(model, verts, attributes, light) if verts.shape[0] else \
        {n: torch.empty(0, 3, device=dev) for n in attributes}
    clock.lap("attributes")
    normals = attrs.pop("normal", None)
    sc = torch.tensor([float(x) for x in center], device=dev)
    verts = verts * float(scale) + sc
    return Mesh(verts, faces, normals, attrs, keys, fkeys)


class _Clock:
    def __init__(self, timings, dev):
        self.t, self.dev, self.time = timings, dev, time.perf_counter
        if timings is not None:
            torch.cuda.synchronize(dev)
            self.last = self.time()

    def lap(self, name):
        if self.t is None:
            return
        torch.cuda.synchronize(self.dev)
        now = self.time()
        self.t[name] = self.t.get(name, 0.0) + now - self.last
        self.last = now


# ---------------------------------------------------------------------------- PLY
def write_ply(path, mesh):
    """Binary little-endian PLY: x y z float, nx ny nz float when the mesh has normals, red
    green blue uchar when it has colours (clamped, round(x * 255)), faces as
    ``list uchar int vertex_indices``.  Faces with two equal vertex positions are dropped
    (trimesh's nondegenerate_faces, extract_mesh.py:119).  Returns (n_vertices, n_faces) written."""
    def host(t, dtype):
        return None if t is None else np.ascontiguousarray(
            t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dtype)
    v = host(mesh.verts, "<f4").reshape(-1, 3)
    f = host(mesh.faces, "<i4").reshape(-1, 3)
    n = host(mesh.normals, "<f4")
    c = host(mesh.color, "<f4")
    if f.shape[0]:
        p = v[f]
        ok = ~((p[:, 0] == p[:, 1]).all(-1) | (p[:, 1] == p[:, 2]).all(-1) | (p[:, 0] == p[:, 2]).all(-1))
        f = f[ok]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0],
            "property float x", "property float y", "property float z"]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        head += ["property float nx", "property float ny", "property float nz"]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    rec = np.zeros(v.shape[0], dtype=fields)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        n = n.reshape(-1, 3)
        rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if c is not None:
        c8 = np.rint(np.clip(c.reshape(-1, 3), 0.0, 1.0) * 255.0).astype("u1")
        rec["red"], rec["green"], rec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.zeros(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"], frec["i"] = 3, f
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        out.write(rec.tobytes())
        out.write(frec.tobytes())
    return v.shape[0], f.shape[0]


# ---------------------------------------------------------------------------- command line
def main(argv=None):
    """extract_mesh.py's flags: --config --checkpoint --resolution --block_res --output_file;
    --textured becomes --attributes normal,reflectance --light x,y,z; --keep_lcc keeps the largest
    component of the whole mesh, --min_component_faces N drops the smaller ones.  --config is a
    YAML path or the name of a built-in preset; --a.b.c=v overrides follow."""
    import argparse
    import os
    from .trainer import Trainer
    ap = argparse.ArgumentParser(description="Extract the SDF surface as a PLY mesh")
    ap.add_argument("--config", required=True)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--block_res", type=int, default=256)
    ap.add_argument("--output_file", default="mesh.ply")
    ap.add_argument("--attributes", default="normal", help="comma list of: " + ", ".join(ATTRIBUTES))
    ap.add_argument("--light", default=None, help="world-space light position x,y,z (for colours)")
    ap.add_argument("--scale", type=float, default=1.0, help="sphere_radius of the scene's annotation")
    ap.add_argument("--center", default="0,0,0", help="sphere_center of the scene's annotation")
    ap.add_argument("--keep_lcc", action="store_true", help="keep only the largest connected component")
    ap.add_argument("--min_component_faces", type=int, default=0, help="drop components with fewer faces")
    args, cfg_cmd = ap.parse_known_args(argv)
    from . import configs
    from .config import load_config, parse_overrides
    if not os.path.exists(args.config) and args.config in configs.PRESETS:
        cfg = configs.preset(args.config, overrides=parse_overrides(cfg_cmd))
    else:
        cfg = load_config(args.config, overrides=cfg_cmd)
    cfg.logdir = ""
    trainer = Trainer(cfg, is_inference=True, seed=0)
    if args.checkpoint is not None:
        trainer.checkpointer.load(args.checkpoint, load_opt=False, load_sch=False)
    trainer.model.eval()
    # the coarse-to-fine levels and tap epsilon of the checkpoint's iteration (extract_mesh.py:75-79)
    if trainer.checkpointer.eval_iteration is not None:
        trainer.current_iteration = trainer.checkpointer.eval_iteration
    trainer._start_of_iteration()
    attributes = tuple(a for a in args.attributes.split(",") if a)
    light = None if args.light is None else tuple(float(x) for x in args.light.split(","))
    mesh = extract_mesh(trainer.model, resolution=args.resolution, block_res=args.block_res, attributes=attributes,
                        light=light, scale=args.scale, center=tuple(float(x) for x in args.center.split(",")),
                        keep_lcc=args.keep_lcc, min_component_faces=args.min_component_faces)
    out_dir = os.path.dirname(args.output_file)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    n_v, n_f = write_ply(args.output_file, mesh)
    print("vertices: %d\nfaces: %d" % (n_v, n_f))
    return 0


if __name__ == "__main__":
    sys.exit(main())
