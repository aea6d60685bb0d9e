"""Wall time of mesh.extract_mesh on synthetic weights, split by phase, as one JSON record.

  python tools/mesh_profile.py --resolution 512 --block_res 128 --out profiles/mesh/res512_block128.json
  python tools/mesh_profile.py --oracle --out profiles/mesh/oracle_cpu.json      (CPU, for scale)
  python tools/mesh_profile.py --block_res 256 --keep_lcc --out profiles/mesh/res512_block256_lcc.json

Phases (host wall clock with a device synchronisation after each, mesh._Clock): lattice_sdf (the
mli_sdf SDF-mode calls and their inputs), marching_cubes (count, the size read-back, emit),
stitch (concatenate, weld, sort, filter), attributes (FIELD + heads at the vertices).  The
marching-cubes launches are also timed with device events (_lib.PROFILE), which leaves out the
read-back: achieved bytes/s = passes * 4 B * lattice points / that time.  --keep_lcc: the run
with and without the connected-component filter in turn, the phase "components" split into
labelling / stats / compaction, the rounds used, and scipy on the host for scale.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MC_PASSES = 3   # count, emit, triangles: each reads the lattice once (4 B per point)


def oracle_record(log2T):
    from mli_nerf_amd import synthetic
    from mli_nerf_amd.mesh import lattice_axis
    from oracle import render as o_render
    sd = synthetic.make_state_dict(log2T=log2T)
    cfg = o_render.PathCfg(log2T=log2T)
    g = torch.from_numpy(lattice_axis(-1.0, 1.0, 2.0 / 32)).float()
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1)
    with torch.no_grad():
        o_render.sdf_net(sd, cfg, pts, False)
        t = time.perf_counter()
        o_render.sdf_net(sd, cfg, pts, False)
        dt = time.perf_counter() - t
    n = pts[..., 0].numel()
    return dict(what="CPU oracle lattice SDF", log2T=log2T, points=n, seconds=dt, threads=torch.get_num_threads(),
                extrapolated_seconds_513cubed=dt * 513 ** 3 / n,
                note="EXTRAPOLATION: the 33^3 time scaled by the point count, for scale only")


def gpu_record(args):
    from mli_nerf_amd import _lib as L
    from mli_nerf_amd import synthetic
    from mli_nerf_amd.configs import preset
    from mli_nerf_amd.mesh import extract_mesh
    from mli_nerf_amd.model import Model
    cfg = preset("syn_hotdog_b", log2T=args.log2T)
    model = Model(cfg.model, cfg.data)
    model.load_state_dict(synthetic.make_state_dict(log2T=args.log2T))
    model = model.to("cuda:0")
    kw = dict(resolution=args.resolution, block_res=args.block_res, attributes=("normal", "reflectance"),
              light=(1.5, -2.0, 2.5))
    if args.keep_lcc:
        return lcc_record(args, model, kw)
    extract_mesh(model, **kw)   # warm-up: allocations, first launches
    runs = []
    for _ in range(args.repeats):
        timings = {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        mesh = extract_mesh(model, timings=timings, **kw)
        torch.cuda.synchronize()
        timings["total"] = time.perf_counter() - t
        runs.append(timings)
    # device time of the launches alone, and the un-instrumented wall time
    L.PROFILE, L.PROFILE_NAMES = [], {"mli_mc_count", "mli_mc_emit", "mli_sdf"}
    extract_mesh(model, **kw)
    torch.cuda.synchronize()
    dev = {}
    for name, e0, e1 in L.PROFILE:
        dev[name] = dev.get(name, 0.0) + e0.elapsed_time(e1) * 1e-3
    calls = sum(1 for name, _, _ in L.PROFILE if name == "mli_mc_count")
    L.PROFILE = L.PROFILE_NAMES = None
    torch.cuda.synchronize()
    t = time.perf_counter()
    extract_mesh(model, **kw)
    torch.cuda.synchronize()
    plain = time.perf_counter() - t
    n = args.resolution + 1
    blocks_side = -(-args.resolution // args.block_res)
    side = [min(args.block_res, args.resolution - b * args.block_res) + 1 for b in range(blocks_side)]
    points = int(sum(a * b * c for a in side for b in side for c in side))   # shared planes counted twice
    mc_dev = dev.get("mli_mc_count", 0.0) + dev.get("mli_mc_emit", 0.0)
    best = min(runs, key=lambda r: r["total"])
    return dict(what="extract_mesh", device=torch.cuda.get_device_name(0), log2T=args.log2T,
                resolution=args.resolution, lattice=[n, n, n], block_res=args.block_res, blocks=calls,
                lattice_points_evaluated=points, vertices=int(mesh.verts.shape[0]), faces=int(mesh.faces.shape[0]),
                attributes=list(kw["attributes"]), runs=runs, best=best, wall_seconds_uninstrumented=plain,
                device_seconds=dev, mc_passes=MC_PASSES, mc_bytes_required=MC_PASSES * 4 * points,
                mc_bytes_per_second=MC_PASSES * 4 * points / mc_dev if mc_dev else None,
                sdf_points_per_second=points / dev["mli_sdf:sdf"] if dev.get("mli_sdf:sdf") else None)


def _timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def lcc_record(args, model, kw):
    """extract_mesh with and without keep_lcc in turn (the same process, the same warm state), the
    components phase split into labelling / stats / compaction on the unfiltered mesh, the device
    time of its launches, and scipy's connected_components on the host for scale."""
    from mli_nerf_amd import _lib as L
    from mli_nerf_amd.mesh import Mesh, cc_max_rounds, connected_components, extract_mesh, filter_components
    extract_mesh(model, keep_lcc=True, **kw)   # warm-up: allocations, first launches
    runs = {False: [], True: []}
    for _ in range(args.repeats):
        for flag in (False, True):
            timings = {}
            mesh, dt = _timed(lambda: extract_mesh(model, timings=timings, keep_lcc=flag, **kw))
            timings["total"] = dt
            runs[flag].append(timings)
            if flag:
                kept = (int(mesh.verts.shape[0]), int(mesh.faces.shape[0]))
    best = {flag: min(r, key=lambda t: t["total"]) for flag, r in runs.items()}
    full = extract_mesh(model, **dict(kw, attributes=()))
    bare = Mesh(full.verts, full.faces, keys=full.keys, face_keys=full.face_keys)
    splits = []
    for _ in range(args.repeats):
        split = {}
        filter_components(bare, timings=split)
        splits.append(split)
    split = min(splits, key=lambda s: sum(s.values()))
    L.PROFILE, L.PROFILE_NAMES = [], set(L.MESH_CC_ENTRY_POINTS)
    cc = connected_components(full.faces, full.verts.shape[0], full.verts)
    torch.cuda.synchronize()
    dev = {}
    for name, e0, e1 in L.PROFILE:
        dev[name] = dev.get(name, 0.0) + e0.elapsed_time(e1) * 1e-3
    L.PROFILE = L.PROFILE_NAMES = None
    host = None
    try:
        import numpy as np
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components as scipy_cc
        t = time.perf_counter()
        f = full.faces.cpu().numpy()
        rows, cols = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]), np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
        n_host, _ = scipy_cc(coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)),
                                        shape=(full.verts.shape[0],) * 2), directed=False)
        host = dict(seconds=time.perf_counter() - t, components=int(n_host),
                    note="scipy.sparse.csgraph.connected_components on the host, the copy of the faces included; "
                         "labels only, no areas; for scale")
    except ImportError:
        pass
    n = args.resolution + 1
    comp = best[True].get("components", 0.0)
    return dict(what="extract_mesh(keep_lcc=True)", device=torch.cuda.get_device_name(0), log2T=args.log2T,
                resolution=args.resolution, lattice=[n, n, n], block_res=args.block_res,
                vertices=int(full.verts.shape[0]), faces=int(full.faces.shape[0]), components=int(cc.ids.numel()),
                vertices_kept=kept[0], faces_kept=kept[1], rounds=cc.rounds,
                max_rounds=cc_max_rounds(int(full.verts.shape[0])),
                runs_plain=runs[False], runs_keep_lcc=runs[True], best_plain=best[False], best_keep_lcc=best[True],
                components_seconds=comp, components_share_of_total=comp / best[True]["total"],
                components_split_seconds=split, device_seconds=dev, host_scipy=host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--block_res", type=int, default=128)
    ap.add_argument("--log2T", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--keep_lcc", action="store_true", help="profile the connected-component filter")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rec = oracle_record(args.log2T) if args.oracle else gpu_record(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
