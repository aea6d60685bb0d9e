"""Wall time of the pseudo-label step (mli_nerf_amd/pseudo_label.py) on one synthetic camera,
split by phase, as one JSON record.

  python tools/labels_profile.py --out profiles/labels/cam512_L8_K3.json
  python tools/labels_profile.py --size 800 --lights 40 --out profiles/labels/cam800_L40_K3.json
  python tools/labels_profile.py --kdtree --size 128 --out profiles/labels/kdtree_cpu_128.json   (CPU, for scale)

The camera: size x size pixels, L lights, blob-shaped visibility common to the lights up to a
per-light shift (so that about 40 % of the pixels are lit by no light after the erosion: the
holes), the ``pair`` setting (K = 3, every pixel without a lit light is a hole).  Phases (host
wall clock with a device synchronisation after each, pseudo_label._Clock): morphology (erosion,
certainty, shading), kmeans, best_ref, fill (index lists, features, search, reduce); best of
``--repeats`` runs per phase.  The fill's launches are also timed with device events
(_lib.PROFILE): pair evaluations per second = holes * donors / that time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flops_per_pair(K):
    """VALU operations per (hole, donor) pair: 14 for the base (5 sub, 5 mul, 4 add), 6 per colour pair
    (2 sub, 2 mul, add, min), the final add and the compare."""
    return 14 + 6 * K * K + 2


def camera(size, lights, seed=0):
    """One camera's results_all entry ([1,C,H,W] CPU tensors) with `rgb_target`."""
    g = torch.Generator().manual_seed(seed)
    cells = max(size // 64, 3)

    def field(n):
        low = torch.rand(n, 1, cells, cells, generator=g)
        return torch.nn.functional.interpolate(low, size=(size, size), mode="bicubic", align_corners=True)
    common, own = field(1), field(lights)
    vis = ((0.8 * common + 0.2 * own) > 0.47).float()
    nxl = (0.1 + 0.85 * field(lights)).clamp(0, 1)
    normal = torch.nn.functional.normalize(field(3).view(1, 3, size, size) - 0.5, dim=1)
    albedo = 0.2 + 0.6 * field(3).view(1, 3, size, size).clamp(0, 1)
    tint = 0.7 + 0.3 * torch.rand(lights, 3, 1, 1, generator=g)
    img = (albedo * tint * (0.3 + 0.7 * nxl) + 0.02 * torch.rand(lights, 3, size, size, generator=g)).clamp(0, 1)
    ones = torch.ones(1, 1, size, size)
    return {str(l): {"normal": normal, "normal_x_light": nxl[l][None], "rgb_render": img[l][None],
                     "rgb_target": img[l][None], "visibility": vis[l][None], "inter_mask": ones}
            for l in range(lights)}


def gpu_record(args):
    from mli_nerf_amd import _lib as L
    from mli_nerf_amd import pseudo_label as P
    lights = camera(args.size, args.lights)
    dev = "cuda:0"
    lights = {k: {n: t.to(dev) for n, t in d.items()} for k, d in lights.items()}   # resident: no upload in the phases
    K = P.SETTINGS[args.setting]["kmeans_num_clusters"]
    P.camera_labels(lights, args.setting, device=dev)   # warm-up
    runs = []
    for _ in range(args.repeats):
        timings = {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        filled, cert, psg, avg = P.camera_labels(lights, args.setting, device=dev, timings=timings)
        torch.cuda.synchronize()
        timings["total"] = time.perf_counter() - t
        runs.append(timings)
    best = {k: min(r[k] for r in runs) for k in runs[0]}
    L.PROFILE, L.PROFILE_NAMES = [], set(L.LABELS_ENTRY_POINTS)
    P.camera_labels(lights, args.setting, device=dev)
    torch.cuda.synchronize()
    device_seconds = {}
    for name, e0, e1 in L.PROFILE:
        device_seconds[name] = device_seconds.get(name, 0.0) + e0.elapsed_time(e1) * 1e-3
    L.PROFILE = L.PROFILE_NAMES = None
    donors = int((psg > 0).any(dim=0).sum())
    holes = args.size * args.size - donors
    pairs = holes * donors
    fill_dev = device_seconds.get("mli_label_fill", 0.0)
    return dict(what="pseudo labels of one camera", device=torch.cuda.get_device_name(0), setting=args.setting,
                size=[args.size, args.size], lights=args.lights, K=K, holes=holes, donors=donors,
                hole_fraction=holes / float(args.size * args.size), runs=runs, best=best,
                device_seconds=device_seconds, pair_evaluations=pairs,
                pair_evaluations_per_second=pairs / fill_dev if fill_dev else None,
                fill_valu_flops_per_second=pairs * flops_per_pair(K) / fill_dev if fill_dev else None,
                finite=bool(torch.isfinite(filled).all()))


def kdtree_record(args):
    """scipy's KD-tree on the same fill at a smaller size, as fill_holes_kd queries it: the K
    copies of the donors in one tree, K queries per hole.  For scale only."""
    from scipy.spatial import KDTree
    rng = np.random.default_rng(0)
    n = args.size * args.size
    K = 3
    base = rng.random((n, 5))
    colour = rng.random((K, n, 2))
    donor = rng.random(n) < 0.6
    tree_pts = np.concatenate([np.concatenate([base[donor], colour[j][donor]], axis=1) for j in range(K)])
    t = time.perf_counter()
    tree = KDTree(tree_pts)
    best = None
    for i in range(K):
        d, _ = tree.query(np.concatenate([base[~donor], colour[i][~donor]], axis=1))
        best = d if best is None else np.minimum(best, d)
    dt = time.perf_counter() - t
    return dict(what="CPU scipy KD-tree fill (7-D, K copies of the donors, K queries per hole)", size=[args.size] * 2,
                K=K, holes=int((~donor).sum()), donors=int(donor.sum()), seconds=dt,
                note="for scale only: random features, one CPU thread, a smaller image than the GPU record")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--lights", type=int, default=8)
    ap.add_argument("--setting", default="pair")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kdtree", action="store_true")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rec = kdtree_record(args) if args.kdtree else gpu_record(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
