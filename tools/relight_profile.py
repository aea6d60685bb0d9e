"""One view under L lights: ``Model.inference_lights`` (the geometry computed once)
against L calls of ``Model.inference``, as one JSON record.

  python tools/relight_profile.py --out profiles/relight/view800.json

Workload: one 800 x 800 view, full-size hash table (log2T 22), 64 + 4 x 16 samples, light visibility
on (blend_z_sphere_tracing, the pseudo-label configuration), synthetic weights; stage b
(syn_hotdog_b, three heads) and stage a (syn_hotdog_a, one head); L in 1, 2, 4, 8.

Method: within one process the two paths alternate, ``--repeats`` times each per L after a warm-up
of both.  Per call: host wall clock around the call with a device synchronisation before and after,
and the device time between two events on the calling stream (the call's side streams are joined
to it before it returns).  The best and the median of each are kept, and the baseline's spread
(max - min over its repeats, relative to its median) stands beside every ratio.  With the chunk
pipeline off, the visibility launches are timed by event pairs (_lib.PROFILE): the baseline's L x
mli_light_visibility, and the shared path's mli_camera_hit and mli_light_shadows; the baseline's
light half is its total minus L x the camera half (the same kernel on the same inputs).  Before any
timing the two paths' maps are compared at the timed size: they must be bit-identical.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VIS = {"enabled": True, "camera_ray_type": "blend_z_sphere_tracing", "type": "sphere_tracing",
       "visibility_bounding_type": "sphere", "visibility_sphere_radius": 0.95}
VIS_OPS = ("mli_light_visibility", "mli_camera_hit", "mli_light_shadows")


def light_poses(n):
    from mli_nerf_amd import synthetic
    out = []
    for k in range(n):
        c2w = torch.eye(4) * torch.tensor([1.0, -1.0, -1.0, 1.0])
        c2w[:3, 3] = torch.tensor(synthetic.light_positions()[k], dtype=torch.float32)
        out.append(synthetic.invert_pose(c2w[:3]))
    return torch.stack(out)


def build(config, size, dev):
    from mli_nerf_amd import synthetic
    from mli_nerf_amd.configs import preset
    from mli_nerf_amd.model import Model
    over = {"data": {"train": {"image_size": [size, size]}, "val": {"image_size": [size, size]}},
            "model": {"light_visibility": VIS}}
    cfg = preset(config, overrides=over)
    model = Model(cfg.model, cfg.data)
    model.load_state_dict(synthetic.make_state_dict(log2T=22, seed=0,
                                                    heads="rgb" if model.stage == "a" else "rgb_r_s"))
    model = model.to(dev)
    model.neural_sdf.set_active_levels(sys.maxsize)   # as test_all_light: iteration sys.maxsize
    model.neural_sdf.set_normal_epsilon()
    model.progress = 1.0
    data = {k: v.to(dev) for k, v in synthetic.make_batch(1, H=size, W=size, frame=5).items()}
    return model, data


def timed(fn, dev):
    """(host wall seconds, device seconds between events on the calling stream, result)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, e0.elapsed_time(e1) * 1e-3, out


def summary(runs):
    return dict(runs=runs, best=min(runs), median=statistics.median(runs),
                spread=(max(runs) - min(runs)) / statistics.median(runs))


def vis_launch_seconds(fn, dev):
    """Device seconds of the visibility launches of ``fn()`` by op, from event pairs."""
    from mli_nerf_amd import _lib as L
    L.PROFILE, L.PROFILE_NAMES = [], set(VIS_OPS)
    try:
        fn()
        torch.cuda.synchronize(dev)
        out = {}
        for name, e0, e1 in L.PROFILE:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1) * 1e-3
            out[name + ":calls"] = out.get(name + ":calls", 0) + 1
        return out
    finally:
        L.PROFILE = L.PROFILE_NAMES = None


def record_stage(config, args, dev):
    model, data = build(config, args.size, dev)
    cases = []
    for n in args.lights:
        lights = light_poses(n).to(dev)
        loop = lambda: [model.inference({**data, "pose_light": lights[l:l + 1]}) for l in range(n)]  # noqa: E731
        shared = lambda: model.inference_lights(data, lights)  # noqa: E731
        # warm-up of both paths at this shape, and the outputs compared at the timed size
        a, b = loop(), shared()
        torch.cuda.synchronize(dev)
        same = all(set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))
        if not same:
            raise RuntimeError("%s L=%d: inference_lights differs from inference per light" % (config, n))
        visible = float(torch.stack([x["visibility_map"][x["inter_mask_map"] > 0.5].mean() for x in a]).mean())
        del a, b
        base_wall, base_dev, new_wall, new_dev = [], [], [], []
        for _ in range(args.repeats):   # alternating
            w, d, _ = timed(loop, dev)
            base_wall.append(w)
            base_dev.append(d)
            w, d, _ = timed(shared, dev)
            new_wall.append(w)
            new_dev.append(d)
        model.pipeline_chunks = False
        try:
            loop(), shared()   # warm-up of the unpipelined schedule
            k_base, k_new = vis_launch_seconds(loop, dev), vis_launch_seconds(shared, dev)
        finally:
            model.pipeline_chunks = True
        cam = k_new["mli_camera_hit"]
        rec = dict(L=n, bit_identical=True, visible_fraction_of_hits=visible,
                   loop_wall=summary(base_wall), loop_device=summary(base_dev),
                   shared_wall=summary(new_wall), shared_device=summary(new_dev),
                   speedup_wall_median=statistics.median(base_wall) / statistics.median(new_wall),
                   speedup_device_median=statistics.median(base_dev) / statistics.median(new_dev),
                   visibility_launches=dict(
                       loop=k_base, shared=k_new, loop_light_half=k_base["mli_light_visibility"] - n * cam,
                       shared_light_shadows=k_new["mli_light_shadows"],
                       light_half_speedup=(k_base["mli_light_visibility"] - n * cam) / k_new["mli_light_shadows"]))
        print(json.dumps({k: rec[k] for k in ("L", "speedup_wall_median", "speedup_device_median")}), flush=True)
        cases.append(rec)
    return dict(config=config, stage=model.stage, heads=len(model.engine.head_specs), size=[args.size, args.size],
                samples=model.pcfg.n_samples, chunk_rays=model.rand_rays_val, log2T=22, cases=cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lights", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--configs", nargs="+", default=["syn_hotdog_b", "syn_hotdog_a"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relight_profile: needs the GPU (no time is reported from a CPU run)")
    dev = torch.device("cuda:0")
    rec = dict(what="one view under L lights: L x Model.inference (loop) against Model.inference_lights (shared)",
               device=torch.cuda.get_device_name(0), repeats=args.repeats,
               stages=[record_stage(c, args, dev) for c in args.configs])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
