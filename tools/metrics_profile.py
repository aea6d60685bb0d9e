"""Wall time of the image-metric op (mli_nerf_amd/metrics.py) on device-resident pairs, as one
JSON record.

  python tools/metrics_profile.py --out profiles/metrics/image_metrics.json
  python tools/metrics_profile.py --cpu --out profiles/metrics/metrics_ref_cpu_800.json   (CPU, for scale)

Cases: one 800 x 800 RGB pair, a batch of 100 such pairs, one 512 x 512 RGB pair; uint8 inputs (the
PNG path) and fp32 maps with ``quantize`` (the ``evaluate`` path).  Host wall clock around
``image_metrics`` (allocation of its scratch, the two launches, the copy of the results to the
host) with a device synchronisation after each call, best of ``--repeats``; the two launches alone
are also timed with device events (_lib.PROFILE).  ``--cpu``: tests/metrics_ref.py (scipy float64)
on one 800 x 800 pair, for scale only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = (("one 800x800 RGB pair", 1, 800), ("100 800x800 RGB pairs", 100, 800), ("one 512x512 RGB pair", 1, 512))


def pairs(B, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randint(0, 256, (B, 3, size, size), generator=g, dtype=torch.uint8)
    low = torch.rand(B, 3, size // 4, size // 4, generator=g)
    field = torch.nn.functional.interpolate(low, size=(size, size), mode="nearest")
    tgt = ((0.6 * field + 0.4 * pred.float() / 255) * 255).round().to(torch.uint8)
    return pred, tgt


def gpu_record(args):
    from mli_nerf_amd import _lib as L
    from mli_nerf_amd import metrics as M
    dev = "cuda:0"
    cases = []
    for what, B, size in CASES:
        pred, tgt = (t.to(dev) for t in pairs(B, size))   # resident: no upload in the timing
        for dtype in ("uint8", "float32+quantize"):
            p, t = (pred, tgt) if dtype == "uint8" else (pred.float() / 255, tgt.float() / 255)
            m = M.image_metrics(p, t)   # warm-up
            runs = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = M.image_metrics(p, t)
                torch.cuda.synchronize()
                runs.append(time.perf_counter() - t0)
            L.PROFILE, L.PROFILE_NAMES = [], set(L.METRICS_ENTRY_POINTS)
            M.image_metrics(p, t)
            torch.cuda.synchronize()
            device_seconds = sum(e0.elapsed_time(e1) for _, e0, e1 in L.PROFILE) * 1e-3
            L.PROFILE = L.PROFILE_NAMES = None
            tiles = B * 3 * (-(-size // L.METRICS_TILE[0])) * (-(-size // L.METRICS_TILE[1]))
            cases.append(dict(what=what, dtype=dtype, B=B, size=[size, size], tiles=tiles, runs=runs, best=min(runs),
                              launches_device_seconds=device_seconds, tiles_per_second=tiles / device_seconds,
                              ssim=float(m["ssim"][0]), psnr=float(m["psnr"][0])))
    return dict(what="image_metrics on device-resident pairs", device=torch.cuda.get_device_name(0), cases=cases)


def cpu_record(args):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import metrics_ref as R
    pred, tgt = (t.numpy() for t in pairs(1, 800))
    R.metrics(pred, tgt)
    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        m = R.metrics(pred, tgt)
        runs.append(time.perf_counter() - t0)
    return dict(what="CPU tests/metrics_ref.py (numpy float64, scipy uniform_filter) on one 800x800 RGB pair",
                runs=runs, best=min(runs), ssim=float(m["ssim"][0]), psnr=float(m["psnr"][0]),
                threads=torch.get_num_threads(), numpy=np.__version__, note="for scale only")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rec = cpu_record(args) if args.cpu else gpu_record(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
