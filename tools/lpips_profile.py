"""Time of the LPIPS op (mli_nerf_amd/lpips.py) on device-resident pairs, as JSON records under
profiles/lpips/.  Seeded random weights (tests/lpips_ref.py): the time does not depend on them.

  python tools/lpips_profile.py --out profiles/lpips/lpips_call.json
      wall time (host clock around LPIPS.__call__, ending in the copy of the results to the host) and
      device time (events around mli_lpips) for 1 and 16 pairs of 800 x 800, best of --repeats
  python tools/lpips_profile.py --layers --out profiles/lpips/lpips_layers.json
      starts a child of itself under ``rocprofv3 --kernel-trace`` (a run of its own), reads the trace and
      gives, per kernel of the last call, its time; per convolution layer also its FLOP rate
      (2 * M * Cout * Cin*k*k, the padding of layer 1's K not counted) as a fraction of the 157.3 TF
      f32 matrix peak.  Reported, not asserted.
  python tools/lpips_profile.py --cpu --out profiles/lpips/lpips_ref_cpu_800.json
      tests/lpips_ref.py (torch float64) on one 800 x 800 pair on the CPU, for scale only
  python tools/lpips_profile.py --bench-ab DIR --out profiles/lpips/bench_ab.json
      collects the JSON lines of ``bench.py --gpus 1 --steps 200 --warmup 10`` saved as
      DIR/bench_parent_{1,2,3}.txt and DIR/bench_new_{1,2,3}.txt (the parent commit and this tree, run
      alternately on one GPU: parent 1, new 1, parent 2, ...) into one record
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F32_MATRIX = 157.3e12
SIZE = 800
BATCHES = (1, 16)


def pairs(B, size=SIZE, seed=0):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randint(0, 256, (B, 3, size, size), generator=g, dtype=torch.uint8)
    low = torch.rand(B, 3, size // 4, size // 4, generator=g)
    field = torch.nn.functional.interpolate(low, size=(size, size), mode="nearest")
    tgt = ((0.6 * field + 0.4 * pred.float() / 255) * 255).round().to(torch.uint8)
    return pred, tgt


def _fn():
    import lpips_ref as R
    from mli_nerf_amd import lpips as P
    return P.LPIPS(R.random_weights(3), "cuda:0")


def conv_flops(B, size=SIZE):
    """Per layer: (M, Cout, K, flops) of the implicit GEMM over the 2B images."""
    from mli_nerf_amd import lpips as P
    shapes = P.tap_shapes(size, size)
    out = []
    for (h, w, cout), (cin, _, k, _, _) in zip(shapes[1:], P.LAYERS):
        M, K = 2 * B * h * w, cin * k * k
        out.append(dict(M=M, N=cout, K=K, flops=2 * M * cout * K))
    return out


def call_record(args):
    from mli_nerf_amd import _lib as L
    fn = _fn()
    cases = []
    for B in BATCHES:
        pred, tgt = (t.to("cuda:0") for t in pairs(B))   # resident: no upload in the timing
        v = fn(pred, tgt)   # warm-up
        runs = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = fn(pred, tgt)
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        dev = []
        for _ in range(args.repeats):
            L.PROFILE, L.PROFILE_NAMES = [], {"mli_lpips"}
            fn(pred, tgt)
            torch.cuda.synchronize()
            dev.append(sum(e0.elapsed_time(e1) for _, e0, e1 in L.PROFILE) * 1e-3)
            L.PROFILE = L.PROFILE_NAMES = None
        flops = sum(l["flops"] for l in conv_flops(B))
        cases.append(dict(what="%d pair(s) of %d x %d, uint8" % (B, SIZE, SIZE), B=B, wall_runs=runs, wall_best=min(runs),
                          device_runs=dev, device_best=min(dev), conv_flops=flops,
                          conv_flops_over_device_time_of_peak=flops / min(dev) / PEAK_F32_MATRIX,
                          lpips=[float(x) for x in v[:2]]))
    return dict(what="LPIPS.__call__ on device-resident pairs; device time: events around mli_lpips (13 launches)",
                device=torch.cuda.get_device_name(0), cases=cases)


def child(B):
    """What the traced run does: a warm-up call and two more."""
    fn = _fn()
    pred, tgt = (t.to("cuda:0") for t in pairs(B))
    for _ in range(3):
        fn(pred, tgt)
    torch.cuda.synchronize()


def layers_record(args):
    cases = []
    for B in BATCHES:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--child", str(B)]
            subprocess.run(cmd, check=True, timeout=args.timeout, stdout=subprocess.DEVNULL)
            found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
            if len(found) != 1:
                raise RuntimeError("expected one kernel trace under %s, found %s" % (tmp, found))
            rows = [r for r in csv.DictReader(open(found[0])) if "lpips_" in r["Kernel_Name"]
                    and "pack" not in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        per_call = 13   # 5 convolutions, 2 pools, 5 distances, 1 reduce
        if len(rows) != 3 * per_call:
            raise RuntimeError("expected %d lpips kernels in the trace, found %d" % (3 * per_call, len(rows)))
        last = rows[-per_call:]
        kernels, convs = [], []
        for r in last:
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            name = re.search(r"lpips_\w+", r["Kernel_Name"]).group(0)
            kernels.append(dict(kernel=name, us=us))
            if "conv" in name:
                convs.append(us)
        layers = []
        for i, (us, g) in enumerate(zip(convs, conv_flops(B))):
            layers.append(dict(layer=i + 1, us=us, tflops=g["flops"] / us / 1e6,
                               of_f32_matrix_peak=g["flops"] / (us * 1e-6) / PEAK_F32_MATRIX, **g))
        span = (int(last[-1]["End_Timestamp"]) - int(last[0]["Start_Timestamp"])) / 1e3
        cases.append(dict(B=B, size=[SIZE, SIZE], kernels=kernels, conv_layers=layers, span_us=span,
                          kernel_sum_us=sum(k["us"] for k in kernels)))
    return dict(what="kernel times of the last of three LPIPS calls, rocprofv3 --kernel-trace; rates reported, "
                     "not asserted", peak_f32_matrix_flops=PEAK_F32_MATRIX, cases=cases)


def cpu_record(args):
    import lpips_ref as R
    w = R.random_weights(3)
    pred, tgt = pairs(1)
    runs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        v = R.lpips(pred, tgt, w)
        runs.append(time.perf_counter() - t0)
    return dict(what="CPU tests/lpips_ref.py (torch float64) on one 800x800 pair", runs=runs, best=min(runs),
                lpips=float(v["lpips"][0]), threads=torch.get_num_threads(), note="for scale only")


def bench_record(args):
    rec = dict(what="bench.py --gpus 1 --steps 200 --warmup 10, the parent commit and this tree alternating on one GPU",
               order="parent 1, new 1, parent 2, new 2, parent 3, new 3")
    for side in ("parent", "new"):
        runs = []
        for i in (1, 2, 3):
            with open(os.path.join(args.bench_ab, "bench_%s_%d.txt" % (side, i))) as f:
                line = [l for l in f.read().splitlines() if l.startswith("{")][-1]
            r = json.loads(line)
            runs.append({k: r.get(k) for k in ("ms_per_step", "value", "unit", "steps", "warmup", "n_gpus")})
        rec[side] = runs
    ms = {side: [r["ms_per_step"] for r in rec[side]] for side in ("parent", "new")}
    rec["parent_spread_ms"] = [min(ms["parent"]), max(ms["parent"])]
    rec["new_spread_ms"] = [min(ms["new"]), max(ms["new"])]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--bench-ab", metavar="DIR", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if not args.out:
        ap.error("--out is needed")
    rec = (bench_record(args) if args.bench_ab else cpu_record(args) if args.cpu else layers_record(args) if args.layers
           else call_record(args))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
