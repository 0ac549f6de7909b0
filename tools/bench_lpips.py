"""Device time of LPIPS (Context.lpips, csrc/lpips.hip) on the dataset's 478 x 478 uint8 pairs for B = 1 and B = 32 with seeded weights,
beside the fp32 torch-CPU restatement's time per pair on the host (tests/lpips_ref.py in float32: the stand-in for the reference's CPU
LPIPS), and the cost of the new column: MetricsAggregator.collect_arrays at B = 32 (64 levels, one angle: its defaults) with and without
weights loaded, wall clock around a synchronised call.  HIP-event timed: two warm-up calls, then the median of the repeats; the whole run
stops at --time-limit seconds.  Prints one JSON object.

python tools/bench_lpips.py [--size 478] [--batches 1,32] [--reps 11] [--time-limit 300] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd")]
import numpy as np
import torch

from bench_eda import device_ms, pairs


def wall_ms(fn, reps):
    fn(); fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter(); fn(); torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=478)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--time-limit", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps: the median of at least ten")
    signal.alarm(args.time_limit)                      # the default action ends the process
    H = W = args.size
    import lpips_ref as R
    import data.eda_methods as E
    from sr355 import Context
    from sr355 import lpips as LP
    ctx = Context.get(0)
    batches = [int(b) for b in args.batches.split(",")]
    lr, hr = pairs(np.random.default_rng(0), max(batches), H, W)
    weights = LP.seeded_weights(7)
    res = {"shape": {"H": H, "W": W}, "weights": "seeded_weights(7)", "host_cpus": len(os.sched_getaffinity(0)), "torch_threads": torch.get_num_threads(), "rows": []}

    def cpu_ms(fn, reps=3):
        fn()
        out = []
        for _ in range(reps):
            t = time.perf_counter(); fn(); out.append((time.perf_counter() - t) * 1e3)
        return statistics.median(out)

    res["torch_cpu_fp32_ms_per_pair"] = cpu_ms(lambda: R.lpips_u8(lr[:1], hr[:1], weights, torch.float32))
    print(json.dumps({"torch_cpu_fp32_ms_per_pair": res["torch_cpu_fp32_ms_per_pair"]}), flush=True)
    try:
        ctx.lpips_set_weights(weights)
        for B in batches:
            dl, dh = ctx.to_device(lr[:B]), ctx.to_device(hr[:B])
            med, lo, hi = device_ms(lambda: ctx.lpips(dl, dh), args.reps)
            row = {"part": "lpips", "B": B, "device_ms_per_pair": med / B, "min_ms_per_pair": lo / B, "max_ms_per_pair": hi / B, "pairs_per_s": 1e3 * B / med,
                   "reps": args.reps}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del dl, dh
        res["mem_info"] = ctx.mem_info()
    finally:
        ctx.lpips_set_weights(None)

    # the cost of the column: collect_arrays on device-resident stacks, unloaded and loaded
    B = max(batches)
    dl, dh = ctx.to_device(lr[:B]), ctx.to_device(hr[:B])
    with tempfile.TemporaryDirectory() as d:
        alex, lins = LP.to_state_dicts(weights)
        p = os.path.join(d, "lpips_seeded.npz")
        np.savez(p, **alex, **lins)
        for label in ("unloaded", "loaded", "unloaded again"):
            if label == "loaded":
                E.ImageDatasetAnalyzer.load_lpips(p)
            else:
                E.ImageDatasetAnalyzer.unload_lpips()
            try:
                med, lo, hi = wall_ms(lambda: E.MetricsAggregator.collect_arrays(dl, dh), args.reps)
            finally:
                E.ImageDatasetAnalyzer.unload_lpips()
            row = {"part": f"collect_arrays, {label}", "B": B, "wall_ms_per_pair": med / B, "min_ms_per_pair": lo / B, "max_ms_per_pair": hi / B, "reps": args.reps}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
