"""Device time of the dataset EDA's per-pair statistics and global accumulators (sr_eda_pair_stats + sr_eda_accumulate; data/EDA.ipynb's
MetricsAggregator.collect without LPIPS and file reading) on the dataset's 478 x 478 pairs with the notebook's settings (256 levels,
four angles), for B = 1 and B = 32, beside the NumPy restatement's CPU time per pair (tests/eda_ref.py, one process on the host's
CPUs; warm-up, then the median of 3, per part).  HIP-event timed: warm-up, then the median of the repeats; the whole run stops at --time-limit seconds.  Prints one JSON object.

python tools/bench_eda.py [--size 478] [--batches 1,32] [--reps 7] [--time-limit 240] [--out FILE]"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd")]
import numpy as np
import torch


def device_ms(fn, reps):
    """Median device time of fn() over `reps` event-timed calls after two warm-up calls."""
    fn(); fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def pairs(rng, n, H, W):
    from sr355.synth import hr_tile
    hr = np.stack([np.ascontiguousarray((hr_tile(rng, H, W) * 255.0).astype(np.uint8)[..., ::-1]) for _ in range(n)])
    pad = np.pad(hr.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    blur = sum(pad[:, i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    lr = np.clip(blur + rng.normal(0, 4, hr.shape), 0, 255).astype(np.uint8)
    return lr, hr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=478)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--time-limit", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    signal.alarm(args.time_limit)                      # the default action ends the process
    H = W = args.size
    import eda_ref as R
    from sr355 import Context
    ctx = Context.get(0)
    batches = [int(b) for b in args.batches.split(",")]
    lr, hr = pairs(np.random.default_rng(0), max(batches), H, W)
    res = {"shape": {"H": H, "W": W}, "glcm_levels": 256, "angles": 4, "host_cpus": len(os.sched_getaffinity(0)), "rows": []}
    def cpu_ms(fn, reps=3):
        fn()                                            # warm-up, as for the device
        out = []
        for _ in range(reps):
            t = time.perf_counter(); fn(); out.append((time.perf_counter() - t) * 1e3)
        return statistics.median(out)

    res["numpy_cpu_ms_per_pair"] = {"pair_stats": cpu_ms(lambda: R.pair_stats(lr[0], hr[0], 256, (0, 1, 2, 3))),
                                    "accumulate": cpu_ms(lambda: R.accumulate(lr[:1], hr[:1])), "reps": 3}
    print(json.dumps({"numpy_cpu_ms_per_pair": res["numpy_cpu_ms_per_pair"]}), flush=True)
    for B in batches:
        dl, dh = ctx.to_device(lr[:B]), ctx.to_device(hr[:B])
        acc = ctx.eda_accumulate(dl, dh)
        for what, fn in (("pair_stats", lambda: ctx.eda_pair_stats(dl, dh, 256, (0, 1, 2, 3))), ("accumulate", lambda: ctx.eda_accumulate(dl, dh, acc))):
            med, lo, hi = device_ms(fn, args.reps)
            row = {"part": what, "B": B, "device_ms_per_pair": med / B, "min_ms_per_pair": lo / B, "max_ms_per_pair": hi / B, "reps": args.reps}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        ctx.eda_pair_stats(dl, dh, 256, (0, 1, 2, 3))
        torch.cuda.synchronize()
        ctx.profile_begin()
        ctx.eda_pair_stats(dl, dh, 256, (0, 1, 2, 3))
        prof = {p["kernel"]: p["total_ms"] / B for p in ctx.profile_end()}
        res["rows"].append({"part": "pair_stats phases, ms per pair", "B": B, **prof})
        print(json.dumps(res["rows"][-1]), flush=True)
        del dl, dh, acc
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
