"""Device time of the dataset synthesis (data/common_methods.py::degrade_batch; sr_degrade_gauss / _motion / _noise / _jpeg and sr_resize)
on the reference's frames, 478 x 478 -> 239 x 239: images per second of degrade_batch end to end (decisions drawn on the host, upload not
counted: the frames are on the device), each stage alone with every image's flag on, and the NumPy restatement (tests/degrade_ref.py +
the oracle's resize, one process on the host's CPUs) on one image as the CPU stand-in.  HIP-event timed: two warm-up calls, then the
median of the repeats; the whole run stops at --time-limit seconds.  Prints one JSON object.

python tools/bench_degrade.py [--size 478] [--batch 64] [--reps 7] [--time-limit 240] [--out FILE]"""
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


def frames(rng, n, H, W):
    from sr355.synth import hr_tile
    return np.stack([np.ascontiguousarray((hr_tile(rng, H, W) * 255.0).astype(np.uint8)[..., ::-1]) for _ in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=478)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--time-limit", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    signal.alarm(args.time_limit)                      # the default action ends the process
    H = W = args.size
    B = args.batch
    import degrade_ref as R
    from data import common_methods as M
    from sr355 import Context
    ctx = Context.get(0)
    hr = frames(np.random.default_rng(0), B, H, W)
    w, h = M.lr_size((H, W, 3), 0.5)
    res = {"shape": {"H": H, "W": W, "h": h, "w": w}, "B": B, "host_cpus": len(os.sched_getaffinity(0)), "reps": args.reps, "rows": []}

    # the CPU stand-in: every stage on, one image
    rec = {"gauss_ksize": 5, "gauss_sigma": 1.4, "motion_size": 7, "interp_code": 2, "interp_name": "INTER_CUBIC", "lr_size": (w, h), "noise_std": 6.0,
           "noise": np.random.default_rng(1).normal(0, 6.0, (h, w, 3)).astype(np.float32), "jpeg_quality": 40}
    stages_cpu = {"gauss": lambda: R.gaussian_blur(hr[0], R.gauss_taps(5, 1.4)), "motion": lambda: R.motion_blur(hr[0], 7),
                  "noise": lambda: R.noise_apply(hr[0, :h, :w], rec["noise"]), "jpeg": lambda: R.jpeg_roundtrip(hr[0, :h, :w], 40),
                  "all_stages_with_resize": lambda: R.degrade_with_record(hr[0], rec)}
    cpu = {}
    for k, fn in stages_cpu.items():
        fn()
        ts = []
        for _ in range(3):
            t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
        cpu[k] = statistics.median(ts)
    res["numpy_cpu_ms_per_image"] = cpu
    print(json.dumps({"numpy_cpu_ms_per_image": cpu}), flush=True)

    x = ctx.to_device(hr)
    lr0 = ctx.resize(x, h, w, "INTER_CUBIC")
    params = ctx.to_device(ctx.degrade_params([rec] * B))
    stages = (("gauss k5, HR", lambda: ctx.degrade_gauss(x, params, check=False)), ("motion 7, HR", lambda: ctx.degrade_motion(x, params, check=False)),
              ("resize INTER_CUBIC", lambda: ctx.resize(x, h, w, "INTER_CUBIC")), ("resize INTER_AREA", lambda: ctx.resize(x, h, w, "INTER_AREA")),
              ("noise (Philox), LR", lambda: ctx.degrade_noise(lr0, params, seed=1, check=False)), ("jpeg q40, LR", lambda: ctx.degrade_jpeg(lr0, params, check=False)))
    for name, fn in stages:
        med, lo, hi = device_ms(fn, args.reps)
        row = {"stage": name, "device_ms_per_image": med / B, "min_ms_per_image": lo / B, "max_ms_per_image": hi / B}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    ctx.degrade_status()
    ctx.profile_begin()
    ctx.degrade_jpeg(lr0, params, check=False)
    res["jpeg_kernels_ms_per_image"] = {p["kernel"]: p["total_ms"] / B for p in ctx.profile_end()}

    # end to end: degrade_batch with its own draws (about 70 / 30 / 70 / 70 % of the stages on), wall clock including the host's share
    med, lo, hi = device_ms(lambda: M.degrade_batch(x, 0.5, seed=3), args.reps)
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter(); M.degrade_batch(x, 0.5, seed=3); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    res["degrade_batch"] = {"device_ms_per_image": med / B, "min_ms_per_image": lo / B, "max_ms_per_image": hi / B,
                            "images_per_s_event_timed": B / (med * 1e-3), "images_per_s_wall": B / statistics.median(ts)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
