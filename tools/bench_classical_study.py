"""The classical study's main loop at the dataset's size: N = 219 synthetic RGB pairs of 478 x 478 / 239 x 239 (sr355.synth).

Measures
  * the wall time of sr355.study.classical_study (first call and a warm second call, one chunk of N);
  * the device time of each new kernel (sr_rgb2gray_u8, sr_freq_to_u8, sr_ssim_map) on the whole batch, by HIP events, and its achieved
    bytes/s (algorithmic bytes: inputs read once per pass, outputs written once) against the ~6.3 TB/s copy rate DESIGN.md measured;
  * the wall time of the per-image route over the same pairs: the body of tests/test_classic_metrics_gpu.py::test_notebook_loop
    (tests/classical_study_ref.py: per_image_route, both of the notebook's passes of every algorithm), which is made only of entry points
    the batched study leaves untouched.  With --parent DIR (a checkout of the parent commit with its library built) that route runs on
    the parent's build, before and after the study (A-B-A); without it, on this build.
Every step is a process of its own with its own time limit and at most 16 CPU threads.  Prints one JSON object.

python tools/bench_classical_study.py [--pairs 219] [--sizes 478,239] [--parent DIR] [--step-timeout 900] [--out FILE]"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "super-resolution-images-for-3d-printing-defect-detection_amd"
COPY_RATE_BYTES_PER_S = 6.3e12          # HBM3E 8 TB/s spec, ~6.3 TB/s measured copy


def _paths(tree):
    """This tool's tests/ (for classical_study_ref and metrics_ref) behind the package and root of `tree` (this checkout or the parent's)."""
    sys.path[:0] = [tree, os.path.join(tree, PKG_NAME), os.path.join(ROOT, "tests")]


def make_pairs_u8(n, H, h, seed=0):
    """uint8 RGB pairs [n,H,H,3] / [n,h,h,3] from sr355.synth (H = scale * h)."""
    import numpy as np
    from sr355.synth import make_pairs
    lr_f, hr_f = make_pairs(n, h, h, H // h, seed=seed)
    return (hr_f * 255).astype(np.uint8), (lr_f * 255).astype(np.uint8)


def device_ms(fn, min_window_s=0.3):
    """Mean device time of fn() over a window of at least min_window_s (after one warm-up call), by HIP events."""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    reps = max(3, min(100, math.ceil(min_window_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def step_per_image(args):
    _paths(args.tree)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import classical_study_ref as SR
    import sr355
    H, h = args.H, args.h
    hr, lr = make_pairs_u8(args.pairs, H, h)
    SR.per_image_route(hr[:1], lr[:1], profile=True)                       # warm-up: arenas, DFT operators, tap tables
    torch.cuda.synchronize()
    t = time.perf_counter()
    stats, _ = SR.per_image_route(hr, lr, profile=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    build = "this build" if os.path.samefile(os.path.dirname(os.path.dirname(sr355.__file__)), os.path.join(ROOT, PKG_NAME)) else "parent commit"
    return {"step": "per_image", "build": build, "pairs": args.pairs, "wall_s": wall, "wall_s_per_pair": wall / args.pairs,
            "psnr_mean_bicubic": float(sum(stats["psnr"]["bicubic"]) / args.pairs)}


def step_study(args):
    _paths(ROOT)
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from sr355 import Context
    from sr355.study import classical_study
    ctx = Context.get(0)
    H, h, N = args.H, args.h, args.pairs
    hr, lr = make_pairs_u8(N, H, h)
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = classical_study(hr, lr)
        walls.append(time.perf_counter() - t)
    out = {"step": "study", "build": "this build", "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "pairs": N,
           "wall_s_first": walls[0], "wall_s_warm": walls[1], "wall_s_per_pair_warm": walls[1] / N,
           "psnr_mean_bicubic": float(np.mean(res["stats"]["psnr"]["bicubic"])),
           "device_time_s_per_image": {a: float(res["stats"]["time"][a][0]) for a in res["stats"]["time"]},
           "device_bytes_per_image": {a: float(res["stats"]["memory"][a][0]) for a in res["stats"]["memory"]}, "kernels": []}
    dhr, dlr = ctx.to_device(hr), ctx.to_device(lr)
    hr_g, lr_g = ctx.rgb2gray(dhr), ctx.rgb2gray(dlr)
    freq = ctx.freq_extrapolate(lr_g, H, H)
    sr_g = ctx.freq_to_u8(freq)[0]
    sr_f = ctx.non_local_means(lr_g, H, H)
    sr_rgb = ctx.resize(dlr, H, H, "INTER_CUBIC")
    px = float(N) * H * H
    cases = (("sr_rgb2gray_u8", lambda: ctx.rgb2gray(dhr), px * 4),                                 # 3 bytes in, 1 out
             ("sr_freq_to_u8", lambda: ctx.freq_to_u8(freq), px * 17),                               # fp64 read by the max pass and again by the scaling pass, 1 out
             ("sr_ssim_map u8/u8 gray", lambda: ctx.ssim_map(hr_g, sr_g), px * 10),                   # 1 + 1 in, fp64 out
             ("sr_ssim_map u8/f32 gray", lambda: ctx.ssim_map(hr_g, sr_f), px * 13),
             ("sr_ssim_map u8/u8 RGB", lambda: ctx.ssim_map(dhr, sr_rgb), px * 30))
    for name, fn, nbytes in cases:
        ms, reps = device_ms(fn)
        rate = nbytes / (ms * 1e-3)
        out["kernels"].append({"kernel": name, "B": N, "device_ms": ms, "reps": reps, "algorithmic_bytes": nbytes, "bytes_per_s": rate,
                               "fraction_of_copy_rate": rate / COPY_RATE_BYTES_PER_S})
    out["clock_mhz_under_mfma_load"] = ctx.measure_clock_mhz()
    return out


def run_step(step, args, tree):
    """One step as a process of its own, under its own time limit; its last line is its JSON."""
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k, "16") or 16)))
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--tree", tree, "--pairs", str(args.pairs), "--sizes", args.sizes]
    t = time.perf_counter()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, env=env)
    except subprocess.TimeoutExpired:
        return {"step": step, "error": f"time limit of {args.step_timeout} s"}, False
    if r.returncode != 0:
        return {"step": step, "error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-1500:]}, False
    row = json.loads(r.stdout.strip().splitlines()[-1])
    row["process_s"] = time.perf_counter() - t
    return row, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=219)
    ap.add_argument("--sizes", default="478,239")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the per-image route runs there")
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=("per_image", "study"), help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.H, args.h = (int(v) for v in args.sizes.split(","))
    if args.step:
        print(json.dumps({"per_image": step_per_image, "study": step_study}[args.step](args)), flush=True)
        return
    tree = os.path.abspath(args.parent) if args.parent else ROOT
    res = {"shape": {"H": args.H, "W": args.H, "h": args.h, "w": args.h, "pairs": args.pairs},
           "per_image_route_build": "parent commit" if args.parent else "this build (the route's entry points are untouched by the batched study)",
           "copy_rate_bytes_per_s": COPY_RATE_BYTES_PER_S, "steps": []}
    for step, where in (("per_image", tree), ("study", ROOT), ("per_image", tree)):          # A-B-A
        row, ok = run_step(step, args, where)
        res["steps"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        if not ok:                                                                           # a failed step ends the run: nothing more starts on the GPU
            break
    done = [r for r in res["steps"] if "error" not in r]
    per = [r["wall_s"] for r in done if r["step"] == "per_image"]
    study = [r for r in done if r["step"] == "study"]
    if per and study:
        res["per_image_wall_s"] = per
        res["study_wall_s_warm"] = study[0]["wall_s_warm"]
        res["study_wall_s_first"] = study[0]["wall_s_first"]
        res["per_image_over_study_warm"] = (sum(per) / len(per)) / study[0]["wall_s_warm"]
        res["per_image_over_study_first"] = (sum(per) / len(per)) / study[0]["wall_s_first"]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if len(done) != 3:
        sys.exit(1)


if __name__ == "__main__":
    main()
