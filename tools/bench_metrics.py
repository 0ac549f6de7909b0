"""Device time of the classical study's nine image-quality scores (sr_classic_scores; profiling_methods.py:45-167 and skimage's PSNR /
SSIM) on the dataset's 478 x 478 pairs, RGB (the interpolation rows) and gray (the advanced rows), for B = 1 (the notebook's per-call
use) and B = 219 (its image count), beside the NumPy restatement's CPU time per pair (tests/metrics_ref.py, B = 1).  Also the DFT
part's achieved fp64 rate (4 h w^2 + 8 h^2 w FLOP per image, two images per pair, the DFT GEMMs timed alone) and the whole study on the
device: 219 pairs x 8 algorithms up-scaled (478 / 239) and scored, in ms.  Prints one JSON object.

python tools/bench_metrics.py [--size 478] [--batches 1,219] [--study-pairs 219] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd")]
import numpy as np
import torch


def device_ms(fn, min_window_s=0.5):
    """Mean device time of fn() over a window of at least min_window_s (after one warm-up call), by HIP events."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    reps = max(3, min(500, math.ceil(min_window_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def cpu_ms(fn):
    t = time.perf_counter(); fn(); return (time.perf_counter() - t) * 1e3


def dft_flops(h, w):
    """fp64 FLOP of one image's DFT: the real x complex product (4 h w^2) and the complex x complex product (8 h^2 w)."""
    return 4.0 * h * w * w + 8.0 * h * h * w


def pairs(rng, n, H, W):
    from sr355.synth import hr_tile
    hr = np.stack([np.clip(hr_tile(rng, H, W) * 255.0 + rng.normal(0, 5, (H, W, 3)), 0, 255).astype(np.uint8) for _ in range(n)])
    sr = np.clip(hr.astype(np.float64) + rng.normal(0, 8, hr.shape), 0, 255).astype(np.uint8)
    return hr, sr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=478)
    ap.add_argument("--batches", default="1,219")
    ap.add_argument("--study-pairs", type=int, default=219)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H = W = args.size
    import metrics_ref as MR
    from sr355 import Context
    ctx = Context.get(0)
    rng = np.random.default_rng(0)
    nmax = max(int(b) for b in args.batches.split(","))
    hr, sr = pairs(rng, nmax, H, W)
    res = {"shape": {"H": H, "W": W}, "clock_mhz_under_mfma_load": ctx.measure_clock_mhz(), "rows": []}
    cpu = {"rgb": cpu_ms(lambda: MR.scores(hr[0], sr[0])), "gray": cpu_ms(lambda: MR.scores(hr[0, ..., 1], sr[0, ..., 1]))}
    for B in (int(b) for b in args.batches.split(",")):
        for kind in ("rgb", "gray"):
            xh = ctx.to_device(hr[:B] if kind == "rgb" else np.ascontiguousarray(hr[:B, ..., 1]))
            xs = ctx.to_device(sr[:B] if kind == "rgb" else np.ascontiguousarray(sr[:B, ..., 1]))
            ms, reps = device_ms(lambda: ctx.classic_scores(xh, xs))
            row = {"pairs": kind, "B": B, "device_ms_per_pair": ms / B, "reps": reps, "numpy_cpu_ms_per_pair": cpu[kind],
                   "dft_fp64_flop_per_pair": 2 * dft_flops(H, W)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del xh, xs
        torch.cuda.empty_cache()
    # the DFT part alone (the two GEMMs of the hf ratio and their gray planes), HIP-event timed inside the library
    for B in (int(b) for b in args.batches.split(",")):
        xh = ctx.to_device(np.ascontiguousarray(hr[:B, ..., 1]))
        xs = ctx.to_device(np.ascontiguousarray(sr[:B, ..., 1]))
        ctx.classic_scores(xh, xs)
        torch.cuda.synchronize()
        reps = 3 if B > 1 else 50
        ctx.profile_begin()
        for _ in range(reps):
            ctx.classic_scores(xh, xs)
        prof = {p["kernel"]: p for p in ctx.profile_end()}
        d = prof["classic_scores_dft"]
        row = {"part": "dft", "B": B, "ms_per_pair": d["total_ms"] / reps / B, "fp64_flop_per_s": d["flops"] / (d["total_ms"] * 1e-3),
               "stats_pass_ms_per_pair": prof["classic_scores_stats"]["total_ms"] / reps / B}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del xh, xs
    torch.cuda.empty_cache()

    # the study: 219 pairs (478 RGB HR, 239 RGB LR) x 8 algorithms up-scaled on the device and scored in place
    n = args.study_pairs
    hs = ctx.to_device(hr[:n] if n <= nmax else pairs(rng, n, H, W)[0])
    h = H // 2
    ls = ctx.resize(hs, h, h, "INTER_AREA")
    coef = torch.tensor([4899, 9617, 1868], dtype=torch.int32, device=hs.device)

    def gray(x):
        return ((x.to(torch.int32) * coef).sum(-1).add(8192) >> 14).to(torch.uint8).contiguous()

    def study():
        for interp in ("INTER_LINEAR", "INTER_CUBIC", "INTER_AREA", "INTER_LANCZOS4"):
            up = ctx.resize(ls, H, W, interp)
            ctx.classic_scores(hs, up)
        hg, lg = gray(hs), gray(ls)
        outs = [ctx.back_projection(hg, lg, 10), ctx.edge_guided(lg, H, W)]
        f = ctx.freq_extrapolate(lg, H, W)
        outs.append((f / f.reshape(n, -1).amax(1).reshape(n, 1, 1) * 255.0).to(torch.uint8))
        for o in outs:
            ctx.classic_scores(hg, o)
        ctx.classic_scores(hg, ctx.non_local_means(lg, H, W).contiguous(), "hr_span")

    ms, reps = device_ms(study, min_window_s=1.0)
    res["study"] = {"pairs": n, "algorithms": 8, "device_ms": ms, "reps": reps}
    print(json.dumps(res["study"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
