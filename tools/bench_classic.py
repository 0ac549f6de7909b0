"""Device time of the classical study's back-projection, NL-means, edge-guided and frequency up-scalers (classic_algorithms.py:23-108)
at the dataset's 478 x 478 / 239 x 239 grayscale pairs, for B = 1 (the notebook's per-call use) and B = 219 (its image count), beside
the NumPy restatement's CPU time per image (tests/classic_ref.py, B = 1).  For NL-means and freq also the kernel's achieved rate
(pixel-shifts/s of sr_nl_means alone; algorithmic fp64 FLOP/s of the two DFT products).  Prints one JSON object.

python tools/bench_classic.py [--sizes 478,239] [--batches 1,219] [--out FILE]"""
import argparse
import ctypes as C
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
    reps = max(3, min(200, math.ceil(min_window_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def cpu_ms(fn):
    t = time.perf_counter(); fn(); return (time.perf_counter() - t) * 1e3


def freq_flops(H, W, h, w):
    """Multiply-adds of the two products as csrc/classic.hip runs them, 2 FLOP each: T = X A_W^T (real x real or real x complex),
    Y = |A_H T| (real / complex operands as their sizes make them)."""
    t_cplx, a_cplx = w % 2 == 0, h % 2 == 0
    p1 = h * W * w * (2 if t_cplx else 1)
    p2 = H * W * h * ((4 if a_cplx else 2) if t_cplx else (2 if a_cplx else 1))
    return 2.0 * (p1 + p2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="478,239")
    ap.add_argument("--batches", default="1,219")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H, h = (int(v) for v in args.sizes.split(","))
    W, w = H, h
    import classic_ref as CR
    from sr355 import Context
    from sr355.synth import hr_tile
    ctx = Context.get(0)
    rng = np.random.default_rng(0)
    nmax = max(int(b) for b in args.batches.split(","))
    hr = np.stack([np.clip(hr_tile(rng, H, W)[:, :, 0] * 255.0 + rng.normal(0, 6, (H, W)), 0, 255).astype(np.uint8) for _ in range(nmax)])
    lr = np.stack([np.asarray(CR.O.cv_resize(im.astype(np.float32)[:, :, None], h, w, CR.O.INTER_AREA))[:, :, 0].astype(np.uint8) for im in hr])
    res = {"shape": {"H": H, "W": W, "h": h, "w": w}, "clock_mhz_under_mfma_load": ctx.measure_clock_mhz(), "rows": []}
    cpu = {
        "ibp": cpu_ms(lambda: CR.back_projection(hr[0], lr[0], 10)),
        "nlm": cpu_ms(lambda: CR.non_local_means((H, W), lr[0])),
        "egi": cpu_ms(lambda: CR.edge_guided(lr[0], H, W)),
        "freq": cpu_ms(lambda: CR.freq_extrapolate(lr[0], H, W)),
    }
    res["numpy_fft_procedure_ms_per_image"] = cpu_ms(lambda: CR.freq_extrapolate_fft(lr[0], H, W))   # the reference's own fft2 route
    for B in (int(b) for b in args.batches.split(",")):
        xh = ctx.to_device(hr[:B], torch.uint8)
        xl = ctx.to_device(lr[:B], torch.uint8)
        sigma = ctx.noise_sigma(xl)
        den = ctx.empty((B, h, w), torch.float32)
        st = ctx.stream()

        def nlm_kernel_only():
            ctx.check(ctx.lib.sr_nl_means(ctx.h, xl.data_ptr(), B, h, w, 5, 6, sigma.data_ptr(), C.c_double(1.15), den.data_ptr(), st))

        runs = {
            "ibp": lambda: ctx.back_projection(xh, xl, 10),
            "nlm": lambda: ctx.non_local_means(xl, H, W),
            "egi": lambda: ctx.edge_guided(xl, H, W),
            "freq": lambda: ctx.freq_extrapolate(xl, H, W),
        }
        for name, fn in runs.items():
            ms, reps = device_ms(fn)
            row = {"algorithm": name, "B": B, "device_ms_per_image": ms / B, "reps": reps, "numpy_cpu_ms_per_image": cpu[name]}
            if name == "nlm":
                kms, _ = device_ms(nlm_kernel_only)
                row["nlm_kernel_ms_per_image"] = kms / B
                row["pixel_shifts_per_s"] = B * h * w * 169 / (kms * 1e-3)
            if name == "freq":
                row["fp64_flop_per_s"] = B * freq_flops(H, W, h, w) / (ms * 1e-3)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        del xh, xl, sigma, den
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
