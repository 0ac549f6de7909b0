"""FineTunedVGG16's training step with and without fine_tune_base, at batch 32 of 128 x 128 (f32 model), from the repository root:

    python tools/probe_vgg_finetune.py [--out profiles/vgg_finetune_step.json] [--no-trace]

  1. ms per training step for head-only, train_last_n_layers = 4 and = 6: the three interleaved in one process on the same batch,
     device-synchronised wall time per step, medians of --reps (7) after --warmup (2), with min-max.
  2. the weight gradient of one block5 layer (B = 32, 8 x 8, 512 -> 512) by sr_conv2d_wgrad and by sr_conv2d_wgrad_maps on the same tensors,
     alternated in the same process, --launches (20) back-to-back launches per sample, medians of 7 after 2 with min-max, and the rule the
     packed kernel is kept by: the medians must differ by more than the larger min-max spread.
  3. the n = 4 step's per-kernel times from `rocprofv3 --kernel-trace --stats`, in child processes of their own under `timeout`: one child runs
     2 steps and one 7, and a kernel's per-step time is the difference of its totals over 5 (set-up, packing and warm-up cancel).
"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.join(os.getcwd(), "super-resolution-images-for-3d-printing-defect-detection_amd")); sys.path.insert(0, os.getcwd())
import numpy as np

B, HW = 32, 128


def make_step(ctx, n_last):
    """-> a closure that runs one training step on a fixed batch: n_last None = head-only (today's fit), else fine_tune_base with that tail."""
    import torch
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    from sr355.train import DeviceAdam, ParamBucket
    from sr355.vgg_train import VGGFineTuner
    m = FineTunedVGG16(compute_dtype="f32")
    m.setup_model(input_shape=(HW, HW, 3), train_last_n_layers=n_last or 4, fine_tune_base=n_last is not None)
    rng = np.random.default_rng(0)
    x = ctx.to_device(rng.uniform(0, 1, (B, HW, HW, 3)).astype(np.float32))
    y = ctx.to_device(rng.integers(0, 2, B).astype(np.int32))
    k0, k1 = ctx.to_device((rng.random((B, 512)) < 0.8).astype(np.uint8)), ctx.to_device((rng.random((B, 256)) < 0.8).astype(np.uint8))
    stats, work = ctx.empty((3,), torch.float64), ctx.dense_head_workspace(B, 2)
    if n_last is None:
        bucket = ParamBucket(ctx, {n: m.weights[n] for n in ("dense", "predictions")})
        opt, grads = DeviceAdam(ctx, bucket.flat, 1e-3, epsilon=1e-7), torch.empty_like(bucket.flat)

        def step():
            ctx.dense_head_step(m._gap_device(x), y, bucket.flat, 2, stats, work, grads, k0, k1, 1.25, 0.0)
            opt.apply(bucket.flat, grads)
        return step
    convs = m._tail_convs()
    tr = VGGFineTuner(ctx, m.weights, convs, 1e-3)
    return lambda: tr.step(m._prefix_device(x, convs[0]), y, stats, work, k0, k1, 1.25, 0.0)


def summary(ms):
    s = sorted(ms)
    return {"ms": [round(v, 4) for v in ms], "median_ms": round(float(np.median(s)), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def interleaved(fns, reps, warmup, inner=1):
    """{name: closure} -> {name: [ms per call]}: the closures alternated A/B/C/A/B/C, `inner` back-to-back calls per sample."""
    import torch
    times = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3 / inner)
    return times


def steps(ctx, reps, warmup):
    fns = {"head_only": make_step(ctx, None), "n4": make_step(ctx, 4), "n6": make_step(ctx, 6)}
    return {k: summary(v) for k, v in interleaved(fns, reps, warmup).items()}


def wgrad_ab(ctx, reps, warmup, launches):
    rng = np.random.default_rng(1)
    x, dy = ctx.to_device(rng.normal(size=(B, 8, 8, 512)).astype(np.float32)), ctx.to_device(rng.normal(size=(B, 8, 8, 512)).astype(np.float32))
    out = (ctx.empty((3, 3, 512, 512)), ctx.empty((512,)))
    fns = {"sr_conv2d_wgrad": lambda: ctx.conv2d_wgrad(x, dy, 3, out=out), "sr_conv2d_wgrad_maps": lambda: ctx.conv2d_wgrad_maps(x, dy, out=out)}
    res = {k: summary(v) for k, v in interleaved(fns, reps, warmup, launches).items()}
    a, b = res["sr_conv2d_wgrad"], res["sr_conv2d_wgrad_maps"]
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    res.update(shape=[B, 8, 8, 512, 512], launches_per_sample=launches, median_gain_ms=round(a["median_ms"] - b["median_ms"], 4),
               largest_min_max_spread_ms=round(spread, 4), keep_packed_kernel=bool(a["median_ms"] - b["median_ms"] > spread))
    return res


def traced_kernels(limit):
    """Two children under rocprofv3 (2 and 7 steps of the n = 4 step) -> [{kernel, launches_per_step, us_per_step}] by the difference of the two."""
    tot = {}
    for nsteps in (2, 7):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
                   sys.executable, os.path.abspath(__file__), "--child-steps", str(nsteps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"rocprofv3 child ({nsteps} steps) ended with {r.returncode}: {r.stderr[-400:]}")
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise RuntimeError("rocprofv3 wrote no kernel statistics")
            tot[nsteps] = {row["Name"]: (int(row["Calls"]), int(row["TotalDurationNs"])) for f in files for row in csv.DictReader(open(f))}
    rows = []
    for name, (c7, t7) in tot[7].items():
        c2, t2 = tot[2].get(name, (0, 0))
        if c7 > c2:
            rows.append({"kernel": name[:160], "launches_per_step": round((c7 - c2) / 5.0, 2), "us_per_step": round((t7 - t2) / 5.0 / 1e3, 2)})
    return sorted(rows, key=lambda r: -r["us_per_step"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/vgg_finetune_step.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-limit", type=int, default=240, help="seconds each rocprofv3 child may run")
    ap.add_argument("--child-steps", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    from sr355 import Context
    c = Context.get(0)
    if a.child_steps:                                          # the traced child: nothing but the steps
        fn = make_step(c, 4)
        for _ in range(a.child_steps):
            fn()
        torch.cuda.synchronize()
        sys.exit(0)
    res = {"batch": B, "input": [HW, HW, 3], "dtype": "f32", "timed_per_mode": a.reps, "warmup_per_mode": a.warmup,
           "order": "interleaved in one process, same batch, device-synchronised wall time",
           "step_ms": steps(c, a.reps, a.warmup), "wgrad_ab": wgrad_ab(c, a.reps, a.warmup, a.launches)}
    print(json.dumps({k: {q: v[q] for q in ("median_ms", "min_ms", "max_ms")} for k, v in res["step_ms"].items()}))
    print(json.dumps({k: v for k, v in res["wgrad_ab"].items() if not isinstance(v, dict)}),
          {k: v["median_ms"] for k, v in res["wgrad_ab"].items() if isinstance(v, dict)})
    if not a.no_trace:
        res["n4_step_kernels"] = traced_kernels(a.trace_limit)
        for r in res["n4_step_kernels"][:12]:
            print(f"{r['us_per_step']:10.2f} us  x{r['launches_per_step']:<5} {r['kernel'][:110]}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
