"""Per-kernel times of the generator at the reference notebook's configuration (x2, NB 4, G 8, 24 x 24 patches; ESRGAN.ipynb:L758-761) and at G 8 / 48 x 48.

--ab: the LDS-resident dense-block kernel (dense_block_lds<bf16,g8>) against the path it replaces, in one process on the same weights and the same 7056 patches:
mask FUSED_ALL and mask FUSED_ALL & ~FUSED_TWO_UP (the cell-packed tile kernels) alternated A/B/A/B, device-synchronised wall time per forward -> per-mask
median and min-max, the per-kernel table of one profiled forward each, and max |difference| of the two outputs, written to --out (profiles/dense_block_g8_ab.json)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.getcwd(), "super-resolution-images-for-3d-printing-defect-detection_amd")); sys.path.insert(0, os.getcwd())
import numpy as np, torch
from sr355 import Model, Context
from sr355.weights import init_weights, bf16_rounded, condition_attention


def kernel_table(ctx, m, x):
    ctx.profile_begin()
    m.forward(x)
    torch.cuda.synchronize()
    agg = {}
    for r in ctx.profile_end():
        a = agg.setdefault(r["kernel"], [0, 0.0, 0.0, 0.0]); a[0] += r.get("launches", 1); a[1] += r["total_ms"]; a[2] += r.get("flops", 0.0); a[3] += r.get("bytes", 0.0)
    return agg


def print_table(title, agg):
    print(f"--- {title}: {sum(a[1] for a in agg.values()):.2f} ms in profiled kernels")
    for k, a in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{k:50s} n={a[0]:4d} {a[1]:8.3f} ms  {a[2] / max(a[1], 1e-9) / 1e9:8.1f} TFLOP/s  {a[3] / max(a[1], 1e-9) / 1e6:8.1f} GB/s")


def build(ctx, scale, nb, g, p, n):
    m = Model("esrgan_g", compute_dtype="bf16", scale_factor=scale, num_blocks=nb, growth_channels=g, use_attention=True, ctx=ctx)
    m.set_weights(bf16_rounded(condition_attention(init_weights(m.layer_shapes(), seed=1))))
    x = ctx.to_device(np.random.default_rng(0).uniform(-1, 1, (n, p, p, 3)).astype(np.float32), torch.bfloat16)
    return m, x


def shapes(ctx):
    for scale, nb, g, p, n in ((2, 4, 8, 24, 7056), (4, 23, 8, 48, 1764)):
        m, x = build(ctx, scale, nb, g, p, n)
        for _ in range(2):
            m.forward(x)
        torch.cuda.synchronize()
        print_table(f"x{scale} NB{nb} G{g} {p}x{p} x {n}", kernel_table(ctx, m, x))
        m.release_workspace()


def ab(ctx, out, reps, warmup):
    m, x = build(ctx, 2, 4, 8, 24, 7056)
    masks = {"FUSED_ALL": ctx.FUSED_ALL, "FUSED_ALL&~FUSED_TWO_UP": ctx.FUSED_ALL & ~ctx.FUSED_TWO_UP}
    times = {k: [] for k in masks}
    ys = {}
    try:
        for i in range(warmup + reps):
            for k, mask in masks.items():                                    # A / B / A / B: both masks see the same drift
                ctx.set_fused(mask, 0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                y = m.forward(x)
                torch.cuda.synchronize()
                if i >= warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                ys[k] = y
        tables = {}
        for k, mask in masks.items():
            ctx.set_fused(mask, 0)
            tables[k] = kernel_table(ctx, m, x)
            print_table(k, tables[k])
    finally:
        ctx.set_fused(ctx.FUSED_ALL, 0)
    a, b = (ys[k].float() for k in masks)
    res = {"shape": [7056, 24, 24, 3], "scale": 2, "num_blocks": 4, "growth_channels": 8, "attention": True, "dtype": "bf16", "timed_forwards_per_mask": reps, "warmup_per_mask": warmup,
           "order": "alternated A/B/A/B in one process, same weights and inputs, device-synchronised wall time per forward",
           "max_abs_output_difference": float((a - b).abs().max()), "output_abs_max": float(a.abs().max()), "masks": {}}
    for k in masks:
        t = sorted(times[k])
        res["masks"][k] = {"mask": int(masks[k]), "ms": [round(v, 4) for v in times[k]], "median_ms": round(float(np.median(t)), 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                           "kernels": [{"kernel": n, "launches": v[0], "total_ms": round(v[1], 4), "tflops": round(v[2] / max(v[1], 1e-9) / 1e9, 2),
                                        "gb_per_s": round(v[3] / max(v[1], 1e-9) / 1e6, 1)} for n, v in sorted(tables[k].items(), key=lambda kv: -kv[1][1])]}
    fa, tl = res["masks"]["FUSED_ALL"], res["masks"]["FUSED_ALL&~FUSED_TWO_UP"]
    spread = max(fa["max_ms"] - fa["min_ms"], tl["max_ms"] - tl["min_ms"])
    res["median_gain_ms"] = round(tl["median_ms"] - fa["median_ms"], 4)
    res["largest_min_max_spread_ms"] = round(spread, 4)
    res["gain_exceeds_spread"] = bool(res["median_gain_ms"] > spread)
    print(json.dumps({k: v for k, v in res.items() if k != "masks"}))
    for k in masks:
        print(k, {q: res["masks"][k][q] for q in ("median_ms", "min_ms", "max_ms")})
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--out", default="profiles/dense_block_g8_ab.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least five timed forwards per mask")
    c = Context.get(0)
    ab(c, a.out, a.reps, a.warmup) if a.ab else shapes(c)
