"""What training the notebook's G = 8 trunk on the LDS-resident dense-block kernels (ESRGANTrainer(train_dtype="bf16", dense_block_impl="lds")) costs per
train_step against the fp32 trainer, in A/B/A order in one process on one GPU; the per-launch times of the new kernels beside the time their MFMA count alone
would take; the peak memory rise of each leg.

    python tools/bench_dense_block_train.py [steps=20] [runs=3] [batches=16,64] [out=profiles/esrgan_g8_train_aba.txt]

The notebook's shape: x2, 4 RRDBs, G = 8, both SelfAttention layers (streamed), device discriminator, `batch` LR patches of 24 x 24.  A = the fp32 trainer (at
G = 8 it takes generator_forward's cat path), B = train_dtype "bf16" with dense_block_impl "lds"; both start from the same weights and see the same batch.

A leg's figure is the median over `runs` runs of the HIP-event time of `steps` train_steps / steps, after a warm-up of two steps on a fresh trainer.  A row runs
A, B, A: its ratio is B / mean(A1, A2), its A/A spread |A1 - A2| / mean(A1, A2); a speed-up is claimed only when every B run is below every A run.  The kernel rows are
sr_profile_begin's per-launch HIP-event times over the steps of one B run.  Prints text rows (also written to `out`), then one JSON line.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd")]

import numpy as np
import torch

from oracle import models as M
from sr355 import Context
from sr355.gan_train import ESRGANTrainer
from sr355.weights import condition_attention, init_weights

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
batches = [int(s) for s in (sys.argv[3] if len(sys.argv) > 3 else "16,64").split(",")]
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "esrgan_g8_train_aba.txt")
SCALE, NB, G, P = 2, 4, 8, 24
KERNELS = ("dense_block_pack_dev<g8>", "dense_block_fwd_lds<bf16,g8,nhwc>", "dense_block_bwd_lds<bf16,g8>")
# MFMAs (v_mfma_f32_16x16x32_bf16, 16 cycles each on one of a CU's four SIMDs) per image and block at 24 x 24 = 36 tiles: forward 36 * 9 * (2 + 3 + 3 + 3) growth +
# 4 * 36 * 27 conv5; backward 6 * 36 * 18 conv5's input gradient + 36 * 9 * (6 + 5 + 5 + 4) the growth convs'
MFMAS = {KERNELS[1]: 36 * 9 * 11 + 4 * 36 * 27, KERNELS[2]: 6 * 36 * 18 + 36 * 9 * 20}
CLOCK_HZ = 2.4e9
ctx = Context.get(0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def weights():
    gw = condition_attention(init_weights(M.esrgan_g_layers(SCALE, G, NB), seed=3000))
    gw = {n: ((k * 0.1, b * 0.1) if n.endswith("_conv5") else (k, b)) for n, (k, b) in gw.items()}
    dw = init_weights(M.discriminator_layers(), seed=5000)
    vw = init_weights(M.vgg19_extractor_layers(), scheme="he_normal", seed=6000)
    vw = {n: (k * 0.05 if n == "block1_conv1" else k, b) for n, (k, b) in vw.items()}
    return gw, dw, vw


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def leg(W, batch, lds, profile=False):
    """-> (median ms per step, peak memory rise in MiB over the leg, per-kernel profile of one more run or None)."""
    gw, dw, vw = W
    kw = {"train_dtype": "bf16", "dense_block_impl": "lds"} if lds else {}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    tr = ESRGANTrainer(ctx, gw, dw, vw, SCALE, NB, attention=True, discriminator="device", attention_impl="streamed", **kw)
    rng = np.random.default_rng(42 + 3)
    lr = ctx.to_device(rng.uniform(-1, 1, (batch, P, P, 3)).astype(np.float32))
    hr = ctx.to_device(rng.uniform(-1, 1, (batch, P * SCALE, P * SCALE, 3)).astype(np.float32))
    for _ in range(2):
        out = tr.train_step(lr, hr)
    assert all(np.isfinite(v) for v in out.values()), out
    times = [event_ms(lambda: [tr.train_step(lr, hr) for _ in range(steps)]) / steps for _ in range(runs)]
    rise = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    prof = None
    if profile:
        ctx.profile_begin()
        for _ in range(steps):
            tr.train_step(lr, hr)
        prof = {r["kernel"]: r for r in ctx.profile_end()}
    del tr
    torch.cuda.empty_cache()
    return float(np.median(times)), times, rise, prof


def aba(W, batch):
    a1, t1, m1, _ = leg(W, batch, False)
    bb, tb, mb, prof = leg(W, batch, True, profile=True)
    a2, t2, m2, _ = leg(W, batch, False)
    mean_a = 0.5 * (a1 + a2)
    every = bool(max(tb) < min(t1 + t2))
    row = {"batch": batch, "A1_ms": a1, "B_ms": bb, "A2_ms": a2, "A1_runs": t1, "B_runs": tb, "A2_runs": t2, "ratio_B_over_A": bb / mean_a,
           "aa_spread": abs(a1 - a2) / mean_a, "every_B_run_below_every_A_run": every, "peak_rise_MiB": {"A1": m1, "B": mb, "A2": m2}, "kernels": {}}
    say(f"ESRGAN x2 NB 4 G 8 batch {batch:3d}  A = fp32 trainer  B = bf16 trunk on LDS-resident blocks   A1 {a1:8.3f}  B {bb:8.3f}  A2 {a2:8.3f} ms/step   "
        f"B/A {row['ratio_B_over_A']:.3f}   A/A spread {100 * row['aa_spread']:.1f} %   {'every B run below every A run' if every else 'NOT every B run below every A run'}")
    say(f"    runs  A1 {' '.join(f'{t:.3f}' for t in t1)}   B {' '.join(f'{t:.3f}' for t in tb)}   A2 {' '.join(f'{t:.3f}' for t in t2)}")
    say(f"    peak memory rise of a leg: A1 {m1:.1f} MiB   B {mb:.1f} MiB   A2 {m2:.1f} MiB")
    for k in KERNELS:
        r = prof.get(k)
        if r is None:
            say(f"    {k}: not launched")
            continue
        us = 1e3 * r["total_ms"] / r["launches"]
        row["kernels"][k] = {"launches": r["launches"], "us_per_launch": us}
        text = f"    {k:36s} {r['launches']:5d} launches in {steps} steps  {us:9.1f} us per launch"
        if k in MFMAS:
            waves = -(-batch // ctx.cu_count())                        # images the busiest workgroup runs
            floor = waves * MFMAS[k] / 4 * 16 / CLOCK_HZ * 1e6
            row["kernels"][k]["mfma_only_us"] = floor
            text += f"   its {MFMAS[k]} MFMAs per image alone: {floor:6.1f} us ({waves} image(s) per workgroup)   measured / MFMA-only {us / floor:.1f}"
        say(text)
    return row


say(f"device {torch.cuda.get_device_name(0)}; {steps} train_steps per run, median of {runs} runs after a warm-up, HIP-event timed; device discriminator, streamed attention")
W = weights()
rows = [aba(W, b) for b in batches]
px = lambda b: b * P * P
for b in batches:
    # per block and pixel the fp32 cat path keeps four concat copies (72 + 80 + 88 + 96 channels), four growth outputs (32), conv5's output and the skip sum (64 + 64);
    # the lds path keeps F (96 bf16 channels: the block's output is slice 0 of the next F)
    say(f"trunk tape batch {b}, from the shapes: 12 dense blocks; fp32 cat path {12 * px(b) * (72 + 80 + 88 + 96 + 32 + 64 + 64) * 4 / 2 ** 20:.1f} MiB; "
        f"lds {12 * px(b) * 96 * 2 / 2 ** 20:.1f} MiB of F, and G, the gradient of F, never reaches memory")
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print(json.dumps({"tool": "bench_dense_block_train", "steps": steps, "runs": runs, "rows": rows}))
