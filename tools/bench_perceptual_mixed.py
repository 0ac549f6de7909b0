"""What ESRGAN's VGG19 perceptual term in bf16 mixed precision (ESRGANTrainer(perceptual_dtype="bf16")) costs per train_step against the fp32
branch, where the step's time goes in both modes, and what each VGG19 layer costs per launch on the three conv routes.  One process, one GPU.

    python tools/bench_perceptual_mixed.py [steps=20] [runs=3] [batches=16,64] [parts=sections,layers,aba] [configs=notebook,cfg3] [outdir=profiles]

Configurations: `notebook` -- x2, 4 RRDBs, G = 8, LR patches of 24 x 24, train_dtype="bf16", dense_block_impl="lds"; `cfg3` -- x4, 23 RRDBs, G = 32, LR patches of
24 x 24, train_dtype="bf16"; both with the device discriminator and streamed attention.  A = perceptual_dtype "f32" (the parent's path), B = "bf16"; both trainers
start from the same weights and see the same batch.

sections  HIP events around the four parts of train_step (the generator forward; the three critic passes and the discriminator update; _content_terms; the
          loss read, the generator backward and its update), batch 16, mean of `steps` steps after a warm-up -> <outdir>/perceptual_mixed_sections.json
layers    VGG19's sixteen convs at B = 32 (forward) and B = 16 (input gradient) at HR 48 and 96: us per launch of sr_conv2d_dev (fp32, the parent's route),
          sr_conv2d_dev_bf16 and sr_conv3x3_small_bf16 on every shape the kernel takes, with what the dispatch rule does with the call; then a sweep of 512 -> 512
          on 6 x 6 and 3 x 3 images over the pixel count of the call; weights prepacked on every route; 20 launches between two HIP events, median of three
aba       a leg's figure is the median over `runs` runs of the HIP-event time of `steps` train_steps / steps, after a warm-up of two steps on a fresh trainer;
          a row runs A, B, A; the peak of torch's allocator over each leg, above what was allocated when the leg began -> <outdir>/perceptual_mixed_aba.txt
Prints text rows, then one JSON line.
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
from sr355 import gan_train as GT
from sr355.weights import condition_attention, init_weights

arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
steps, runs = int(arg(1, 20)), int(arg(2, 3))
batches = [int(s) for s in arg(3, "16,64").split(",")]
parts, configs = arg(4, "sections,layers,aba").split(","), arg(5, "notebook,cfg3").split(",")
outdir = arg(6, os.path.join(ROOT, "profiles"))
CONFIGS = {"notebook": dict(scale=2, nb=4, g=8, kw=dict(train_dtype="bf16", dense_block_impl="lds")),
           "cfg3": dict(scale=4, nb=23, g=32, kw=dict(train_dtype="bf16"))}
ctx = Context.get(0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def weights(cfg):
    """sr355.bench_rows.cfg3_train_step's recipe."""
    gw = condition_attention(init_weights(M.esrgan_g_layers(cfg["scale"], cfg["g"], cfg["nb"]), seed=3000))
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


def make(cfg, W, batch, perceptual_dtype):
    gw, dw, vw = W
    tr = GT.ESRGANTrainer(ctx, gw, dw, vw, cfg["scale"], cfg["nb"], attention=True, discriminator="device", attention_impl="streamed",
                          perceptual_dtype=perceptual_dtype, **cfg["kw"])
    rng = np.random.default_rng(42 + 3)
    lr = ctx.to_device(rng.uniform(-1, 1, (batch, 24, 24, 3)).astype(np.float32))
    hr = ctx.to_device(rng.uniform(-1, 1, (batch, 24 * cfg["scale"], 24 * cfg["scale"], 3)).astype(np.float32))
    for _ in range(2):
        out = tr.train_step(lr, hr)
    assert all(np.isfinite(v) for v in out.values()), out
    return tr, lr, hr


# ---------------------------------------------------------------------------------------------------------------- where the step goes
def sections(name, cfg, W, batch, perceptual_dtype):
    tr, lr, hr = make(cfg, W, batch, perceptual_dtype)
    marks = []
    mark = lambda: (marks.append(torch.cuda.Event(enable_timing=True)), marks[-1].record())
    forward, content = GT.generator_forward, tr._content_terms

    def timed_forward(*a, **k):
        y = forward(*a, **k)
        mark()
        return y

    def timed_content(*a, **k):
        mark()
        out = content(*a, **k)
        mark()
        return out
    GT.generator_forward, tr._content_terms = timed_forward, timed_content
    try:
        torch.cuda.synchronize()
        for _ in range(steps):
            mark()
            tr.train_step(lr, hr)
            mark()
        torch.cuda.synchronize()
    finally:
        GT.generator_forward = forward
    assert len(marks) == 5 * steps
    t = np.array([[marks[5 * s + i].elapsed_time(marks[5 * s + i + 1]) for i in range(4)] for s in range(steps)]).mean(axis=0)
    row = {"config": name, "batch": batch, "perceptual_dtype": perceptual_dtype, "generator_forward_ms": t[0], "critics_and_d_update_ms": t[1], "content_terms_ms": t[2],
           "read_g_backward_update_ms": t[3], "step_ms": float(t.sum())}
    say(f"{name:8s} batch {batch:3d} perceptual {perceptual_dtype:4s}  G forward {t[0]:8.3f}  critics + D update {t[1]:8.3f}  _content_terms {t[2]:8.3f}  "
        f"read + G backward + update {t[3]:8.3f}  sum {t.sum():8.3f} ms")
    del tr
    torch.cuda.empty_cache()
    return {k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in row.items()}


# ---------------------------------------------------------------------------------------------------------------- per layer
def timed_us(fn):
    fn()
    return 1e3 * float(np.median([event_ms(lambda: [fn() for _ in range(20)]) / 20 for _ in range(3)]))


def conv_row(label, B, h, w, ci, co, rot):
    """One call shape on the three routes; the small-image kernel is timed wherever it TAKES the shape (Context.small_conv_takes), and the row says whether the
    dispatch rule (gan_train.small_conv_wins) gives it the call."""
    k = torch.randn((3, 3, co, ci) if rot else (3, 3, ci, co), device=ctx.torch_device) * float(np.sqrt(2.0 / (9 * ci)))
    bias = None if rot else torch.zeros((co,), device=ctx.torch_device)
    act = "linear" if rot else "relu"
    x32 = torch.relu(torch.randn((B, h, w, ci), device=ctx.torch_device))
    x16 = x32.to(torch.bfloat16)
    ctx.conv_prepack(ctx.pack_list([(k, bias, rot)]))
    ctx.conv_prepack_bf16(ctx.pack_list([(k, bias, rot)]))
    row = {"label": label, "pass": "dgrad" if rot else "fwd", "B": B, "h": h, "w": w, "pixels": B * h * w, "cin": ci, "cout": co,
           "f32_us": timed_us(lambda: ctx.conv2d_dev(x32, k, bias, co, rot=rot, act=act)),
           "bf16_us": timed_us(lambda: ctx.conv2d_dev_bf16(x16, k, bias, co, rot=rot, act=act)), "small_us": None,
           "rule_gives_it_to_small": bool(GT.small_conv_wins(h, w, ci, co, B))}
    if ctx.small_conv_takes(h, w, ci, co):
        handle = ctx.conv3x3_small_pack(k, rot=rot)
        row["small_us"] = timed_us(lambda: ctx.conv3x3_small_bf16(x16, None, bias, co, rot=rot, act=act, packed=handle))
    ctx.conv_prepack(None)
    ctx.conv_prepack_bf16(None)
    gf = 2.0 * 9 * ci * co * B * h * w / 1e3
    sm = "      --" if row["small_us"] is None else f"{row['small_us']:8.1f}"
    tail = "" if row["small_us"] is None else (f"   ({gf / row['small_us'] / 1e3:6.1f} TFLOP/s; small / best other {row['small_us'] / min(row['f32_us'], row['bf16_us']):.2f}; "
                                               f"rule: {'small' if row['rule_gives_it_to_small'] else 'conv2d'})")
    say(f"{label:16s} {row['pass']:5s} B {B:3d} {h:2d} x {w:2d} ({B * h * w:5d} px) {ci:3d} -> {co:3d}   fp32 {row['f32_us']:8.1f}   bf16 {row['bf16_us']:8.1f}   small {sm} us{tail}")
    return row


def layer_rows(hr):
    rows = []
    for name, h, w, cin, cout, _, _, _ in GT.perceptual_routes(hr, hr)[1:]:                 # (the RGB entry has one route)
        rows.append(conv_row(f"HR {hr} {name}", 32, h, w, cin, cout, False))
        rows.append(conv_row(f"HR {hr} {name}", 16, h, w, cout, cin, True))
    return rows


def crossover_rows():
    """512 -> 512 on 3 x 3 and 6 x 6 images over the pixel count of the call: where the small-image kernel stops winning."""
    rows = []
    for h, counts in ((6, (8, 12, 16, 18, 20, 24, 28, 32, 64)), (3, (16, 32, 64, 96, 128, 256))):
        for B in counts:
            rows.append(conv_row(f"sweep {h} x {h}", B, h, h, 512, 512, False))
            rows.append(conv_row(f"sweep {h} x {h}", B, h, h, 512, 512, True))
    return rows


# ---------------------------------------------------------------------------------------------------------------- the step, A / B / A
def leg(cfg, W, batch, perceptual_dtype):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    tr, lr, hr = make(cfg, W, batch, perceptual_dtype)
    times = [event_ms(lambda: [tr.train_step(lr, hr) for _ in range(steps)]) / steps for _ in range(runs)]
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    del tr
    torch.cuda.empty_cache()
    return times, peak


def aba(name, cfg, W, batch):
    legs = [leg(cfg, W, batch, d) for d in ("f32", "bf16", "f32")]
    (a1, b, a2), peaks = [float(np.median(t)) for t, _ in legs], [p for _, p in legs]
    mean_a = 0.5 * (a1 + a2)
    below = max(legs[1][0]) < min(legs[0][0] + legs[2][0])
    row = {"config": name, "batch": batch, "A1_ms": a1, "B_ms": b, "A2_ms": a2, "A1_runs": legs[0][0], "B_runs": legs[1][0], "A2_runs": legs[2][0],
           "ratio_B_over_A": b / mean_a, "aa_spread": abs(a1 - a2) / mean_a, "every_B_run_below_every_A_run": bool(below), "peak_MiB": peaks}
    say(f"{name:8s} batch {batch:3d}  A = fp32 branch  B = bf16 branch   A1 {a1:9.3f}  B {b:9.3f}  A2 {a2:9.3f} ms/step   B/A {row['ratio_B_over_A']:.3f}   "
        f"A/A spread {100 * row['aa_spread']:.1f} %   {'every B run below every A run' if below else 'NOT every B run below every A run'}   "
        f"peak rise A1 {peaks[0]:.0f}  B {peaks[1]:.0f}  A2 {peaks[2]:.0f} MiB")
    say(f"         runs  A1 {[round(t, 3) for t in legs[0][0]]}  B {[round(t, 3) for t in legs[1][0]]}  A2 {[round(t, 3) for t in legs[2][0]]}")
    return row


say(f"device {torch.cuda.get_device_name(0)}; {steps} train_steps per run, median of {runs} runs after a warm-up, HIP-event timed; device discriminator, streamed attention")
result = {"tool": "bench_perceptual_mixed", "steps": steps, "runs": runs}
Ws = {c: weights(CONFIGS[c]) for c in configs}
if "sections" in parts:
    say("")
    say("sections of train_step, batch 16, ms (mean of the steps of one run after a warm-up)")
    result["sections"] = [sections(c, CONFIGS[c], Ws[c], 16, d) for c in configs for d in ("f32", "bf16")]
    with open(os.path.join(outdir, "perceptual_mixed_sections.json"), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "steps": steps, "rows": result["sections"]}, fh, indent=1)
if "layers" in parts:
    say("")
    say("per launch, us: VGG19's convs at B = 32 (forward) and B = 16 (input gradient), then 512 -> 512 on 6 x 6 and 3 x 3 images over the pixel count; weights prepacked "
        "on every route; 20 launches between two HIP events, median of three; small = sr_conv3x3_small_bf16, timed on every shape it takes")
    result["layers"] = [r for hr in (48, 96) for r in layer_rows(hr)]
    result["crossover"] = crossover_rows()
if "aba" in parts:
    say("")
    say("train_step, A / B / A, ms per step; A = perceptual_dtype f32, B = bf16")
    result["aba"] = [aba(c, CONFIGS[c], Ws[c], b) for c in configs for b in batches]
if parts:
    with open(os.path.join(outdir, "perceptual_mixed_aba.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
print(json.dumps(result))
