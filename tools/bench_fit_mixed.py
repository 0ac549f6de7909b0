"""What EDSR's bf16 mixed-precision training (EDSR(update="device", train_dtype="bf16")) costs per step against the fp32 device fit, in A/B/A order in
one process on one GPU, and the bf16 weight-gradient kernel against the fp32 one.

    python tools/bench_fit_mixed.py [steps=20] [fits=3] [scales=2,4] [batches=16,64,256] [out=profiles/edsr_mixed_aba.txt]

EDSR x2 and x4, 16 residual blocks, 64 filters, batches of 24 x 24 patches from a device-resident sr355.patches.PatchPairs (the input path of
profiles/fit_device_aba.txt, whose 3.4 ms per step at x2, batch 16 is what leg A should show).  A = train_dtype "f32", B = "bf16"; both fits start
from the same weights and see the same patches.

A leg's figure is the median over `fits` one-epoch fits (after one warm-up fit) of the HIP-event time of the fit / its training steps; a fit has
`steps` steps and one validation batch.  A row runs A, B, A: its ratio is B / mean(A1, A2), its A/A spread |A1 - A2| / mean(A1, A2); B is faster
"beyond the spread" when B < min(A1, A2).  The kernel rows time 20 launches between two HIP events, median of three, after a warm-up, and report
TFLOP/s of 2 * 9 * Cin * Cout * pixels.  Prints text rows (also written to `out`), then one JSON line.
"""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd")]

import numpy as np
import torch

from sr355 import Context
from sr355.patches import PatchPairs, window_table

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
fits = int(sys.argv[2]) if len(sys.argv) > 2 else 3
scales = [int(s) for s in (sys.argv[3] if len(sys.argv) > 3 else "2,4").split(",")]
batches = [int(s) for s in (sys.argv[4] if len(sys.argv) > 4 else "16,64,256").split(",")]
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "edsr_mixed_aba.txt")
ctx = Context.get(0)
rng = np.random.default_rng(0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def dataset(scale, batch):
    """Random uint8 stacks -> PatchPairs views of exactly steps * batch training patches and one validation batch."""
    lr_hw = (239, 239) if scale == 2 else (120, 120)
    need = (steps + 1) * batch
    hr_hw = (lr_hw[0] * scale, lr_hw[1] * scale)
    n_images = -(-need // len(window_table(1, lr_hw, hr_hw, "scale", 24, 12, scale)[0]))
    lr = rng.integers(0, 256, (n_images,) + lr_hw + (3,), dtype=np.uint8)
    hr = rng.integers(0, 256, (n_images,) + hr_hw + (3,), dtype=np.uint8)
    ds = PatchPairs.from_stacks(lr, hr, "scale", 24, 12, scale, ctx=ctx)
    assert len(ds) >= need, (len(ds), need)
    pick = np.random.default_rng(1).permutation(len(ds))[:need]
    tr, va = ds.subset(pick[:steps * batch]), ds.subset(pick[steps * batch:])
    return tr.X, tr.Y, va.X, va.Y


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ms_per_step(data, scale, batch, train_dtype):
    """Median over `fits` counted fits (after one warm-up) of a fresh model's one-epoch fit, in ms per training step."""
    from SRModels.deep_learning_models.EDSR_model import EDSR
    times = []
    for i in range(fits + 1):
        m = EDSR(update="device", train_dtype=train_dtype)
        with contextlib.redirect_stdout(io.StringIO()):
            m.setup_model(scale_factor=scale, num_res_blocks=16, num_filters=64, learning_rate=1e-4)
            ms = event_ms(lambda: m.fit(*data, batch_size=batch, epochs=1, verbose=False))
        if i:
            times.append(ms / steps)
    ctx.conv_prepack_bf16(None)
    return float(np.median(times))


def aba(scale, batch, data):
    a1 = ms_per_step(data, scale, batch, "f32")
    bb = ms_per_step(data, scale, batch, "bf16")
    a2 = ms_per_step(data, scale, batch, "f32")
    mean_a = 0.5 * (a1 + a2)
    row = {"scale": scale, "batch": batch, "A1_ms": a1, "B_ms": bb, "A2_ms": a2, "ratio_B_over_A": bb / mean_a, "aa_spread": abs(a1 - a2) / mean_a,
           "B_faster_beyond_spread": bool(bb < min(a1, a2))}
    say(f"EDSR x{scale} batch {batch:3d}  A = fp32 device fit  B = bf16 mixed   A1 {a1:9.3f}  B {bb:9.3f}  A2 {a2:9.3f} ms/step   B/A {row['ratio_B_over_A']:.3f}   "
        f"A/A spread {100 * row['aa_spread']:.1f} %   {'B faster beyond the spread' if row['B_faster_beyond_spread'] else 'B NOT faster beyond the spread'}")
    return row


def kernel_row(shape):
    B, H, W, cin, cout = shape
    x = torch.randn((B, H, W, cin), device=ctx.torch_device)
    dy = torch.randn((B, H, W, cout), device=ctx.torch_device)
    x16, dy16 = x.to(torch.bfloat16), dy.to(torch.bfloat16)
    out = (ctx.empty((3, 3, cin, cout)), ctx.empty((cout,)))
    flop = 2.0 * 9 * cin * cout * B * H * W

    def timed(fn):
        fn()
        return float(np.median([event_ms(lambda: [fn() for _ in range(20)]) / 20 for _ in range(3)]))
    t32 = timed(lambda: ctx.conv2d_wgrad(x, dy, 3, out=out))
    t16 = timed(lambda: ctx.conv2d_wgrad_bf16(x16, dy16, 3, out=out))
    row = {"shape": list(shape), "f32_us": 1e3 * t32, "bf16_us": 1e3 * t16, "f32_tflops": flop / t32 / 1e9, "bf16_tflops": flop / t16 / 1e9}
    say(f"wgrad {str(shape):24s} sr_conv2d_wgrad {1e3 * t32:8.1f} us {row['f32_tflops']:7.2f} TFLOP/s   sr_conv2d_wgrad_bf16 {1e3 * t16:8.1f} us {row['bf16_tflops']:7.2f} TFLOP/s   "
        f"bf16 / fp32 time {t16 / t32:.3f}")
    return row


say(f"device {torch.cuda.get_device_name(0)}; {steps} steps per fit, median of {fits} fits after a warm-up, HIP-event timed")
rows = []
for scale in scales:
    for batch in batches:
        data = dataset(scale, batch)
        rows.append(aba(scale, batch, data))
        del data
krows = [kernel_row(s) for s in ((16, 24, 24, 64, 64), (64, 24, 24, 64, 64), (16, 48, 48, 64, 256))]
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
print(json.dumps({"tool": "bench_fit_mixed", "steps": steps, "fits": fits, "rows": rows, "kernels": krows}))
