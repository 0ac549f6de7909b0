"""FineTunedVGG16.fit's training data, as a dense fp32 patch array against a sr355.patches.LabeledPatches view, at the reference's shapes:
478 x 478 frames generated from a seed, 96 x 96 patches at stride 48 (64 per frame), batch 32, augmentation and dropout on.  Alternates the
array fit and the view fit in one process after a warm-up round, as tools/bench_vgg_fit.py does, and prints one JSON line:

  * ms per batch of both paths, every counted round (the spread of a path against itself is the yardstick for their difference);
  * seconds from "frames decoded" (a uint8 stack on the host) to "first augmented batch ready on the device": the array path builds the
    loader's patch array and uploads it, the view path uploads the stack;
  * host and device bytes each path holds for the training set.

    python tools/bench_vgg_fit_input.py [n_frames=16] [epochs=1] [rounds=3] [dtype=f32] [out.json]

A path's time is the wall time of a whole fit (validation pass and per-epoch host work included) divided by the batches it ran.
"""
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd")]

import numpy as np
import torch

from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
from sr355 import Context
from sr355.patches import LabeledPatches

n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dtype = sys.argv[4] if len(sys.argv) > 4 else "f32"
out_path = sys.argv[5] if len(sys.argv) > 5 else None
S, PATCH, STRIDE, BS, N_VAL_FRAMES = 478, 96, 48, 32, 2
rng = np.random.default_rng(0)
frames = rng.integers(0, 256, (n_frames, S, S, 3), dtype=np.uint8)
labels = rng.integers(0, 2, n_frames)
val_frames = rng.integers(0, 256, (N_VAL_FRAMES, S, S, 3), dtype=np.uint8)
val_labels = np.arange(N_VAL_FRAMES) % 2
ctx = Context.get()


def patch_array(fr, lab):
    """load_defects_dataset_as_patches' (X, y) from decoded frames: every window of every frame, fp32."""
    X, y = [], []
    for f, l in zip(fr, lab):
        img = f.astype(np.float32) / 255.0
        for i in range(0, S - PATCH + 1, STRIDE):
            for j in range(0, S - PATCH + 1, STRIDE):
                X.append(img[i:i + PATCH, j:j + PATCH])
                y.append(int(l))
    return np.array(X, dtype=np.float32), np.array(y, dtype=np.int64)


def first_batch(path):
    """Seconds from the decoded frames to the first augmented batch on the device."""
    eye = ctx.warp_params(np.broadcast_to(np.eye(2), (BS, 2, 2)), np.zeros((BS, 2)), np.zeros(BS, bool))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if path == "array":
        X, _ = patch_array(frames, labels)
        ctx.affine_warp(ctx.to_device(X), np.arange(BS), eye)
    else:
        ds = LabeledPatches.from_stacks(frames, labels, PATCH, STRIDE, ctx=ctx)
        ds.warped_batch(ds.set_order(np.arange(len(ds))), 0, BS, eye)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed_fit(m, X, y, Xv, yv):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        m.fit(X, y, Xv, yv, epochs=epochs, use_augmentation=True, seed=1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


first = {p: [first_batch(p) for _ in range(3)] for p in ("array", "view")}            # the first of each also warms the kernels up
X, y = patch_array(frames, labels)
Xv, yv = patch_array(val_frames, val_labels)
ds = LabeledPatches.from_stacks(frames, labels, PATCH, STRIDE, ctx=ctx)
dv = LabeledPatches.from_stacks(val_frames, val_labels, PATCH, STRIDE, ctx=ctx)
batches_per_fit = epochs * ((len(X) + BS - 1) // BS)
m = FineTunedVGG16(compute_dtype=dtype)
m.setup_model(input_shape=(PATCH, PATCH, 3), num_classes=2, dropout_rate=0.2, learning_rate=1e-4)
t = {"array": [], "view": []}
for r in range(rounds + 1):                           # round 0: warm-up of both paths
    for name, args in (("array", (X, y, Xv, yv)), ("view", (ds.X, ds.y, dv.X, dv.y))):
        s = timed_fit(m, *args)
        if r:
            t[name].append(1e3 * s / batches_per_fit)
row = {"bench": "vgg16_fit_input", "dtype": dtype, "batch": BS, "frame": S, "patch": PATCH, "stride": STRIDE, "n_frames": n_frames,
       "n_patches": len(X), "n_val_patches": len(Xv), "epochs_per_fit": epochs, "rounds": rounds,
       "array_ms_per_batch": t["array"], "view_ms_per_batch": t["view"],
       "array_ms_per_batch_median": float(np.median(t["array"])), "view_ms_per_batch_median": float(np.median(t["view"])),
       "array_spread_ms": float(max(t["array"]) - min(t["array"])), "view_spread_ms": float(max(t["view"]) - min(t["view"])),
       "array_first_batch_s": first["array"][1:], "view_first_batch_s": first["view"][1:],
       "array_host_bytes": int(X.nbytes), "array_device_bytes": int(X.nbytes),
       "view_host_bytes": int(ds.host_bytes()), "view_device_bytes": int(ds.device_bytes())}
line = json.dumps(row)
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
