"""FineTunedVGG16.fit (VGG16_model.py:111-157) at the reference's batch: 32 images of 128 x 128 x 3, augmentation and dropout on, fp32 and
bf16.  Times the device path (FineTunedVGG16.fit: sr_affine_warp, the frozen base, sr_dense_head_step + DeviceAdam) and the host reference
path composed from _augment (SciPy), _gap_features and train.fit_head, alternating them in one process.  Prints one JSON line per dtype:
ms per batch and epochs per second of each path and their ratio.

    python tools/bench_vgg_fit.py [n_train=256] [epochs=2] [rounds=2] [dtypes=f32,bf16] [paths=device,host]

A path's time is the wall time of a whole fit (validation pass and per-epoch host work included) divided by the batches it ran; the first
fit of each path and dtype is a warm-up and is not counted.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd")]
import contextlib
import io

import numpy as np
import torch

from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
from sr355.train import fit_head

n_train = int(sys.argv[1]) if len(sys.argv) > 1 else 256
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
dtypes = (sys.argv[4] if len(sys.argv) > 4 else "f32,bf16").split(",")
paths = (sys.argv[5] if len(sys.argv) > 5 else "device,host").split(",")      # "device" alone: a kernel-trace run of the device path
HW, BS, N_VAL = 128, 32, 64
rng = np.random.default_rng(0)
X, y = rng.uniform(0, 1, (n_train, HW, HW, 3)).astype(np.float32), rng.integers(0, 2, n_train)
Xv, yv = rng.uniform(0, 1, (N_VAL, HW, HW, 3)).astype(np.float32), rng.integers(0, 2, N_VAL)
batches_per_fit = epochs * ((n_train + BS - 1) // BS)


def model(dtype):
    m = FineTunedVGG16(compute_dtype=dtype)
    m.setup_model(input_shape=(HW, HW, 3), num_classes=2, dropout_rate=0.2, learning_rate=1e-4)
    return m


def device_fit(m):
    return m.fit(X, y, Xv, yv, epochs=epochs, use_augmentation=True, seed=1)


def host_fit(m):
    r = np.random.default_rng(1)

    def batches(epoch):
        order = r.permutation(len(X))
        for i in range(0, len(order), BS):
            idx = order[i:i + BS]
            yield m._augment(X[idx], r), y[idx]

    return fit_head(m._gap_features, m.weights, batches, y, Xv, yv, learning_rate=m.learning_rate, batch_size=BS, epochs=epochs,
                    dropout_rate=m.dropout_rate, seed=1)


def timed(fn, m):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        fn(m)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for dtype in dtypes:
    m = model(dtype)
    t = {"device": [], "host": []}
    for r in range(rounds + 1):                       # round 0: warm-up of both paths
        for name, fn in (("device", device_fit), ("host", host_fit)):
            if name not in paths:
                continue
            s = timed(fn, m)
            if r:
                t[name].append(s)
    row = {"bench": "vgg16_fit", "dtype": dtype, "batch": BS, "hw": HW, "n_train": n_train, "n_val": N_VAL, "epochs_per_fit": epochs,
           "rounds": rounds}
    for name in paths:
        s = float(np.median(t[name]))
        row[f"{name}_ms_per_batch"] = 1e3 * s / batches_per_fit
        row[f"{name}_epochs_per_s"] = epochs / s
    if len(paths) == 2:
        row["speedup"] = row["host_ms_per_batch"] / row["device_ms_per_batch"]
    print(json.dumps(row), flush=True)
