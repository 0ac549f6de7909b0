"""What the host round trip per image costs the classifier path, measured: prints one JSON line.

(a) 64 dataset-sized frames (478 x 478, VGG_PATCH_SIZE 96 / VGG_STRIDE 48: 81 patches each) classified by a loop of
    `classify_defects_method` (one extraction, one predict, one read and a host vote per frame) and by one `classify_defects_batch`
    (one extraction, one predict, one device vote, one read).
(b) `stream_sr_classify` at the cfg4 shape of sr355.bench_rows (1080p uint8 frames -> ESRGAN x4, NB = 23, G = 32, bf16 -> 14 400 classifier
    patches per frame) with vote="host" and vote="device".

Both pairs run in one process after a warm-up, interleaved A-B-A-B; every repetition's wall time is kept, the line states median, min and
max.  The loop and the "host" vote are the baseline.

    python tools/bench_study.py [reps=5] [stream_frames=4]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd")]
import numpy as np
import torch

from sr355 import Context
from sr355.pipeline import stream_sr_classify
from sr355.synth import hr_tile
from sr355.weights import bf16_rounded, condition_attention, init_weights
from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
stream_frames = int(sys.argv[2]) if len(sys.argv) > 2 else 4
ctx = Context.get(0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": [round(v, 3) for v in ms]}


c = FineTunedVGG16(compute_dtype="bf16")
c.setup_model(input_shape=(96, 96, 3), num_classes=2)
c.set_weights(c.weights)

# ---- (a) 64 frames of 478 x 478, resident on the device as the SR methods leave them
rng = np.random.default_rng(64)
stack = ctx.to_device(np.stack([hr_tile(rng, 478, 478) for _ in range(64)]))
loop = lambda: [c.classify_defects_method(stack[i]) for i in range(len(stack))]
batch = lambda: c.classify_defects_batch(stack)
ref, got = loop(), batch()                                                   # warm-up; how far the two paths agree goes into the line
agree = {"classes_equal": [r[0] for r in ref] == [int(v) for v in got[0]], "max_confidence_diff": max(abs(r[1] - float(g)) for r, g in zip(ref, got[1]))}
t_loop, t_batch = [], []
for _ in range(reps):
    t_loop.append(timed(loop)[0])
    t_batch.append(timed(batch)[0])
part_a = {"frames": 64, "frame": "478x478 fp32 RGB on the device", "patches_per_frame": ctx.num_patches(478, 478, 3, 96, 48),
          "loop_classify_defects_method": spread(t_loop), "classify_defects_batch": spread(t_batch),
          "loop_ms_per_frame": statistics.median(t_loop) / 64, "batch_ms_per_frame": statistics.median(t_batch) / 64, "agreement": agree}
del stack

# ---- (b) the cfg4 stream, vote on the host against vote on the device
g = ESRGAN(compute_dtype="bf16")
g.setup_model(scale_factor=4, growth_channels=32, num_rrdb_blocks=23)
g.set_weights(bf16_rounded(condition_attention(init_weights(g.generator.layer_shapes(), seed=3000))))
rng = np.random.default_rng(42 + 4)
base = [(hr_tile(rng, 1080, 1920) * 255).astype(np.uint8) for _ in range(2)]
frames = [base[i % 2] for i in range(stream_frames)]
kw = dict(patch_size_lr=48, stride=24, batch_size=3600)
run = lambda vote: stream_sr_classify(g, c, frames, sr_kwargs=kw, batch_size=2048, vote=vote)
for vote in ("host", "device"):
    stream_sr_classify(g, c, frames[:1], sr_kwargs=kw, batch_size=2048, vote=vote)     # warm-up: workspaces, first touch
walls, cls_ms, votes = {"host": [], "device": []}, {"host": [], "device": []}, {}
for _ in range(reps):
    for vote in ("host", "device"):
        res, stats = run(vote)
        walls[vote].append(1e3 * stats["wall_s"] / len(frames))
        cls_ms[vote].append(stats["host_ms_per_frame_classify"])
        votes[vote] = [(r["class"], round(r["confidence"], 4)) for r in res]
part_b = {"frames": len(frames), "frame": "1080x1920 uint8 RGB (LR input)", "patches_classifier_per_frame": 14400,
          "vote_host_ms_per_frame": spread(walls["host"]), "vote_device_ms_per_frame": spread(walls["device"]),
          "host_ms_per_frame_classify": {k: statistics.median(v) for k, v in cls_ms.items()}, "votes": votes}

print(json.dumps({"bench": "study", "device": torch.cuda.get_device_name(0), "reps": reps, "classify_64_frames": part_a, "cfg4_stream": part_b}))
