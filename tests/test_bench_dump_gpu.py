"""`bench.py --dump-outputs DIR` end to end: the last timed step's outputs land as float .npy files under the 64 MB cap, agree with the JSON
line's metrics, and two runs with the same arguments write the same arrays (seeded inputs, deterministic kernels)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0", "--tiles", "2", "--tiles-per-call", "2",
           "--no-cpu-baseline", "--no-parity", "--no-rows", "--no-profile", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert lines, r.stdout[-2000:]
    return json.loads(lines[-1])


def test_dump_outputs_are_the_timed_steps_results_and_reproducible(tmp_path):
    line = _bench(tmp_path / "a")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    names = sorted(line["dump_outputs"]["arrays"])
    assert names == ["metric_sums", "psnr", "sr_sample", "ssim"] and sorted(os.listdir(tmp_path / "a")) == [n + ".npy" for n in names]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64_000_000
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    sr = a["sr_sample"]
    assert sr.shape[0] == 2 and sr.shape[2] == 3 and np.isfinite(sr).all() and sr.min() >= 0.0 and sr.max() <= 1.0
    assert a["metric_sums"][2] == 2 and np.allclose(a["metric_sums"][:2], [a["psnr"].sum(), a["ssim"].sum()], rtol=1e-12)
    assert a["psnr"].mean() == pytest.approx(line["quality"]["mean_psnr_vs_hr_db"], rel=1e-12)
    _bench(tmp_path / "b")
    for n in names:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy")), n


def test_plain_run_carries_the_headline_and_nothing_that_needs_runs_of_its_own():
    """Without --full the line holds the headline and what the timed steps give anyway; the per-kernel pass, the clock reading, the CPU baseline,
    the parity objects and the other BASELINE rows are --full's."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--tiles", "2", "--tiles-per-call", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "4x-SR MPix/s on 512x512 LR batch" and line["unit"] == "MPix/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * 2048 * 2048 / 1e6 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["config"]["full"] is False and line["roofline"] is None and line["kernels"] == []
    assert not {"cpu_baseline", "parity", "parity_trained_like", "rows", "dump_outputs"} & set(line)
