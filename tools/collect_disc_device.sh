#!/bin/bash
# cfg3 (the full ESRGAN _train_step at x4 / NB 23 / G 32 / 16 x 24^2) with the discriminator's update on the host and on the device, from the repo root:
#     tools/collect_disc_device.sh OUTPUT_DIR          (a directory that does not exist yet, or an empty one)
#   1. tools/bench_train.py three times in each mode, alternating, at its default steps / batch  -> disc_device_cfg3.json (six JSON lines)
#   2. rocprofv3 --kernel-trace --memory-copy-trace (no counters) of 2 and of 5 timed steps in each mode; the difference of the two runs' copy
#      counts over 3 is the copies of one step AS THE TRACER SEES THEM, set-up and warm-up excluded  -> disc_device_copies.json
#      the device mode's 5-step run also writes per-kernel statistics; the new kernels' rows     -> disc_device_new_kernel_stats.csv
#   3. tools/count_step_copies.py: the copies the step's host code issues, counted at the call   -> disc_device_step_copies.json
# Every GPU step has its own time limit and the script stops at the first one that fails.
set -o pipefail
ROOT=$(pwd)
OUT=${1:?usage: tools/collect_disc_device.sh OUTPUT_DIR}
case "$OUT" in /*) ;; *) OUT=$ROOT/$OUT ;; esac
if [ -e "$OUT" ] && { [ ! -d "$OUT" ] || [ -n "$(ls -A "$OUT")" ]; }; then echo "$OUT exists and is not an empty directory: not touched"; exit 2; fi
mkdir -p "$OUT"
: > "$OUT/disc_device_cfg3.json"
for rep in 1 2 3; do
    for mode in host device; do
        timeout -k 10 240 python3 tools/bench_train.py 3 16 $mode 2> "$OUT/bench_${mode}_${rep}.err" | tail -1 >> "$OUT/disc_device_cfg3.json" || { echo "bench $mode $rep failed"; tail -5 "$OUT/bench_${mode}_${rep}.err"; exit 1; }
    done
done
cut -c1-260 "$OUT/disc_device_cfg3.json"
for mode in host device; do
    for steps in 2 5; do
        stats=; [ "$mode$steps" = device5 ] && stats=--stats
        timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace $stats --output-format csv -d "$OUT/trace_${mode}_${steps}" -o t -- python3 tools/bench_train.py $steps 16 $mode > "$OUT/trace_${mode}_${steps}.log" 2>&1 \
            || { echo "trace $mode $steps failed"; tail -5 "$OUT/trace_${mode}_${steps}.log"; exit 1; }
    done
done
python3 - "$OUT" <<'EOF' | tee "$OUT/disc_device_copies.json"
import csv, glob, json, sys
out = sys.argv[1]


def counts(d):
    c = {"kernels": 0}
    for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
        c["kernels"] += sum(1 for _ in csv.DictReader(open(f)))
    for f in glob.glob(f"{d}/**/*memory_copy_trace.csv", recursive=True):
        for row in csv.DictReader(open(f)):
            k = next((v for key, v in row.items() if key and "irection" in key), "UNKNOWN")
            c[k] = c.get(k, 0) + 1
    return c


res = {}
for mode in ("host", "device"):
    a, b = counts(f"{out}/trace_{mode}_2"), counts(f"{out}/trace_{mode}_5")
    res[mode] = {"per_step": {k: (b.get(k, 0) - a.get(k, 0)) / 3.0 for k in sorted(set(a) | set(b))}, "run_of_2_steps": a, "run_of_5_steps": b}
print(json.dumps(res))
EOF
f=$(find "$OUT/trace_device_5" -name "*kernel_stats.csv" | head -1)
{ head -1 "$f"; grep -E "spectral_norm_kernel|disc_head_(rows|grads)_kernel" "$f"; } > "$OUT/disc_device_new_kernel_stats.csv" || { echo "no statistics of the new kernels"; exit 1; }
cut -c1-200 "$OUT/disc_device_new_kernel_stats.csv"
for mode in host device; do for steps in 2 5; do rm -rf "$OUT/trace_${mode}_${steps}"; done; done
timeout -k 10 400 python3 tools/count_step_copies.py 2> "$OUT/count.err" | tail -1 | tee "$OUT/disc_device_step_copies.json" || { echo "copy count failed"; tail -5 "$OUT/count.err"; exit 1; }
