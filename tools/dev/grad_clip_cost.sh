#!/bin/bash
# Gradient clipping: cost of max_grad_norm on one box, in one call (NOTES.md 0.04).
#   bash tools/dev/grad_clip_cost.sh OUT_DIR [PARENT_TREE]
# 1. tools/dev/grad_clip_step.py: alternating rounds of the headline step with max_grad_norm = None / a finite bound / inf;
# 2. bench.py of PARENT_TREE (a built checkout of the parent commit; skipped when not given) and of this tree, alternated;
# 3. one rocprofv3 --kernel-trace --stats run of clipped steps, for the two norm kernels' and the clipped Adam's times.
# Every GPU step under its own timeout, chained with &&.
set -u
R="$(cd "$(dirname "$0")/../.." && pwd)"
O="${1:?output directory}"
P="${2:-}"
mkdir -p "$O"
bench_line() { ( cd "$1" && timeout -k 10 240 python3 bench.py --gpus 1 --steps 20 --warmup 5 ) > "$O/$2.log" 2> "$O/$2.err" && tail -n 1 "$O/$2.log" > "$O/$2.json"; }
timeout -k 10 400 python3 "$R/tools/dev/grad_clip_step.py" "$O/grad_clip_step.json" > "$O/grad_clip_step.log" 2>&1 &&
{ [ -z "$P" ] || bench_line "$P" bench_parent_1; } &&
bench_line "$R" bench_this_1 &&
{ [ -z "$P" ] || bench_line "$P" bench_parent_2; } &&
bench_line "$R" bench_this_2 &&
MODE=trace STEPS=16 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace" -- python3 "$R/tools/dev/grad_clip_step.py" > "$O/trace.log" 2>&1
rc=$?
cat "$O/grad_clip_step.log"
python3 - "$O" <<'PY'
import glob, json, sys
o = sys.argv[1]
for f in sorted(glob.glob(o + "/bench_*.json")):
    d = json.loads(open(f).read())
    print(f.rsplit("/", 1)[1], {k: d.get(k) for k in ("ms_per_step", "loss", "value") if k in d} or list(d)[:12])
for f in glob.glob(o + "/trace/**/*kernel_stats.csv", recursive=True):
    for line in open(f):
        if any(k in line for k in ("Name", "grad_norm", "adam_kernel")):
            print(line.rstrip())
PY
exit $rc
