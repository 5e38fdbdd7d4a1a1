#!/bin/bash
# Gradient accumulation: cost of step_accumulated on one box, in one call (NOTES.md 0.05).
#   bash tools/dev/grad_accum_cost.sh OUT_DIR [PARENT_TREE]
# 1. tools/dev/grad_accum_step.py: alternating rounds of step() against step_accumulated at the headline shape ((a) - (d));
# 2. (e) bench.py of PARENT_TREE (a built checkout of the parent commit; skipped when not given) and of this tree, alternated.
# Every GPU step under its own timeout, chained with &&.
set -u
R="$(cd "$(dirname "$0")/../.." && pwd)"
O="${1:?output directory}"
P="${2:-}"
mkdir -p "$O"
O="$(cd "$O" && pwd)"
[ -z "$P" ] || P="$(cd "$P" && pwd)"
bench_line() { ( cd "$1" && timeout -k 10 240 python3 bench.py --gpus 1 --steps 20 --warmup 5 ) > "$O/$2.log" 2> "$O/$2.err" && tail -n 1 "$O/$2.log" > "$O/$2.json"; }
timeout -k 10 420 python3 "$R/tools/dev/grad_accum_step.py" "$O/grad_accum_step.json" > "$O/grad_accum_step.log" 2>&1 &&
{ [ -z "$P" ] || bench_line "$P" bench_parent_1; } &&
bench_line "$R" bench_this_1 &&
{ [ -z "$P" ] || bench_line "$P" bench_parent_2; } &&
bench_line "$R" bench_this_2 &&
{ [ -z "$P" ] || bench_line "$P" bench_parent_3; } &&
bench_line "$R" bench_this_3
rc=$?
cat "$O/grad_accum_step.log"
python3 - "$O" <<'PY'
import glob, json, sys
o = sys.argv[1]
for f in sorted(glob.glob(o + "/bench_*.json")):
    d = json.loads(open(f).read())
    print(f.rsplit("/", 1)[1], {k: d.get(k) for k in ("ms_per_step", "loss", "value") if k in d} or list(d)[:12])
PY
exit $rc
