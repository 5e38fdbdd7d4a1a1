#!/bin/bash
# Sequence-level REINFORCE: cost and gain of score_function="sequence" on one box, in one call (NOTES.md 0.06).
#   bash tools/dev/seq_score_cost.sh OUT_DIR [PARENT_TREE]
# 1. tools/dev/seq_score_step.py: alternating rounds of "path" against "sequence" (K = 4, both baselines, capped and not, fresh and
#    trained model), loss-section phase, peak memory;
# 2. MODE=variance: mean and variance of the REINFORCE gradient over 256 sampler offsets, both score functions;
# 3. one rocprofv3 --kernel-trace --stats run each of the fresh and the trained model with "sequence" (the new kernels' times);
# 4. bench.py of PARENT_TREE (a built checkout of the parent commit; skipped when not given) and of this tree, alternated.
# Every GPU step under its own timeout, chained with &&.
set -u
R="$(cd "$(dirname "$0")/../.." && pwd)"
O="${1:?output directory}"
P="${2:-}"
mkdir -p "$O"
O="$(cd "$O" && pwd)"
[ -z "$P" ] || P="$(cd "$P" && pwd)"
bench_line() { ( cd "$1" && timeout -k 10 240 python3 bench.py --gpus 1 --steps 20 --warmup 5 ) > "$O/$2.log" 2> "$O/$2.err" && tail -n 1 "$O/$2.log" > "$O/$2.json"; }
trace() { ( cd "$R" && STATE=$1 MODE=trace CONFIG=seq_loo STEPS=6 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace_$1" -- python3 tools/dev/seq_score_step.py ) > "$O/trace_$1.log" 2>&1; }
timeout -k 10 420 python3 "$R/tools/dev/seq_score_step.py" "$O/seq_score_step.json" > "$O/seq_score_step.log" 2>&1 &&
MODE=variance timeout -k 10 300 python3 "$R/tools/dev/seq_score_step.py" "$O/seq_score_variance.json" > "$O/seq_score_variance.log" 2>&1 &&
trace fresh && trace trained &&
{ [ -z "$P" ] || bench_line "$P" bench_parent_1; } &&
bench_line "$R" bench_this_1 &&
{ [ -z "$P" ] || bench_line "$P" bench_parent_2; } &&
bench_line "$R" bench_this_2 &&
{ [ -z "$P" ] || bench_line "$P" bench_parent_3; } &&
bench_line "$R" bench_this_3
rc=$?
cat "$O/seq_score_step.log" "$O/seq_score_variance.log"
for s in fresh trained; do
    f=$(find "$O/trace_$s" -name "*kernel_stats.csv" 2>/dev/null | head -n 1)
    [ -z "$f" ] || { echo "== kernel stats, $s model"; grep -E "Name|ctc_|pg_loss_value" "$f" | cut -c1-220; }
done
python3 - "$O" <<'PY'
import glob, json, sys
o = sys.argv[1]
for f in sorted(glob.glob(o + "/bench_*.json")):
    d = json.loads(open(f).read())
    print(f.rsplit("/", 1)[1], {k: d.get(k) for k in ("ms_per_step", "loss", "value") if k in d} or list(d)[:12])
PY
exit $rc
