#!/bin/bash
# A/B of the headline workload between two BUILT trees on one MI355X: the parent commit (ingest_kernel + solve kernel per solve) and
# this one (the quad kernel converts the caller's inputs itself: one dispatch per solve).
#   1. bench.py c2, 2000 steps, parent / new / parent / new ..., every run its own process under its own time limit;
#   2. one rocprofv3 --kernel-trace --stats run of 200 steps per tree (no counters in the same run);
#   3. the outputs of the last solve of both trees (--dump-outputs), compared byte for byte.
# Stops at the first step that fails or runs into its time limit.  Writes OUT/fused_ingest_ab.txt (the layout of
# profiles/fused_ingest_ab.txt) and keeps the raw lines beside it.
# usage: scripts/fused_ingest_ab.sh PARENT_TREE NEW_TREE OUT_DIR [runs per tree, default 5]
set -u -o pipefail
PARENT=$(realpath "$1") NEW=$(realpath "$2") OUT=$(realpath -m "$3") RUNS=${4:-5}
mkdir -p "$OUT"
TXT=$OUT/fused_ingest_ab.txt
BENCH="python bench.py --no-cpu-baseline --no-secondary --no-extra-modes"
field() { python -c "import json,sys; d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1]); print(d[sys.argv[2]])" "$1" "$2"; }

echo "# scripts/fused_ingest_ab.sh on one MI355X: parent = the commit before (event, ingest_kernel, event, solve kernel, event per solve)," > "$TXT"
echo "# new = this tree (event, solve kernel, event).  $BENCH --steps 2000 --warmup 50, runs interleaved" >> "$TXT"
for i in $(seq 1 "$RUNS"); do
  for side in parent new; do
    tree=$PARENT; [ $side = new ] && tree=$NEW
    (cd "$tree" && timeout -k 10 180 $BENCH --steps 2000 --warmup 50) > "$OUT/bench_${side}_$i.json" 2> "$OUT/bench_${side}_$i.err" || { echo "bench $side $i failed: $?" | tee -a "$TXT"; exit 1; }
    printf "c2 %-7s run %d  value %s  ms_per_step %s\n" $side "$i" "$(field "$OUT/bench_${side}_$i.json" value)" "$(field "$OUT/bench_${side}_$i.json" ms_per_step)" | tee -a "$TXT"
  done
done
python - "$OUT" "$RUNS" <<'EOF' | tee -a "$TXT"
import json, statistics, sys
out, runs = sys.argv[1], int(sys.argv[2])
v = {s: [json.loads([l for l in open(f"{out}/bench_{s}_{i}.json") if l.startswith("{")][-1]) for i in range(1, runs + 1)] for s in ("parent", "new")}
for key in ("value", "ms_per_step"):
    p, n = ([d[key] for d in v[s]] for s in ("parent", "new"))
    print(f"{key}: parent median {statistics.median(p):.5g} (min {min(p):.5g}, max {max(p):.5g}, spread {max(p) - min(p):.3g})  "
          f"new median {statistics.median(n):.5g} (min {min(n):.5g}, max {max(n):.5g})  "
          f"difference of medians {statistics.median(n) - statistics.median(p):+.3g} = {(statistics.median(n) / statistics.median(p) - 1) * 100:+.2f} %, "
          f"{abs(statistics.median(n) - statistics.median(p)) / max(max(p) - min(p), 1e-300):.1f} x the parent's spread")
EOF

for side in parent new; do
  tree=$PARENT; [ $side = new ] && tree=$NEW
  rm -rf "$OUT/trace_$side"
  (cd "$tree" && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/trace_$side" -o t --output-format csv -- $BENCH --steps 200 --warmup 10) > "$OUT/trace_$side.log" 2>&1 || { echo "trace $side failed: $?" | tee -a "$TXT"; exit 1; }
  echo "# rocprofv3 --kernel-trace --stats, $side, 200 steps + 10 warm-up: Name,Calls,TotalDurationNs,AverageNs,Percentage,MinNs,MaxNs,StdDev" >> "$TXT"
  find "$OUT/trace_$side" -name "*kernel_stats.csv" | head -1 | xargs grep -E "ddp_solve_quad_kernel|ingest_kernel" | tee -a "$TXT"
done

for side in parent new; do
  tree=$PARENT; [ $side = new ] && tree=$NEW
  (cd "$tree" && timeout -k 10 180 $BENCH --steps 50 --warmup 5 --dump-outputs "$OUT/dump_$side") > "$OUT/dump_$side.log" 2>&1 || { echo "dump $side failed: $?" | tee -a "$TXT"; exit 1; }
done
same=1
for f in $(ls "$OUT/dump_parent"); do
  cmp -s "$OUT/dump_parent/$f" "$OUT/dump_new/$f" || { same=0; echo "outputs differ: $f" | tee -a "$TXT"; }
done
[ $same = 1 ] && echo "# --dump-outputs: $(ls "$OUT/dump_parent" | tr '\n' ' ')byte-identical between the two trees" | tee -a "$TXT"
[ $same = 1 ]
