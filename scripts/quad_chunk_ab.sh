#!/bin/bash
# A/B of the quad kernel between two BUILT trees on one MI355X (the procedure of scripts/fused_ingest_ab.sh): the parent commit and
# this one (the Riccati chunk's diet).  Every run is its own process under its own time limit, on the library of
# its side (NMPC_HIP_DDP_LIB: the Python side is this tree's for both); the script stops at the first step that fails.
#   1. bench.py c2 (2000 steps), c3 (1000 steps) and --mode m1 (200 steps): parent / new / parent / new ...;
#   2. one rocprofv3 --kernel-trace --stats run of 200 c2 steps per side (no counters in the same run);
#   3. the backward / forward split of the solve kernel, c2 and c3 (scripts/quad_phases.py);
#   4. the default bench line of both sides (M1 leg, c3), once each;
#   5. the outputs of the last solve (--dump-outputs) of c2, c3 and m1, compared byte for byte.
# Writes OUT/quad_chunk_ab.txt (the layout of profiles/quad_chunk_ab.txt) and keeps the raw lines beside it.
# usage: scripts/quad_chunk_ab.sh PARENT_TREE NEW_TREE OUT_DIR [runs per side, default 5]
set -u -o pipefail
PARENT=$(realpath "$1") NEW=$(realpath "$2") OUT=$(realpath -m "$3") RUNS=${4:-5}
mkdir -p "$OUT"
TXT=$OUT/quad_chunk_ab.txt
BENCH="python bench.py --no-cpu-baseline --no-secondary --no-extra-modes"
lib() { [ "$1" = new ] && echo "$NEW/nmpc_amd/lib/libnmpc_hip_ddp.so" || echo "$PARENT/nmpc_amd/lib/libnmpc_hip_ddp.so"; }
cd "$NEW" || exit 1

echo "# scripts/quad_chunk_ab.sh on one MI355X: parent = the commit before, new = this tree.  $BENCH, runs interleaved" > "$TXT"
for leg in "c2 --workload c2 --steps 2000 --warmup 50" "c3 --workload c3 --steps 1000 --warmup 50" "m1 --mode m1 --steps 200 --warmup 10"; do
  set -- $leg; name=$1; shift
  for i in $(seq 1 "$RUNS"); do
    for side in parent new; do
      NMPC_HIP_DDP_LIB=$(lib $side) timeout -k 10 180 $BENCH "$@" > "$OUT/bench_${name}_${side}_$i.json" 2> "$OUT/bench_${name}_${side}_$i.err" \
        || { echo "bench $name $side $i failed: $?" | tee -a "$TXT"; exit 1; }
    done
  done
  python - "$OUT" "$RUNS" "$name" "$*" <<'EOF' | tee -a "$TXT"
import json, statistics, sys
out, runs, name, args = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
v = {s: [json.loads([l for l in open(f"{out}/bench_{name}_{s}_{i}.json") if l.startswith("{")][-1]) for i in range(1, runs + 1)] for s in ("parent", "new")}
print(f"# {name}: {args}")
for i in range(runs):
    for s in ("parent", "new"):
        print(f"{name} {s:7s} run {i + 1}  value {v[s][i]['value']:.1f}  ms_per_step {v[s][i]['ms_per_step']:.5f}")
p, n = ([d["value"] for d in v[s]] for s in ("parent", "new"))
spread = max(p) - min(p)
print(f"{name} value: parent median {statistics.median(p):.1f} (min {min(p):.1f}, max {max(p):.1f}, spread {spread:.1f})  new median {statistics.median(n):.1f} "
      f"(min {min(n):.1f}, max {max(n):.1f})  difference of medians {statistics.median(n) - statistics.median(p):+.1f} = "
      f"{(statistics.median(n) / statistics.median(p) - 1) * 100:+.2f} %, {(statistics.median(n) - statistics.median(p)) / max(spread, 1e-300):.1f} x the parent's spread; "
      f"every new run above every parent run: {min(n) > max(p)}")
EOF
done

for side in parent new; do
  rm -rf "$OUT/trace_$side"
  NMPC_HIP_DDP_LIB=$(lib $side) timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/trace_$side" -o t --output-format csv -- $BENCH --steps 200 --warmup 10 \
    > "$OUT/trace_$side.log" 2>&1 || { echo "trace $side failed: $?" | tee -a "$TXT"; exit 1; }
  echo "# rocprofv3 --kernel-trace --stats, $side, c2, 200 steps + 10 warm-up: Name,Calls,TotalDurationNs,AverageNs,Percentage,MinNs,MaxNs,StdDev" >> "$TXT"
  find "$OUT/trace_$side" -name "*kernel_stats.csv" | head -1 | xargs grep -E "ddp_solve_quad_kernel" | tee -a "$TXT"
done

echo "# solve kernel: HIP-event ms and its split by the phases' shader-clock shares (scripts/quad_phases.py: medians of 50 solves)" >> "$TXT"
for w in c2 c3; do
  for side in parent new; do
    NMPC_HIP_DDP_LIB=$(lib $side) timeout -k 10 180 python scripts/quad_phases.py $w $side 2> "$OUT/phases_${w}_$side.err" | tee -a "$TXT" \
      || { echo "phases $w $side failed" | tee -a "$TXT"; exit 1; }
  done
done

echo "# the default line (python bench.py --no-cpu-baseline), parent / new" >> "$TXT"
for side in parent new; do
  NMPC_HIP_DDP_LIB=$(lib $side) timeout -k 10 600 python bench.py --no-cpu-baseline > "$OUT/default_$side.json" 2> "$OUT/default_$side.err" \
    || { echo "default line $side failed: $?" | tee -a "$TXT"; exit 1; }
  python - "$OUT/default_$side.json" $side <<'EOF' | tee -a "$TXT"
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
def find(o, key):
    if isinstance(o, dict):
        for k, v in o.items():
            if k == key:
                yield v
            yield from find(v, key)
    elif isinstance(o, list):
        for v in o:
            yield from find(v, key)
m1 = next(find(d, "m1_value"), None)
sec = d.get("secondary", {})
c3 = sec.get("c3", {}) if isinstance(sec, dict) else {}
print(f"{sys.argv[2]:7s} c2 {d['value']:.1f} ({d['ms_per_step']:.5f})  m1 {m1}  c3 {c3.get('value') if isinstance(c3, dict) else c3}")
EOF
done

same=1
for leg in "c2 --workload c2" "c3 --workload c3" "m1 --mode m1"; do
  set -- $leg; name=$1; shift
  for side in parent new; do
    NMPC_HIP_DDP_LIB=$(lib $side) timeout -k 10 180 $BENCH "$@" --steps 20 --warmup 2 --dump-outputs "$OUT/dump_${name}_$side" > "$OUT/dump_${name}_$side.log" 2>&1 \
      || { echo "dump $name $side failed: $?" | tee -a "$TXT"; exit 1; }
  done
  leg_same=1
  for f in $(ls "$OUT/dump_${name}_parent"); do
    cmp -s "$OUT/dump_${name}_parent/$f" "$OUT/dump_${name}_new/$f" || { leg_same=0; same=0; echo "outputs differ: $name $f" | tee -a "$TXT"; }
  done
  [ $leg_same = 1 ] && echo "# --dump-outputs $name: $(ls "$OUT/dump_${name}_parent" | tr '\n' ' ')byte-identical between the two sides" | tee -a "$TXT"
done
[ $same = 1 ]
