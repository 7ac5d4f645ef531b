#!/bin/bash
# One lease of an A/B of the headline against another built checkout (the protocol of profiles/r08a_dispatch_ab.txt):
# 5 alternating pairs, the other tree first, of `python bench.py` and `python tools/step_launch_floor.py`; one traced
# `python bench.py` per tree (rocprofv3 --kernel-trace --stats, nothing else traced); one alternating pair of
# `python bench.py --full`.  Every run has its own time limit and the lease stops at the first abnormal exit.
#   bash tools/ab_bench.sh <built checkout of the parent> <output directory>
#   python tools/ab_bench_summary.py <output directory of lease 1> <output directory of lease 2>
set -o pipefail
PARENT=$(cd "$1" && pwd) || exit 2
HERE=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$2" || exit 2
OUT=$(cd "$2" && pwd)
one() {  # tree tag limit command...
  local dir=$1 tag=$2 lim=$3; shift 3
  ( cd "$dir" && timeout -k 10 "$lim" "$@" > "$OUT/$tag.log" 2> "$OUT/$tag.err" )
  local rc=$?
  if [ $rc -ne 0 ]; then echo "ABNORMAL EXIT $rc: $tag"; tail -5 "$OUT/$tag.err"; exit 1; fi
}
for p in 1 2 3 4 5; do
  one "$PARENT" parent_bench_$p 120 python bench.py
  one "$PARENT" parent_floor_$p 120 python tools/step_launch_floor.py
  one "$HERE" change_bench_$p 120 python bench.py
  one "$HERE" change_floor_$p 120 python tools/step_launch_floor.py
  echo "pair $p done"
done
one "$PARENT" parent_trace 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_parent" -- python bench.py
one "$HERE" change_trace 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_change" -- python bench.py
for t in parent change; do
  find "$OUT/trace_$t" -name "*kernel_stats.csv" -exec cp {} "$OUT/kernel_stats_$t.csv" \;
  rm -rf "$OUT/trace_$t"
done
one "$PARENT" parent_full 900 python bench.py --full
one "$HERE" change_full 900 python bench.py --full
echo "lease complete: $OUT"
