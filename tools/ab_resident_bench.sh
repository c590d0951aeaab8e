#!/bin/bash
# Same-box A/B of the plain bench.py run (200 steps at 1024^2): AB_PARENT (a
# build of the parent commit, e.g. tools/micro/_var/parent.so) against the
# in-tree library, alternating, AB_RUNS (default 6) runs each, profiler off;
# per run bench.py's ms_per_step and the event-timed per-step times of 400-
# and 2000-step launches (tools/resident_launch_timing.py).  Ends with the
# acceptance arithmetic: every new run below every parent run, and the median
# gain against three times the parent's own max - min.
set -o pipefail
cd "$(dirname "$0")/.."
PARENT=${AB_PARENT:-tools/micro/_var/parent.so}
OUT=${AB_OUT:-ab_resident_pipeline.out}
mkdir -p "$(dirname "$OUT")"
: > $OUT
for rep in $(seq 1 ${AB_RUNS:-6}); do
  for lib in $PARENT path_planning_2d_amd/libpp2_hip.so; do
    tag=$([ $lib = $PARENT ] && echo parent || echo new)
    ms=$(PP2_LIBRARY=$PWD/$lib timeout -k 10 120 python3 bench.py --gpus 1 --steps 200 --warmup 20 2>/dev/null |
         tail -1 | python3 -c "import json,sys; print('%.6f' % json.loads(sys.stdin.read())['ms_per_step'])") || exit 1
    ev=$(PP2_NS=400,2000 PP2_LIBRARY=$PWD/$lib timeout -k 10 60 python3 tools/resident_launch_timing.py 2>/dev/null |
         grep -E "^n= *(400|2000):" | sed -E 's/^n= *([0-9]+):.*events +[0-9.]+ us \( *([0-9.]+)\/step\).*/n\1 \2/' | tr '\n' ' ') || exit 1
    echo "$tag run $rep: bench ms_per_step $ms  events us/step $ev" >> $OUT
  done
done
python3 - $OUT > $OUT.sum <<'EOF'
import re, statistics, sys
runs = {"parent": [], "new": []}
for line in open(sys.argv[1]):
    m = re.match(r"(parent|new) run \d+: bench ms_per_step ([\d.]+)", line)
    if m:
        runs[m.group(1)].append(float(m.group(2)))
p, n = runs["parent"], runs["new"]
gain = statistics.median(p) - statistics.median(n)
spread = max(p) - min(p)
print(f"parent ms_per_step: min {min(p):.6f} median {statistics.median(p):.6f} max {max(p):.6f}")
print(f"new    ms_per_step: min {min(n):.6f} median {statistics.median(n):.6f} max {max(n):.6f}")
print(f"every new run below every parent run: {max(n) < min(p)}")
print(f"median gain {gain:.6f} ms ({100 * gain / statistics.median(p):.1f} %), parent max - min {spread:.6f}: "
      f"gain / spread = {gain / spread if spread else float('inf'):.1f} (bar: >= 3)")
EOF
cat $OUT.sum >> $OUT && rm -f $OUT.sum
cat $OUT
