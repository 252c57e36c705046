#!/bin/bash
# tools/batch_sweep.sh -- SURVEY.md 8d's batch-size sweep for config 2: B independent 2-FSK streams x 1.2 M samples resident in HBM,
# 20 timed launches after 3 warm-ups (bench.py's own clock: barrier + synchronize around the 20 steps; kernel_ms: HIP events per launch).
# One line per B and pass. Below 3072 streams the chip is not full (one stream = one wavefront, 3072 resident), which is what the table shows.
#   SIZES="1024 2048 ..."  batch sizes (default: the seven of the first sweep)      PASSES=n  passes over all sizes (default 1)
#   TREE=dir               the tree whose bench.py and library run (default: this one)
# Behind the table: the least-squares line t = intercept + slope x (B / 3072) through the launches of at least one residency (B >= 3072),
# and the largest pass-to-pass spread of a size.
set -o pipefail
R=${TREE:-$(cd "$(dirname "$0")/.." && pwd)}
SIZES=${SIZES:-"64 256 1024 3072 4096 6144 16384"}
PASSES=${PASSES:-1}
tmp=$(mktemp)
echo "# streams  G samples/s  ms per launch (HIP events)  fraction of HBM roofline (2.0058 B/sample)"
for pass in $(seq 1 $PASSES); do
for B in $SIZES; do
  python $R/bench.py --streams $B --steps 20 --warmup 3 --full --no-cpu-baseline --no-extra --check-streams 8 2>/dev/null | python3 -c "
import sys, json
j = json.loads(sys.stdin.read())
print('%8d  %10.1f  %10.3f  %8.4f  bit_errors_vs_cpu_ref %d' % ($B, j['value'] / 1e3, j['roofline']['kernel_ms'], j['roofline']['frac'], j['bit_errors_vs_cpu_ref']))" | tee -a $tmp || { echo "# bench.py failed at $B streams: stopping"; rm -f $tmp; exit 1; }
done
done
python3 - $tmp <<'EOF'
import sys
import numpy as np
rows = np.array([[float(v) for v in ln.split()[:3]] for ln in open(sys.argv[1]) if ln.strip()])
full = rows[rows[:, 0] >= 3072]
if len(np.unique(full[:, 0])) >= 2:
    slope, icpt = np.polyfit(full[:, 0] / 3072.0, full[:, 2], 1)
    res = full[:, 2] - (icpt + slope * full[:, 0] / 3072.0)
    spread = max(rows[rows[:, 0] == b, 2].max() - rows[rows[:, 0] == b, 2].min() for b in np.unique(rows[:, 0]))
    print("# fit over B >= 3072 (%d launches): t = %.3f ms + %.3f ms x (B / 3072); residual rms %.3f ms; largest pass-to-pass spread of a size %.3f ms"
          % (len(full), icpt, slope, float(np.sqrt((res ** 2).mean())), spread))
EOF
rm -f $tmp
