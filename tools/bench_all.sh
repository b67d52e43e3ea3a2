#!/bin/bash
# Every bench.py workload once (the contract headline with all its legs, --full, and BASELINE configs[2..4]), one
# GPU box.   usage: bash tools/bench_all.sh [TAG [OUTDIR]]   (OUTDIR defaults to bench_out)
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R=${1:-r01}
O=${2:-bench_out}
mkdir -p $O
for w in validate capt fetch_prm prm_edges pair rrtc; do
  timeout -k 10 300 python bench.py --full --workload $w --steps 10 --warmup 2 > $O/bench_${R}_$w.json 2> $O/bench_${R}_$w.err || { echo "bench $w failed"; tail -20 $O/bench_${R}_$w.err; exit 1; }
  cat $O/bench_${R}_$w.json
done
