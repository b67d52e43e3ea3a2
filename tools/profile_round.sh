#!/bin/bash
# Round profile: rocprofv3 kernel-trace stats of the contract bench with all its legs (--full), plus separate PMC
# passes (FETCH_SIZE, WRITE_SIZE) for the HBM traffic of the head kernel.  Writes OUTDIR/prof_* and OUTDIR/pmc_*;
# tools/profile_collect.py turns them into profiles/<round>_*.{csv,json}.
#   usage: bash tools/profile_round.sh [ROUND [OUTDIR]]   (OUTDIR defaults to bench_out)
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
R=${1:-r01}
O=${2:-bench_out}
mkdir -p $O
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof_$R -o bench --output-format csv -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu > $O/prof_$R.log 2>&1 || { echo "kernel-trace pass failed"; tail -20 $O/prof_$R.log; exit 1; }
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 600 rocprofv3 --pmc $C --kernel-include-regex "SrcHead|SrcTail|scatter_items|tail_counts|panda_validate|panda_sphere_fk" -d $O/pmc_${R}_$C -o pmc --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu > $O/pmc_${R}_$C.log 2>&1 || { echo "pmc $C failed"; tail -20 $O/pmc_${R}_$C.log; exit 1; }
done
echo done
