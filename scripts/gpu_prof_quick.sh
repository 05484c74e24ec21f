#!/bin/bash
# GPU-box: rocprofv3 kernel trace + stats of a short default bench (no CPU baseline / host-to-host);
# extra arguments go to bench.py.  usage: scripts/gpu_prof_quick.sh TAG [bench args...]
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out}   # results directory
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=$1; shift
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-h2h "$@" > $OUT/prof_$TAG.json 2> $OUT/prof_$TAG.err
rc=$?; echo "rc=$rc"; [ $rc -eq 0 ] || { tail -5 $OUT/prof_$TAG.err; exit $rc; }
f=$(find $OUT/prof_$TAG -name '*kernel_stats.csv' | head -1)
cp "$f" $OUT/${TAG}_kernel_stats.csv
python3 -c "
import csv,sys
for r in list(csv.DictReader(open(sys.argv[1])))[:24]: print('%-60s %6s %12.1f' % (r['Name'][:60], r['Calls'], float(r['AverageNs'])/1e3))" $OUT/${TAG}_kernel_stats.csv
