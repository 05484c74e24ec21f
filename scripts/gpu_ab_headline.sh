#!/bin/bash
# GPU-box: the default bench alternated between the tree's library and a scratch_libs/ variant
# (A B A B), no CPU baseline / host-to-host; prints value and the isolated k_n4_study launch.
# usage: scripts/gpu_ab_headline.sh TAG LIB_B
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out}   # results directory
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=$1; B=$2
for lib in A B A B; do
  if [ $lib = A ]; then L=vent_analysis_amd/libventhip.so; else L=scratch_libs/$B.so; fi
  VH_LIB_PATH=$L timeout -k 10 300 python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-h2h \
      > $OUT/${TAG}_$lib.json 2> $OUT/${TAG}_$lib.err
  rc=$?; [ $rc -eq 0 ] || { echo "$lib rc=$rc"; tail -3 $OUT/${TAG}_$lib.err; exit $rc; }
  python3 -c "import json,sys; d=json.loads(open(sys.argv[1]).read().splitlines()[-1]); r=d['roofline']; print(sys.argv[2], d['value'], d['ms_per_step'], 'iso', r['avg_launch_us'], 'study mean', d['n4_study_times']['mean_us'], 'sort', r['kernel_us_per_launch'].get('sort'), 'non_n4', r.get('non_n4_us_per_step'))" $OUT/${TAG}_$lib.json $lib
done
