#!/bin/bash
# GPU-box check: parity tests, smoke, short bench.  Stops at the first crash/timeout.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out}   # results directory
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -q -rA > $OUT/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc" | tee -a $OUT/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stopping after pytest crash/timeout"; exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full --steps 5 --warmup 1 --cpu-seconds 10 > $OUT/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; exit $rc
