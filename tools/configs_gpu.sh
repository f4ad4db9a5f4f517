#!/bin/bash
# GPU round trip for the SURVEY.md 8(d) QP-level configs: parity tests, then one bench line per config.
# Logs go to $OUT (default: diag/ in the repository).
set -u
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/diag}
cd $R && mkdir -p $OUT
export PYTHONUNBUFFERED=1
if [ "${TESTS:-1}" = "1" ]; then
  timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { tail -40 $OUT/gpu_tests.log; exit 11; }
  tail -3 $OUT/gpu_tests.log
fi
# (--full: the metrics step and the CPU baseline next to the timed steps)
for c in C2 C3 C5; do
  timeout -k 10 240 python -u bench.py --full --config $c --cpu-sample-s ${CPU_S:-10} > $OUT/bench_$c.log 2>&1 || { tail -20 $OUT/bench_$c.log; exit 12; }
  grep '^{' $OUT/bench_$c.log
done
for c in C2 C5; do
  timeout -k 10 240 python -u bench.py --full --config $c --fixed-work --no-cpu-baseline > $OUT/bench_${c}_fw.log 2>&1 || { tail -20 $OUT/bench_${c}_fw.log; exit 13; }
  grep '^{' $OUT/bench_${c}_fw.log
done
echo done
