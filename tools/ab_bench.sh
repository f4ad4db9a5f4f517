#!/bin/bash
# A/B timing of differently compiled builds of libdat.so (build_var/libdat_<name>.so) on the C4
# bench (run on a GPU machine): ROUNDS (default 1) alternating rounds over VARIANTS, one short
# bench per variant and round, one summary line each.  The first failing bench ends the script.
#   VARIANTS="parent head" ROUNDS=3 tools/ab_bench.sh
# FULL=1: the bench's --full run without the CPU baseline (metrics step and sustained loop) instead of the
# plain timed steps; BENCH_ARGS: further bench.py arguments (e.g. --config C2); AB_OUT: directory of the
# per-run logs (default bench_out); DUMP=1: every run also writes its --dump-outputs arrays to
# $AB_OUT/<tag>_<variant>_r<round>/ (tools/same_dumps.py compares them bitwise).
set -u
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R && mkdir -p gpurun_out
export PYTHONUNBUFFERED=1
MODE_ARG=""; [ "${FULL:-0}" = "1" ] && MODE_ARG="--full --no-cpu-baseline"
TAG=${TAG:-ab}
OUT=${AB_OUT:-bench_out}
mkdir -p $OUT
for r in $(seq 1 ${ROUNDS:-1}); do
  for v in ${VARIANTS:-base}; do
    log=$OUT/${TAG}_${v}_r$r.log
    DUMP_ARG=""; [ "${DUMP:-0}" = "1" ] && DUMP_ARG="--dump-outputs $OUT/${TAG}_${v}_r$r"
    DAT_LIB_PATH=$R/build_var/libdat_$v.so timeout -k 10 ${BENCH_TIMEOUT:-200} python -u bench.py $MODE_ARG --steps ${STEPS:-6} --warmup ${WARMUP:-2} ${BENCH_ARGS:-} $DUMP_ARG > $log 2>&1 || { echo "$v round $r failed"; tail -5 $log; exit 11; }
    python - "$v" "$r" $log <<'PY' || exit 12
import json, sys
line = [l for l in open(sys.argv[3]) if l.startswith('{')][-1]
j = json.loads(line)
roof, st = j.get('roofline') or {}, j.get('stats') or {}
print(f"{sys.argv[1]:>12} r{sys.argv[2]}: {j['ms_per_step']:.4f} ms/step  {roof.get('kernel', 'kernel')} "
      f"{roof.get('launch_ms', float('nan')):.4f} ms  {j['value']/1e6:.2f} M QP/s  "
      f"ipm/qp {st.get('mean_ipm_iters_per_qp', float('nan')):.3f}")
PY
  done
done
