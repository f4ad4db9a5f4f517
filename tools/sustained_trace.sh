#!/bin/bash
# Kernel trace of the bench's 10 s sustained loop (per-step composition of the late regime: k_cadmm, the
# concurrent tail launch, the hand-over tail launch).  Output under $OUT/sust_kt (default: diag/ in the repository).
set -u
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/diag}
mkdir -p $OUT
# (--full: the sustained loop runs after the timed steps)
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/sust_kt -o run --output-format csv -- python3 $R/bench.py --full --no-cpu-baseline --steps 5 --warmup 1 > $OUT/sust_kt.log 2>&1 || exit 12
echo done
