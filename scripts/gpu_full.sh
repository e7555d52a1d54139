#!/bin/bash
# GPU-box round check: gpu tests -> bench (default config) -> rocprofv3 kernel stats of a short bench.
# Stops at the first failure; every GPU step has its own time limit.
# usage: bash scripts/gpu_full.sh TAG [bench args...]
set -o pipefail
tag=${1:-run}; shift
OUT=${OUT:-bench_out}  # where the logs and traces go
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -x -v -m gpu --timeout 120 --timeout-method thread > $OUT/${tag}_tests.log 2>&1
rc=$?; echo "pytest rc=$rc"; grep -E "passed|failed|error" $OUT/${tag}_tests.log | tail -5
[ $rc -ne 0 ] && exit $rc
timeout -k 10 600 python -u bench.py --full "$@" > $OUT/${tag}_bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -2 $OUT/${tag}_bench.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${tag}_prof -o run -- python3 -u bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-single-window "$@" > $OUT/${tag}_prof.log 2>&1
rc=$?; echo "rocprof rc=$rc"; tail -1 $OUT/${tag}_prof.log
exit $rc
