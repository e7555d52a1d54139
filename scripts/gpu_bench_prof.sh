set -o pipefail
OUT=${OUT:-bench_out}  # where the logs and traces go
mkdir -p $OUT
timeout -k 10 600 python -u bench.py --full > $OUT/r03p_bench.log 2>&1; rc=$?; tail -1 $OUT/r03p_bench.log | cut -c1-150; [ $rc -ne 0 ] && exit $rc
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/r03p_prof -o run -- python3 -u bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-single-window > $OUT/r03p_prof.log 2>&1 || exit 1
bash scripts/pmc_pass.sh r03p 48 > $OUT/r03p_pmc.log 2>&1; rc=$?; grep hbm_bytes $OUT/r03p_traffic.json; exit $rc
