# Two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE -- separate runs, TCC slots) of a
# short eager bench, then the per-ls_conv2d-call HBM traffic -> profiles/pmc_traffic.json
# usage: bash scripts/pmc_pass.sh TAG [windows per UNet call, default 48 = bench.py's configs[1]]
set -o pipefail
tag=${1:-pmc}
nw=${2:-48}
export TMPDIR=/tmp
OUT=${OUT:-bench_out}  # where the logs and traces go
mkdir -p $OUT
B="scripts/pmc_step.py $nw 3"
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 240 rocprofv3 --pmc $c --output-format csv -d $OUT/${tag}_$c -o run -- python3 $B > $OUT/${tag}_$c.log 2>&1
  rc=$?; echo "pmc $c rc=$rc"; [ $rc -ne 0 ] && { tail -5 $OUT/${tag}_$c.log; exit $rc; }
done
python3 scripts/pmc_traffic.py $OUT/${tag}_FETCH_SIZE $OUT/${tag}_WRITE_SIZE $OUT/${tag}_traffic.json
python3 scripts/pmc_per_kernel.py $OUT/${tag}_FETCH_SIZE $OUT/${tag}_WRITE_SIZE 60 > $OUT/${tag}_per_kernel.txt
